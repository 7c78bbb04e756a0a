"""grouped_gemm_mx_decode on the MI355X against a plain per-expert fp64 matmul, as tests/test_grouped_gemm_mx_gpu.py
tests grouped_gemm_mx: hand-built codes whose every partial sum is exact in fp32 must come out bit for bit -- whatever
the split of the contraction over the waves and the order of their partial sums -- and real pairs within the derived
bound.  K = 128 / 640 / 1152 is 1 step (three idle waves), 5 (an uneven split) and 9."""
import functools

import pytest
import torch

from tests.mx_ref import MX, mx_back_ref
from tests.test_grouped_gemm_mx_gpu import BACK, FORMATS, cuda, exact_in_fp32, exact_pair, layout

pytestmark = pytest.mark.gpu

COUNTS = (16, 1, 0, 40, 17)      # a full tile, one valid row, an empty expert sharing its start, 2.5 tiles, a ragged end
pair_of = functools.lru_cache(maxsize=None)(exact_pair)


def fprop_ref(a, b, align, counts=COUNTS, bound=False):
    """fp64 [N, O] of a [>= N, K] and b [E, O, K]: zeros on the padding rows; bound: K * 2^-23 * sum |a||b|."""
    starts, ends, N = layout(counts, align)
    out = torch.zeros((N, b.shape[1]), dtype=torch.float64)
    for e, (s, t) in enumerate(zip(starts, ends)):
        out[s:t] = a[s:t].abs() @ b[e].abs().T * a.shape[1] * 2.0 ** -23 if bound else a[s:t] @ b[e].T
    return out


def ends_tensor(align):
    return torch.tensor(layout(COUNTS, align)[1], dtype=torch.int32, device='cuda')


def check_exact(fa, fb, K, O, align):
    import deepep_amd
    E, N = len(COUNTS), layout(COUNTS, align)[2]
    a, av = pair_of(fa, N, K, 1)
    b, bv = pair_of(fb, E * O, K, 2)
    exact_in_fp32(av, bv)
    ref = fprop_ref(av, bv.view(E, O, K), align)
    args = (cuda(a), cuda(b, (E, O)), ends_tensor(align))
    out32 = deepep_amd.grouped_gemm_mx_decode(*args, expert_alignment=align, out_dtype=torch.float32)
    out16 = deepep_amd.grouped_gemm_mx_decode(*args, expert_alignment=align)
    assert torch.equal(out32.cpu().double(), ref)
    assert torch.equal(out16.cpu().double(), ref.float().to(torch.bfloat16).double())


@pytest.mark.parametrize('O', [64, 192])
@pytest.mark.parametrize('K', [128, 640, 1152])
@pytest.mark.parametrize('fb', FORMATS)
@pytest.mark.parametrize('fa', FORMATS)
def test_exact_sums_are_bitwise(fa, fb, K, O):
    check_exact(fa, fb, K, O, 16)


@pytest.mark.parametrize('fa,fb', [('fp8', 'fp4')])
def test_exact_sums_at_alignment_32(fa, fb):
    check_exact(fa, fb, 640, 64, 32)


@pytest.mark.parametrize('fmt', FORMATS)
def test_real_pairs_within_the_derived_bound(fmt):
    import deepep_amd
    cast = {'fp8': lambda t: deepep_amd.per_token_cast_to_fp8(t, True, True, group_size=32),
            'fp4': deepep_amd.per_token_cast_to_fp4, 'fp6': deepep_amd.per_token_cast_to_fp6}[fmt]
    E, K, O, N = len(COUNTS), 640, 192, layout(COUNTS, 16)[2]
    g = torch.Generator().manual_seed(5)
    a = cast(torch.randn((N, K), generator=g).to(torch.bfloat16).cuda())
    b = cast((torch.randn((E * O, K), generator=g) * K ** -0.5).to(torch.bfloat16).cuda())
    av, bv = BACK[fmt](*a).double(), BACK[fmt](*b).double().view(E, O, K)
    ref, bound = fprop_ref(av, bv, 16), fprop_ref(av, bv, 16, bound=True)
    args = (a, tuple(t.view(E, O, -1) for t in b), ends_tensor(16))
    for dtype, extra in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
        out = deepep_amd.grouped_gemm_mx_decode(*args, expert_alignment=16, out_dtype=dtype).cpu().double()
        err = (out - ref).abs()
        print(f'{fmt} {dtype}: largest error / (K 2^-23 S) = {float((err / bound)[bound > 0].max()):.4f}')
        assert bool((err <= bound + extra * ref.abs()).all())


def test_stays_inside_its_rows_of_a_worst_case_handle(monkeypatch):
    from deepep_amd.kernels import HipKernels
    from tests import guard as guard_module
    monkeypatch.setitem(guard_module.OUTPUTS, 'grouped_gemm_mx_decode', ('out',))
    guard = guard_module.Guard(HipKernels())
    E, K, O = len(COUNTS), 640, 64
    starts, ends, used = layout(COUNTS, 16)
    N = used + 32                                # two tiles past the last expert; formats: _lib.MX_FP6 = 2, MX_FP4 = 4
    (aq, asf), av = pair_of('fp6', used, K, 21)
    (bq, bsf), bv = pair_of('fp4', E * O, K, 22)
    a = torch.full((N, aq.shape[1]), 0xff, dtype=torch.uint8)   # NaN-scaled garbage on every row that is not valid
    a_sf = torch.full((N, K // 32), 0xff, dtype=torch.uint8)
    for s, t in zip(starts, ends):
        a[s:t], a_sf[s:t] = aq[s:t], asf[s:t]
    out = torch.full((N, O), 7.0, dtype=torch.float32, device='cuda')
    guard.grouped_gemm_mx_decode(2, 4, a.cuda(), a_sf.cuda(), bq.cuda(), bsf.cuda(), ends_tensor(16), 16, out)
    assert guard.verify() >= 1
    assert torch.equal(out[:used].cpu().double(), fprop_ref(av, bv.view(E, O, K), 16))
    assert bool((out[used:] == 7.0).all())


def test_dispatch_gemm_combine_at_one_rank():
    """The chain over the handle's own tensor, against the same chain with the fp64 matmul rounded to bf16 between."""
    import deepep_amd
    from tests.test_cast_keyword_gpu import _group1, _inputs
    T, H, K_top, E, O = 64, 256, 2, 4, 64
    x, idx, w = _inputs(7, T, H, K_top, E)
    buf = deepep_amd.ElasticBuffer(_group1(), num_max_tokens_per_rank=T, hidden=H, num_topk=K_top)
    pair, _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True,
                                            expert_alignment=16, do_zero_padding=True, **MX)
    ends = handle.psum_num_recv_tokens_per_expert
    g = torch.Generator().manual_seed(8)
    wq = deepep_amd.per_token_cast_to_fp8((torch.randn((E * O, H), generator=g) * H ** -0.5).to(torch.bfloat16).cuda(),
                                          True, True, group_size=32)
    y = deepep_amd.grouped_gemm_mx_decode(pair, tuple(t.view(E, O, -1) for t in wq), ends, expert_alignment=16)
    ends_l = ends.cpu().tolist()
    counts = [t - (0 if e == 0 else (ends_l[e - 1] + 15) // 16 * 16) for e, t in enumerate(ends_l)]
    used = layout(counts, 16)[2]
    assert sum(counts) > 0 and used <= y.shape[0]
    av, bv = mx_back_ref(*pair).double()[:used], mx_back_ref(*wq).double().view(E, O, H)
    ref, bound = fprop_ref(av, bv, 16, counts), fprop_ref(av, bv, 16, counts, bound=True)
    err = (y[:used].cpu().double() - ref).abs()
    assert bool((err <= bound + 2.0 ** -8 * ref.abs()).all())
    y_ref = y.clone()
    y_ref[:used] = ref.to(torch.bfloat16).cuda()
    out, _, _ = buf.combine(y, handle, topk_weights=ex_w)
    out_ref, _, _ = buf.combine(y_ref, handle, topk_weights=ex_w)
    assert not torch.equal(y.view(torch.int16), y_ref.view(torch.int16)) or torch.equal(out, out_ref)
    # K_top rows a token, each off by what the GEMM is off, and one bf16 rounding of the sum on either side
    delta = K_top * float((y[:used].double() - y_ref[:used].double()).abs().max())
    assert bool(((out.double() - out_ref.double()).abs() <= delta + 2.0 ** -7 * out_ref.double().abs()).all())


def test_it_captures_into_a_graph():
    import deepep_amd
    E, N, K, O = len(COUNTS), layout(COUNTS, 16)[2], 640, 64
    a, b = cuda(pair_of('fp8', N, K, 9)[0]), cuda(pair_of('fp6', E * O, K, 10)[0], (E, O))
    ends = ends_tensor(16)
    eager = deepep_amd.grouped_gemm_mx_decode(a, b, ends)
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            got = deepep_amd.grouped_gemm_mx_decode(a, b, ends)
        for _ in range(2):
            got.fill_(float('nan'))
            graph.replay()
            stream.synchronize()
            assert torch.equal(got, eager)
