"""grouped_gemm_mx / grouped_gemm_mx_wgrad on the MI355X against a plain per-expert fp64 matmul of the operands as the
CPU cast-back references dequantise them.  The sharp tests are the exact ones: hand-built codes (integer magnitudes,
exponent bytes 125..129) whose every partial sum is exact in fp32, so the output must equal the reference bit for bit,
which no wrong lane, K block, nibble, FP6 bit or scale-byte assignment survives."""
import pytest
import torch

from tests.fp4_ref import E2M1_VALUES, fp4_back_ref, fp4_pack
from tests.fp6_ref import E2M3_VALUES, fp6_back_ref, fp6_pack
from tests.mx_ref import MX, mx_back_ref

pytestmark = pytest.mark.gpu

FORMATS = ('fp8', 'fp4', 'fp6')
BACK = {'fp8': mx_back_ref, 'fp4': fp4_back_ref, 'fp6': fp6_back_ref}
COUNTS, ALIGN = (128, 1, 0, 200), 128           # a full segment, one valid row, an empty expert, a ragged one
MAGNITUDES = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0, 6.0])     # integers every format holds


def layout(counts=COUNTS, align=ALIGN):          # (starts, ends, N) of the expanded layout dispatch_scan gives
    starts, ends, at = [], [], 0
    for c in counts:
        starts.append(at)
        ends.append(at + c)
        at = (at + c + align - 1) // align * align
    return starts, ends, at


def exact_pair(fmt, rows, C, seed, keep=None):
    """A hand-built pair over [rows, C] and its fp64 values; keep: a bool [C] mask of the columns that are not zero."""
    g = torch.Generator().manual_seed(seed)
    mag = MAGNITUDES[torch.randint(0, 6, (rows, C), generator=g)]
    if keep is not None:
        mag = mag * keep
    neg = torch.randint(0, 2, (rows, C), generator=g).bool()
    sf = torch.randint(125, 130, (rows, C // 32), generator=g).to(torch.uint8)
    if fmt == 'fp8':
        q = torch.where(neg, -mag, mag).to(torch.float8_e4m3fn)
    else:
        table, sign, pack = ((E2M1_VALUES, 8, fp4_pack) if fmt == 'fp4' else (E2M3_VALUES, 32, fp6_pack))
        code = torch.tensor([table.index(v) for v in MAGNITUDES.tolist()], dtype=torch.uint8)[
            torch.bucketize(mag, MAGNITUDES)]
        q = pack(code | (neg.to(torch.uint8) * sign))
    return (q, sf), BACK[fmt](q, sf).double()


def cuda(pair, lead=None):
    return tuple(t.cuda() if lead is None else t.cuda().view(*lead, -1) for t in pair)


def fprop_ref(a, b, counts=COUNTS, bound=False):
    """fp64 [N, O] of a [N, K] and b [E, O, K]: the per-expert matmul, zeros on the padding rows.  bound: of the
    magnitudes, times K * 2^-23 -- K additions, each off by at most one fp32 ulp of a partial sum below S."""
    starts, ends, N = layout(counts)
    out = torch.zeros((N, b.shape[1]), dtype=torch.float64)
    for e, (s, t) in enumerate(zip(starts, ends)):
        out[s:t] = a[s:t].abs() @ b[e].abs().T * a.shape[1] * 2.0 ** -23 if bound else a[s:t] @ b[e].T
    return out


def wgrad_ref(dy, x):
    return torch.stack([dy[:, s:t] @ x[:, s:t].T for s, t in zip(*layout()[:2])])


def ends_tensor():
    return torch.tensor(layout()[1], dtype=torch.int32, device='cuda')


def exact_in_fp32(a, b):                        # every partial sum of |a||b| is below 2^22 units of 2^-4
    assert float((a.abs() @ b.abs().T).max()) * 16 < 2 ** 22


@pytest.mark.parametrize('O', [128, 256])
@pytest.mark.parametrize('K', [128, 384])
@pytest.mark.parametrize('fb', FORMATS)
@pytest.mark.parametrize('fa', FORMATS)
def test_exact_sums_are_bitwise(fa, fb, K, O):
    import deepep_amd
    E, N = len(COUNTS), layout()[2]
    a, av = exact_pair(fa, N, K, 1)
    b, bv = exact_pair(fb, E * O, K, 2)
    exact_in_fp32(av, bv)
    ref = fprop_ref(av, bv.view(E, O, K))
    args = (cuda(a), cuda(b, (E, O)), ends_tensor())
    out32 = deepep_amd.grouped_gemm_mx(*args, expert_alignment=ALIGN, out_dtype=torch.float32)
    out16 = deepep_amd.grouped_gemm_mx(*args, expert_alignment=ALIGN)
    assert torch.equal(out32.cpu().double(), ref)               # equal values are equal bits, but for a zero's sign
    assert torch.equal(out16.cpu().double(), ref.float().to(torch.bfloat16).double())


def token_mask(N):
    keep = torch.zeros(N, dtype=torch.bool)
    for s, t in zip(*layout()[:2]):
        keep[s:t] = True
    return keep


@pytest.mark.parametrize('H', [128, 256])
@pytest.mark.parametrize('O', [128, 256])
@pytest.mark.parametrize('fa,fb', [('fp8', 'fp8'), ('fp4', 'fp4'), ('fp6', 'fp6'), ('fp8', 'fp4')])
def test_exact_sums_of_the_wgrad_schedule_are_bitwise(fa, fb, O, H):
    import deepep_amd
    N = layout()[2]
    dy, dyv = exact_pair(fa, O, N, 3, token_mask(N))            # zero codes on every padding token
    x, xv = exact_pair(fb, H, N, 4, token_mask(N))
    exact_in_fp32(dyv, xv)
    out = deepep_amd.grouped_gemm_mx_wgrad(cuda(dy), cuda(x), ends_tensor(), expert_alignment=ALIGN)
    assert out.dtype == torch.float32 and torch.equal(out.cpu().double(), wgrad_ref(dyv, xv))
    assert not out[2].any()                                     # the expert without rows


@pytest.mark.parametrize('fmt', FORMATS)
def test_real_pairs_within_the_derived_bound(fmt):
    import deepep_amd
    cast = {'fp8': lambda t: deepep_amd.per_token_cast_to_fp8(t, True, True, group_size=32),
            'fp4': deepep_amd.per_token_cast_to_fp4, 'fp6': deepep_amd.per_token_cast_to_fp6}[fmt]
    E, K, O = len(COUNTS), 384, 256
    N = layout()[2]
    g = torch.Generator().manual_seed(5)
    a = cast(torch.randn((N, K), generator=g).to(torch.bfloat16).cuda())
    b = cast((torch.randn((E * O, K), generator=g) * K ** -0.5).to(torch.bfloat16).cuda())
    av, bv = BACK[fmt](*a).double(), BACK[fmt](*b).double().view(E, O, K)
    ref, bound = fprop_ref(av, bv), fprop_ref(av, bv, bound=True)
    args = (a, tuple(t.view(E, O, -1) for t in b), ends_tensor())
    for dtype, extra in ((torch.float32, 0.0), (torch.bfloat16, 2.0 ** -8)):
        out = deepep_amd.grouped_gemm_mx(*args, expert_alignment=ALIGN, out_dtype=dtype).cpu().double()
        err = (out - ref).abs()
        print(f'{fmt} {dtype}: largest error / (K 2^-23 S) = {float((err / bound)[bound > 0].max()):.4f}')
        assert bool((err <= bound + extra * ref.abs()).all())


def test_dispatch_gemm_combine_at_one_rank():
    """The chain over the handle's own tensor, against the same chain with the fp64 matmul rounded to bf16 between."""
    import deepep_amd
    from tests.test_cast_keyword_gpu import _group1, _inputs
    T, H, K_top, E, O = 64, 256, 2, 4, 128
    x, idx, w = _inputs(7, T, H, K_top, E)
    buf = deepep_amd.ElasticBuffer(_group1(), num_max_tokens_per_rank=T, hidden=H, num_topk=K_top)
    pair, _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True,
                                            expert_alignment=128, do_zero_padding=True, **MX)
    ends = handle.psum_num_recv_tokens_per_expert
    g = torch.Generator().manual_seed(8)
    wq = deepep_amd.per_token_cast_to_fp8((torch.randn((E * O, H), generator=g) * H ** -0.5).to(torch.bfloat16).cuda(),
                                          True, True, group_size=32)
    y = deepep_amd.grouped_gemm_mx(pair, tuple(t.view(E, O, -1) for t in wq), ends, expert_alignment=128)
    ends_l = ends.cpu().tolist()
    counts = [t - (0 if e == 0 else (ends_l[e - 1] + 127) // 128 * 128) for e, t in enumerate(ends_l)]
    used = layout(counts)[2]
    assert sum(counts) > 0 and used <= y.shape[0]
    av, bv = mx_back_ref(*pair).double()[:used], mx_back_ref(*wq).double().view(E, O, H)
    ref, bound = fprop_ref(av, bv, counts), fprop_ref(av, bv, counts, bound=True)
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


def test_both_schedules_capture_into_a_graph():
    import deepep_amd
    E, N, K, O = len(COUNTS), layout()[2], 256, 128
    a, b = cuda(exact_pair('fp8', N, K, 9)[0]), cuda(exact_pair('fp6', E * O, K, 10)[0], (E, O))
    dy, x = (cuda(exact_pair(f, rows, N, 11, token_mask(N))[0]) for f, rows in (('fp4', O), ('fp8', K)))
    ends = ends_tensor()
    eager = (deepep_amd.grouped_gemm_mx(a, b, ends), deepep_amd.grouped_gemm_mx_wgrad(dy, x, ends))
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            got = (deepep_amd.grouped_gemm_mx(a, b, ends), deepep_amd.grouped_gemm_mx_wgrad(dy, x, ends))
        for _ in range(2):
            for t in got:
                t.fill_(float('nan'))
            graph.replay()
            stream.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(got, eager))


@pytest.fixture
def guard(monkeypatch):
    """Canary bands around the output (tests/guard.py); the mixin's wrapper is declared for the test's duration."""
    from deepep_amd.kernels import HipKernels
    from tests import guard as guard_module
    monkeypatch.setitem(guard_module.OUTPUTS, 'grouped_gemm_mx', ('out',))
    return guard_module.Guard(HipKernels())


def test_fprop_stays_inside_its_rows_of_a_worst_case_handle(guard):
    E, used, K, O = len(COUNTS), layout()[2], 128, 256
    N = used + 256                               # two tiles past the last expert; formats: _lib.MX_FP6 = 2, MX_FP4 = 4
    (aq, asf), av = exact_pair('fp6', used, K, 21)
    (bq, bsf), bv = exact_pair('fp4', E * O, K, 22)
    a = torch.full((N, aq.shape[1]), 0xff, dtype=torch.uint8)   # NaN-scaled garbage behind the valid rows
    a_sf = torch.full((N, K // 32), 0xff, dtype=torch.uint8)
    a[:used], a_sf[:used] = aq, asf
    out = torch.full((N, O), 7.0, dtype=torch.float32, device='cuda')
    guard.grouped_gemm_mx(False, 2, 4, a.cuda(), a_sf.cuda(), bq.cuda(), bsf.cuda(), ends_tensor(), ALIGN, out)
    assert guard.verify() >= 1
    assert torch.equal(out[:used].cpu().double(), fprop_ref(av, bv.view(E, O, K)))
    assert bool((out[used:] == 7.0).all())


def test_wgrad_stays_inside_its_output(guard):
    E, N, O, H = len(COUNTS), layout()[2], 256, 128
    dy, dyv = exact_pair('fp8', O, N, 23, token_mask(N))
    x, xv = exact_pair('fp6', H, N, 24, token_mask(N))
    out = torch.empty((E, O, H), dtype=torch.float32, device='cuda')
    guard.grouped_gemm_mx(True, 0, 2, *cuda(dy), *cuda(x), ends_tensor(), ALIGN, out)
    assert guard.verify() >= 1
    assert torch.equal(out.cpu().double(), wgrad_ref(dyv, xv))
