"""MXFP6 (e2m3 rows, 32 codes to 24 bytes, one UE8M0 exponent byte per 32 columns) on the GPU, bitwise: the cast
(deepep_cast_fp6_mx, both store widths) against tests/fp6_ref.fp6_pair, over every finite bf16 bit pattern with the
group's pin in each of its 32 columns (which also pins the order of the codes); the cast back (deepep_cast_back_fp6_mx)
against tests/fp6_ref.fp6_back_ref, over every code in every position; and dispatch(..., cast_to_fp6=True) against the
same build's tuple dispatch of fp6_pair(x) -- at EP = 1 (the casting copy), over 4 thread ranks (the casting pack:
local bypass on / off, the padded exchange) and over xGMI windows in two processes.  Thread ranks and processes are
started and time-limited as in tests/test_mx_gpu.py."""
import os
import sys
import threading
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fp6_ref import FP6, fp6_back_ref, fp6_cases, fp6_pack, fp6_pair, fp6_unpack
from tests.test_cast_keyword_gpu import _free_port, _group1
from tests.test_fp8_cast_gpu import _same
from tests.test_mx_gpu import _buffer, _mx_inputs
from tests.ue8m0_ref import packed_differences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BF16_MAX = torch.finfo(torch.bfloat16).max


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


# ----------------------------------------------------------------------------- the cast
def _cast_input(T: int, H: int) -> torch.Tensor:
    """tests/test_fp4_gpu._cast_input for 7.5 in place of 6: in every row, group 0 below the 1e-4 clamp (row 0: all
    zeros), group 1 with amax an exact power of two times 7.5 (the mantissa-zero branch of the ceiling), group 2 with
    the largest finite bf16; the other groups random over +-20 binades."""
    g = torch.Generator().manual_seed(T * 10007 + H)
    x = torch.randn((T, H), generator=g) * torch.exp2(torch.randint(-20, 20, (T, H // 32, 1), generator=g).float()
                                                      ).expand(T, H // 32, 32).reshape(T, H)
    x[:, :32] = torch.randn((T, 32), generator=g) * 1e-6
    x[0, :32] = 0
    x[:, 32:64] = x[:, 32:64].clamp(-1, 1) * 2.0 ** -5
    x[:, 32 + 5] = 7.5 * torch.exp2(torch.arange(T).float() % 9 - 4)
    x[:, 64:96] = x[:, 64:96].clamp(-1, 1)
    x[:, 64 + 29] = -BF16_MAX
    return x.to(torch.bfloat16)


def _check_cast(kern, x_cpu: torch.Tensor, x_gpu=None):
    import deepep_amd
    T, H = x_cpu.shape
    x_gpu = x_cpu.cuda() if x_gpu is None else x_gpu
    q_ref, sf_ref = fp6_pair(x_cpu)
    outs = []
    for store_bytes in (None, 8, 16):
        q = torch.full((T, 3 * H // 4), 0x5a, dtype=torch.uint8, device='cuda')          # poison
        sf = torch.full((T, H // 32), 0xee, dtype=torch.uint8, device='cuda')
        kern.cast_fp6(x_gpu, q, sf, store_bytes=store_bytes)
        outs.append((store_bytes, q, sf))
    q_pub, sf_pub = deepep_amd.per_token_cast_to_fp6(x_gpu)
    torch.cuda.synchronize()
    for store_bytes, q, sf in outs:
        bad = (sf.cpu() != sf_ref).nonzero()
        assert bad.numel() == 0, f'stores of {store_bytes}: {bad.shape[0]} exponent bytes differ, first at ' \
                                 f'{bad[0].tolist()}: {sf.cpu()[tuple(bad[0])].item()} != ' \
                                 f'{sf_ref[tuple(bad[0])].item()}'
        if not _same(q, q_ref):
            got, want = fp6_unpack(q), fp6_unpack(q_ref)
            bad = (got != want).nonzero()
            assert False, f'stores of {store_bytes}: {bad.shape[0]} codes differ, first at {bad[0].tolist()}: ' \
                          f'{got[tuple(bad[0])].item():#x} != {want[tuple(bad[0])].item():#x} for x ' \
                          f'{x_cpu[tuple(bad[0])].item()}'
    assert _same(q_pub, q_ref) and _same(sf_pub, sf_ref) and q_pub.is_contiguous() and sf_pub.is_contiguous()
    return q_ref, sf_ref


@pytest.mark.parametrize('T', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 640, 2176, 7168])  # one quad; five quads; a pass and a quad; three passes and a part
def test_fp6_cast(kern, T, H):
    x = _cast_input(T, H)
    _, exp = _check_cast(kern, x)
    assert int(exp[0, 0]) == 111 and int(exp[:, 2].max()) == 253 and int(exp.min()) >= 111
    assert int(exp[0, 1]) == 127 - 4                           # 7.5 * 2^-4: exactly a power of two, no round up


def test_fp6_cast_strided_rows_and_wrapper_rejections(kern):
    T, H = 37, 640
    x = _cast_input(T, H)
    wide = torch.zeros((T, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x.cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 64 and not view.is_contiguous()
    _check_cast(kern, x, x_gpu=view)
    xg = x.cuda()
    q = torch.zeros((T, 3 * H // 4), dtype=torch.uint8, device='cuda')
    sf = torch.full((T, H // 32), 7, dtype=torch.uint8, device='cuda')
    for what, args in (('float rows', (xg.float(), q, sf)),
                       ('H % 128 != 0', (xg[:, :96], q[:, :72], sf[:, :3])),
                       ('rows of H / 2 bytes', (xg, torch.zeros((T, H // 2), dtype=torch.uint8, device='cuda'), sf)),
                       ('the per-128 shape', (xg, q, sf[:, :H // 128].contiguous())),
                       ('fp32 scale factors', (xg, q, torch.zeros((T, H // 32), device='cuda'))),
                       ('strided scale factors', (xg, q, torch.zeros((T, H // 16), dtype=torch.uint8,
                                                                     device='cuda')[:, ::2])),
                       ('CPU outputs', (xg, q.cpu(), sf))):
        with pytest.raises(RuntimeError):
            kern.cast_fp6(*args)
    with pytest.raises(RuntimeError):
        kern.cast_fp6(xg, q, sf, store_bytes=4)
    torch.cuda.synchronize()
    assert bool((sf == 7).all()), 'a rejected call launched'


def _exhaustive_cast_input() -> torch.Tensor:
    """Every finite bf16 bit pattern, in groups whose amax is pinned by one element 7.5 * 2^k, k in (-14, -4, 0, 7,
    100): for every k the patterns of magnitude up to the pin fill the 31 other columns of a group, and the whole set
    is laid out 32 times with the pin at each column (so every pattern meets every position of the 24-byte string,
    both lanes of a pair and every byte of the dword of exponent bytes).  The patterns above 7.5 * 2^100 pin their own
    group, one to a group."""
    bits = torch.arange(65536, dtype=torch.int32)
    finite = bits[(bits & 0x7f80) != 0x7f80].to(torch.int16)
    vals = finite.view(torch.bfloat16)
    groups = []
    for k in (-14, -4, 0, 7, 100):
        pin = 7.5 * 2.0 ** k
        small = vals[vals.float().abs() <= pin]
        small = torch.cat([small, torch.zeros((-small.numel()) % 31, dtype=torch.bfloat16)]).view(-1, 31)
        for r in range(32):
            g = torch.empty((small.shape[0], 32), dtype=torch.bfloat16)
            g[:, :r] = small[:, :r]
            g[:, r] = pin
            g[:, r + 1:] = small[:, r:]
            groups.append(g)
    large = vals[vals.float().abs() > 7.5 * 2.0 ** 100]
    g = torch.zeros((large.numel(), 32), dtype=torch.bfloat16)
    g[torch.arange(large.numel()), torch.arange(large.numel()) % 32] = large
    groups.append(g)
    flat = torch.cat(groups)
    flat = torch.cat([flat, torch.zeros(((-flat.shape[0]) % 4, 32), dtype=torch.bfloat16)])
    return flat.view(-1, 128)


def test_fp6_cast_exhaustive(kern):
    x = _exhaustive_cast_input()
    seen = torch.zeros(65536, dtype=torch.bool)
    seen[x.view(torch.int16).to(torch.int32).view(-1) & 0xffff] = True
    assert int(seen.sum()) == 65536 - 256                      # every finite pattern
    q_ref, sf_ref = _check_cast(kern, x)
    assert int(sf_ref.min()) >= 111 and int(sf_ref.max()) == 253
    codes = fp6_unpack(q_ref)
    assert bool((codes == 0x20).any()) and bool((codes == 0x3f).any()) and bool((codes == 0x1f).any())
    # the pin's code 31 was seen in each of the 32 positions: the order of the codes is pinned
    assert sorted(set(((codes & 31) == 31).nonzero()[:, 1].remainder(32).tolist())) == list(range(32))


# ----------------------------------------------------------------------------- the cast back
EXPONENTS = (0, 1, 111, 127, 128, 253, 254)            # byte 0: the factor +0.0f, signed zeros


def _bytes(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))


def _rows(codes: np.ndarray) -> torch.Tensor:
    return fp6_pack(_bytes(codes))


def _check_back(q_cpu, sf_cpu, q_gpu=None, sf_gpu=None):
    """per_token_cast_back_fp6 on the GPU == fp6_back_ref on the CPU, bit for bit (no code is a NaN; products past the
    largest fp32 are infinities on both sides)."""
    import deepep_amd
    q_gpu = q_cpu.cuda() if q_gpu is None else q_gpu
    sf_gpu = sf_cpu.cuda() if sf_gpu is None else sf_gpu
    out = deepep_amd.per_token_cast_back_fp6(q_gpu, sf_gpu)
    torch.cuda.synchronize()
    ref = fp6_back_ref(q_cpu, sf_cpu)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == ref.shape
    got = out.cpu()
    bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} values differ, first at {bad[0].tolist()}: ' \
                             f'{got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}'
    return ref


def test_fp6_cast_back_exhaustive():
    """All 64 codes in each of the 32 positions of each group of a 128-column row, against each exponent byte: seven
    blocks of 64 rows; in a block a group keeps one exponent while each of its columns runs through all 64 codes; over
    the blocks every group of the row (all four byte positions of the dword) meets every exponent."""
    n, H = len(EXPONENTS), 128
    r, c = np.arange(64 * n).reshape(-1, 1), np.arange(H).reshape(1, -1)
    q = _rows((r + c) % 64)
    exp = np.asarray(EXPONENTS, dtype=np.uint8)[(r // 64 + np.arange(H // 32).reshape(1, -1)) % n]
    ref = _check_back(q, _bytes(exp))
    zero = ref[:64, :32].view(torch.int16)                     # block 0, group 0: exponent byte 0
    assert bool(((zero == 0) | (zero == -32768)).all()) and bool((zero == -32768).any())
    # block 3, group 0, exponent 127 = 2^0: row 3 * 64 holds code c in column c
    assert ref[3 * 64, 8].item() == 1.0 and ref[3 * 64, 31].item() == 7.5 and ref[3 * 64 + 32, 31].item() == -7.5


@pytest.mark.parametrize('M', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 640, 2176, 7168])
def test_fp6_cast_back_shapes(M, H):
    rng = np.random.default_rng(M * 10007 + H)
    codes = rng.integers(0, 64, size=(M, H), dtype=np.uint8)
    exp = np.asarray(EXPONENTS[1:6], dtype=np.uint8)[rng.integers(0, 5, size=(M, H // 32))]
    _check_back(_rows(codes), _bytes(exp))


def test_fp6_cast_back_of_the_cast_equals_the_reference():
    import deepep_amd
    x = _cast_input(67, 640)
    q, sf = deepep_amd.per_token_cast_to_fp6(x.cuda())
    torch.cuda.synchronize()
    ref = _check_back(q.cpu(), sf.cpu())
    assert _same(ref, fp6_back_ref(*fp6_pair(x)))
    assert bool((ref[0, :32] == 0).all())


def test_fp6_cast_back_strided_rows_column_major_and_typed_scales():
    M, H = 37, 640
    rng = np.random.default_rng(9)
    q = _rows(rng.integers(0, 64, size=(M, H), dtype=np.uint8))
    sf = _bytes(np.asarray(EXPONENTS[1:6], dtype=np.uint8)[rng.integers(0, 5, size=(M, H // 32))])
    wide = torch.zeros((M, 3 * H // 4 + 16), dtype=torch.uint8, device='cuda')
    wide[:, :3 * H // 4] = q.cuda()
    view = wide[:, :3 * H // 4]
    assert view.stride(0) == 3 * H // 4 + 16 and not view.is_contiguous()
    _check_back(q, sf, q_gpu=view)
    # the column-major tensor of use_tma_aligned_col_major_sf (uint8: columns 48 bytes apart): read in place, no copy
    col = torch.empty_strided((M, H // 32), (1, 48), dtype=torch.uint8, device='cuda')
    col.copy_(sf.cuda())
    assert col.stride() == (1, 48)
    _check_back(q, sf, sf_gpu=col)
    _check_back(q, sf, q_gpu=view, sf_gpu=col)
    # contiguous columns in rows further apart than H / 32 bytes: still read as dwords
    rows = torch.zeros((M, H // 32 + 12), dtype=torch.uint8, device='cuda')
    rows[:, :H // 32] = sf.cuda()
    _check_back(q, sf, sf_gpu=rows[:, :H // 32])
    # torch's own dtype
    _check_back(q, sf, sf_gpu=sf.cuda().view(torch.float8_e8m0fnu))
    _check_back(q, sf, q_gpu=view, sf_gpu=col.view(torch.float8_e8m0fnu))


def test_fp6_cast_back_of_no_rows_calls_no_wrapper(monkeypatch):
    import deepep_amd
    from deepep_amd.kernels import Fp6Kernels

    def called(*a, **kw):
        raise AssertionError('M == 0 reached the kernel wrapper')

    monkeypatch.setattr(Fp6Kernels, 'cast_back_fp6', called)
    out = deepep_amd.per_token_cast_back_fp6(torch.empty((0, 96), dtype=torch.uint8, device='cuda'),
                                             torch.empty((0, 4), dtype=torch.uint8, device='cuda'))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 128) and out.is_cuda


def test_fp6_cast_back_wrapper_rejections(kern):
    q = torch.zeros((4, 192), dtype=torch.uint8, device='cuda')
    sf = torch.full((4, 8), 0x7f, dtype=torch.uint8, device='cuda')
    out = torch.full((4, 256), 7.0, dtype=torch.bfloat16, device='cuda')
    odd = torch.zeros((4, 9), dtype=torch.uint8, device='cuda')[:, :8]      # contiguous columns, rows 9 bytes apart
    bad = [dict(sf=sf[:, :2]), dict(sf=sf[:2]), dict(sf=sf.cpu()), dict(sf=sf.to(torch.int8)), dict(sf=odd),
           dict(sf=torch.zeros((4, 2), dtype=torch.uint8, device='cuda')),           # the per-128 shape
           dict(q=q.view(torch.float8_e4m3fn)), dict(q=q[:, :128]), dict(q=q[:, :96]), dict(q=q.cpu()),
           dict(out=out.float()), dict(out=out.t()), dict(out=out[:, :128])]
    for kw in bad:
        args = dict(dict(q=q, sf=sf, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.cast_back_fp6(args['q'], args['sf'], args['out'])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    kern.cast_back_fp6(q, sf, out)
    torch.cuda.synchronize()
    assert _same(out, torch.zeros((4, 256), dtype=torch.bfloat16))


# ----------------------------------------------------------------------------- the pack, kernel level
@pytest.mark.parametrize('peer', [False, True])
@pytest.mark.parametrize('T,H,K', [(33, 256, 4), (3, 7168, 8), (70, 1152, 2)])
def test_pack_cast_fp6_equals_pack_of_the_reference_pair(kern, T, H, K, peer):
    """deepep_dispatch_pack_cast_fp6_mx(x) writes the rows deepep_dispatch_pack writes for fp6_pair(x): codes,
    exponent bytes, top-k indices, weights and source index, for every destination of R = 4; in one local buffer and
    (peer) through per-destination base addresses with system-scope stores.  H = 1152: 36 groups, the last lane pair
    ends the row."""
    from deepep_amd.kernels import RowLayout
    from tests.test_fp8_cast_gpu import _payload, _routes
    R, E = 4, 16
    dev = torch.device('cuda')
    idx, w, dst_slot, send_offsets, rows = _routes(T, K, E, R, seed=T * 31 + H)
    x = _payload(T, H, T + H)
    q, sf = fp6_pair(x)
    layout = RowLayout.make(3 * H // 4, H // 32, K)
    idx, w, dst_slot, send_offsets = idx.to(dev), w.to(dev), dst_slot.to(dev), send_offsets.to(dev)
    ref = torch.zeros((rows + 2, layout.row_bytes), dtype=torch.uint8, device=dev)      # 2 canary rows behind
    got = torch.zeros_like(ref)
    kern.dispatch_pack(q.to(dev), sf.to(dev), idx, w, 1000, dst_slot, send_offsets, ref[:rows], layout)
    x_bytes = x.to(dev).view(torch.uint8).view(T, 2 * H)
    if peer:
        bases = torch.full((R,), got.data_ptr(), dtype=torch.int64, device=dev)
        kern.dispatch_pack_cast_fp6(x_bytes, idx, w, 1000, dst_slot, send_offsets, None, layout, dest_bases=bases,
                                    dest_rows=rows)
    else:
        kern.dispatch_pack_cast_fp6(x_bytes, idx, w, 1000, dst_slot, send_offsets, got[:rows], layout)
    torch.cuda.synchronize()
    assert bool((ref[:rows, :3 * H // 4] != 0).any())                    # the reference rows were written
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} bytes differ, first at row/byte {bad[0].tolist()} ' \
                             f'(sf at {layout.sf_off}, idx at {layout.idx_off})'


# ----------------------------------------------------------------------------- dispatch at EP = 1
T1, K1, E1 = 33, 3, 8


# one dword of exponent bytes; 128 groups: exactly one 3 KiB chunk of codes (4096 columns); 208: a chunk, the first
# half of the next and a part of its second half
@pytest.mark.parametrize('H', [128, 4096, 6656])
def test_keyword_equals_tuple_dispatch_one_rank(H):
    buf = _buffer(_group1(), T1, H, K1)
    fails = fp6_cases(buf, _mx_inputs(H, T1, H, K1, E1), _mx_inputs(H + 1, 0, H, K1, E1), E1)
    torch.cuda.synchronize()
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast_fp6' in names and 'dispatch_pack_cast_fp6' not in names and 'cast_fp6' not in names
    assert 'dispatch_copy_cast' not in names and 'dispatch_copy_cast_fp4' not in names


def test_cached_fp6_dispatch_launches_never_syncs_and_captures_into_a_graph():
    from tests.fp4_ref import FP4
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(7, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    handle = buf.dispatch(x, **base)[3]
    others = [_mx_inputs(70 + i, T1, H, K1, E1)[0] for i in range(2)]
    pairs = [fp6_pair(x)] + [fp6_pair(o) for o in others]
    torch.cuda.synchronize()
    before = len(buf.kernels.calls)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, **FP6)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    launches = [c[0] for c in buf.kernels.calls[before:]]
    before = len(buf.kernels.calls)
    buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, **FP4)
    swap = {'dispatch_copy_cast_fp4': 'dispatch_copy_cast_fp6', 'dispatch_pack_cast_fp4': 'dispatch_pack_cast_fp6'}
    fp4_launches = [c[0] for c in buf.kernels.calls[before:]]
    assert launches == [swap.get(n, n) for n in fp4_launches] and 'dispatch_copy_cast_fp6' in launches
    want = buf.dispatch(pairs[0], handle=handle, topk_weights=w, do_expand=True)
    assert not packed_differences(got, want)
    # one capture of the cached FP6 dispatch, replayed twice with x rewritten in between
    xs = x.clone()

    def call():
        return buf.dispatch(xs, handle=handle, topk_weights=w, do_expand=True, **FP6)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in (1, 2):
        xs.copy_(others[i - 1])
        graph.replay()
        torch.cuda.synchronize()
        want = buf.dispatch(pairs[i], handle=handle, topk_weights=w, do_expand=True)
        assert not packed_differences(out, want), f'replay {i}'
    assert not _same(pairs[1][0], pairs[2][0])                 # the two replays carried different rows
    del graph


def test_fp6_dispatch_under_a_cu_budget():
    H = 128
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(13, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    for mode in (dict(num_sms=32), dict(num_sms=32, async_with_compute_stream=True)):
        fresh = (x * 1) * 1                                    # produced on the compute stream right before the call
        got = buf.dispatch(fresh, **mode, **FP6, **base)
        want = buf.dispatch(fp6_pair(x), **mode, **base)
        if mode.get('async_with_compute_stream'):
            got[4].current_stream_wait()
            want[4].current_stream_wait()
        bad = packed_differences(got, want)
        assert not bad, (mode, bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('col_major', [False, True])
def test_fp6_dispatch_cast_back_combine_round_trip(col_major):
    """dispatch(cast_to_fp6=True) -> per_token_cast_back_fp6 -> combine == the combine of the CPU-cast-back rows of
    the tuple dispatch."""
    import deepep_amd
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(11, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                use_tma_aligned_col_major_sf=col_major)
    (q, sf), _, ex_w, handle, _ = buf.dispatch(x, **FP6, **base)
    (q_t, sf_t), _, _, _, _ = buf.dispatch(fp6_pair(x), **base)
    assert q.dtype == torch.uint8 and q.shape[1] == 3 * H // 4 and sf.dtype == torch.uint8 and sf.shape[1] == H // 32
    assert sf.is_contiguous() != col_major
    y = deepep_amd.per_token_cast_back_fp6(q, sf)
    out, out_w, _ = buf.combine(y, handle, topk_weights=ex_w)
    y_ref = fp6_back_ref(q_t, sf_t).cuda()
    ref, ref_w, _ = buf.combine(y_ref, handle, topk_weights=ex_w)
    torch.cuda.synchronize()
    assert _same(y, y_ref) and _same(out, ref) and _same(out_w, ref_w)
    assert bool((out.float().abs().sum(dim=1)[idx.ge(0).any(dim=1)] > 0).all())      # routed tokens came back


# ----------------------------------------------------------------------------- EP = 4, thread ranks
T4, H4, K4, E4 = 33, 128, 4, 8


def _rank_thread(rank, comm, bypass, leaving, results):
    from tests.sim import FakeGroup
    buf = inputs = empty = None
    try:
        torch.cuda.set_device(0)
        buf = _buffer(FakeGroup(rank, comm.n, comm), T4, H4, K4)
        comm.install(buf, rank)
        buf.local_bypass = bypass
        inputs = _mx_inputs(40 + rank, T4, H4, K4, E4)
        empty = _mx_inputs(50 + rank, 0 if rank == 1 else T4, H4, K4, E4)
        # every mode, the padded exchange of do_cpu_sync=False and a rank without tokens among them
        fails = fp6_cases(buf, inputs, empty, E4)
        torch.cuda.synchronize()
        names = buf.kernels.names()
        if 'dispatch_pack_cast_fp6' not in names or 'dispatch_copy_cast_fp6' in names or 'cast_fp6' in names:
            fails.append(f'EP > 1 casts in the pack only, got {sorted(set(names))}')
        results[rank] = fails
    except Exception:
        results[rank] = [traceback.format_exc()]
        comm.bar.abort()
    finally:
        with leaving:                                          # the ranks leave one at a time, the device idle
            torch.cuda.synchronize()
            buf = inputs = empty = None


@pytest.mark.parametrize('bypass', [True, False])
def test_keyword_equals_tuple_dispatch_four_thread_ranks(bypass):
    from tests.sim import ThreadComm, run_threads
    comm = ThreadComm(4)
    results = run_threads(4, _rank_thread, (comm, bypass, threading.Lock()), timeout=120)
    assert sorted(results) == [0, 1, 2, 3], results
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad


# ----------------------------------------------------------------------------- EP = 2 over xGMI windows
def _xgmi_worker(rank, world, port, queue):
    sys.path.insert(0, ROOT)
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        os.environ['DEEPEP_TRANSPORT'] = 'xgmi'
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        buf = _buffer(dist.group.WORLD, T4, H4, K4, explicitly_destroy=True, num_gpu_timeout_secs=20)
        fails = fp6_cases(buf, _mx_inputs(60 + rank, T4, H4, K4, E4),
                          _mx_inputs(65 + rank, 0 if rank == 1 else T4, H4, K4, E4), E4)
        torch.cuda.synchronize()
        buf._sym.check()
        if 'dispatch_pack_cast_fp6' not in buf.kernels.names():
            fails.append('the casting pack did not run')
        buf.destroy()
        queue.put((rank, fails))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        queue.put((rank, [traceback.format_exc()]))


def test_keyword_equals_tuple_dispatch_over_xgmi_windows():
    world = 2
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_xgmi_worker, args=(r, world, port, queue)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, failures = queue.get(timeout=150)
            results[rank] = failures
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    if len(results) != world or any(results.values()):
        tails = {r: [f[-1500:] for f in fl] for r, fl in results.items()}
        pytest.fail(f'{len(results)}/{world} ranks reported; failures: {tails}', pytrace=False)
