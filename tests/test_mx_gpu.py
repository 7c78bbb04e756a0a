"""MXFP8 (one UE8M0 exponent byte per 32 columns) on the GPU, bitwise: the cast (deepep_cast_fp8_mx) against
tests/mx_ref.mx_pair; the cast back (deepep_cast_back_fp8_mx) against the torch cast back with
float_from_bits(byte << 23); and dispatch(..., cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True,
fp8_group_size=32) against the same build's tuple dispatch of mx_pair(x) -- at EP = 1 (the casting copy), over 4 thread
ranks (the casting pack: local bypass on / off, the padded exchange) and over xGMI windows in two processes.  Thread
ranks and processes are started and time-limited as in tests/test_ue8m0_gpu.py."""
import os
import sys
import threading
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fp8_oracle_kernels import Spy
from tests.mx_ref import MX, mx_back_ref, mx_cases, mx_pair
from tests.test_cast_keyword_gpu import _free_port, _group1, _inputs
from tests.test_fp8_cast_gpu import _same, _u8, cast_ref
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
    """tests/test_ue8m0_gpu._cast_input per 32 columns: in every row, group 0 below the 1e-4 clamp (row 0: all zeros),
    group 1 with amax an exact power of two times 448 (the mantissa-zero branch of the ceil), group 2 with the largest
    finite bf16; the other groups random over +-20 binades."""
    g = torch.Generator().manual_seed(T * 10007 + H)
    x = torch.randn((T, H), generator=g) * torch.exp2(torch.randint(-20, 20, (T, H // 32, 1), generator=g).float()
                                                      ).expand(T, H // 32, 32).reshape(T, H)
    x[:, :32] = torch.randn((T, 32), generator=g) * 1e-6
    x[0, :32] = 0
    x[:, 32:64] = x[:, 32:64].clamp(-1, 1)
    x[:, 32 + 5] = 448.0 * torch.exp2(torch.arange(T).float() % 9 - 4)
    x[:, 64:96] = x[:, 64:96].clamp(-1, 1)
    x[:, 64 + 29] = -BF16_MAX
    return x.to(torch.bfloat16)


def _check_cast(kern, x_cpu: torch.Tensor, x_gpu=None):
    import deepep_amd
    T, H = x_cpu.shape
    x_gpu = x_cpu.cuda() if x_gpu is None else x_gpu
    q_ref, sf_ref = mx_pair(x_cpu)
    q = torch.full((T, H), 1.0, dtype=torch.float32, device='cuda').to(torch.float8_e4m3fn)      # poison: 0x38
    sf = torch.full((T, H // 32), 0xee, dtype=torch.uint8, device='cuda')
    kern.cast_fp8(x_gpu, q, sf, True, mx=True)
    q_pub, sf_pub = deepep_amd.per_token_cast_to_fp8(x_gpu, round_scale=True, use_ue8m0=True, group_size=32)
    torch.cuda.synchronize()
    bad = (sf.cpu() != sf_ref).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} exponent bytes differ, first at {bad[0].tolist()}: ' \
                             f'{sf.cpu()[tuple(bad[0])].item()} != {sf_ref[tuple(bad[0])].item()}'
    bad = (_u8(q) != _u8(q_ref)).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} fp8 codes differ, first at {bad[0].tolist()}: ' \
                             f'{_u8(q)[tuple(bad[0])]:#x} != {_u8(q_ref)[tuple(bad[0])]:#x}'
    assert _same(q_pub, q) and _same(sf_pub, sf) and sf_pub.dtype == torch.uint8 and sf_pub.is_contiguous()
    return q_ref, sf_ref


@pytest.mark.parametrize('T', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 640, 7168])        # a quarter pass; a pass and a quarter; the workload's row
def test_mx_cast(kern, T, H):
    x = _cast_input(T, H)
    q_ref, exp = _check_cast(kern, x)
    assert int(exp[0, 0]) == 105 and int(exp[:, 2].max()) == 247 and int(exp.min()) >= 105
    assert int(exp[0, 1]) == 127 - 4                           # 448 * 2^-4: exactly a power of two, no round up
    # on such input a cast that ignores the group size gives other e4m3fn bytes
    assert not torch.equal(_u8(q_ref), _u8(cast_ref(x, True)[0]))


def test_mx_cast_strided_rows_under_guard_bands_and_wrapper_rejections(kern):
    from tests.guard import Guard
    T, H = 37, 640
    x = _cast_input(T, H)
    wide = torch.zeros((T, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x.cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 64 and not view.is_contiguous()
    _check_cast(kern, x, x_gpu=view)
    guard = Guard(kern)
    _check_cast(guard, x)
    _check_cast(guard, x, x_gpu=view)
    assert guard.verify() >= 2 and guard.guarded_calls == 2
    xg = x.cuda()
    q = torch.zeros((T, H), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    sf = torch.full((T, H // 32), 7, dtype=torch.uint8, device='cuda')
    for what, args, kw in (('without round_scale', (xg, q, sf, False), dict(mx=True)),
                           ('with ue8m0', (xg, q, sf, True), dict(mx=True, ue8m0=True)),
                           ('fp32 scale factors', (xg, q, torch.zeros((T, H // 32), device='cuda'), True), dict(mx=True)),
                           ('the per-128 shape', (xg, q, sf[:, :H // 128].contiguous(), True), dict(mx=True)),
                           ('strided scale factors', (xg, q, torch.zeros((T, H // 16), dtype=torch.uint8,
                                                                         device='cuda')[:, ::2], True), dict(mx=True)),
                           ('uint8 scale factors without mx', (xg, q, sf, True), dict())):
        with pytest.raises(RuntimeError):
            kern.cast_fp8(*args, **kw)
    torch.cuda.synchronize()
    assert bool((sf == 7).all()), 'a rejected call launched'


# ----------------------------------------------------------------------------- the cast back
EXPONENTS = (1, 105, 127, 128, 247, 254, 0)            # byte 0: the factor +0.0f, signed zeros


def _fp8(codes: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)


def _bytes(exp: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(exp, dtype=np.uint8))


def _check_back(q_cpu, sf_cpu, q_gpu=None, sf_gpu=None):
    """per_token_cast_back(q, MX sf) on the GPU == the torch cast back with float_from_bits(byte << 23) on the CPU;
    NaN bytes compared as NaN."""
    import deepep_amd
    q_gpu = q_cpu.cuda() if q_gpu is None else q_gpu
    sf_gpu = sf_cpu.cuda() if sf_gpu is None else sf_gpu
    out = deepep_amd.per_token_cast_back(q_gpu, sf_gpu)
    torch.cuda.synchronize()
    ref = mx_back_ref(q_cpu, sf_cpu)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == ref.shape
    got = out.cpu()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan)
    bad = ((got.view(torch.int16) != ref.view(torch.int16)) & ~nan).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} values differ, first at {bad[0].tolist()}: ' \
                             f'{got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}'
    return ref


def test_mx_cast_back_exhaustive():
    """All 256 bytes in every column position of a group, against each exponent byte: seven blocks of 256 rows; in a
    block a group keeps one exponent while each of its columns runs through all 256 bytes; over the blocks every group
    of the 256 columns (two dwords, all four byte positions) meets every exponent."""
    n, H = len(EXPONENTS), 256
    r, c = np.arange(256 * n).reshape(-1, 1), np.arange(H).reshape(1, H)
    q = _fp8((r + c) % 256)
    exp = np.asarray(EXPONENTS, dtype=np.uint8)[(r // 256 + np.arange(H // 32).reshape(1, -1)) % n]
    ref = _check_back(q, _bytes(exp))
    assert int(ref.isnan().sum()) == n * 2 * H                 # 0x7f and 0xff once per column and block
    zero = ref[6 * 256:7 * 256, :32].view(torch.int16)         # block 6, group 0: exponent byte 0
    finite = ~ref[6 * 256:7 * 256, :32].isnan()
    assert bool(((zero == 0) | (zero == -32768))[finite].all()) and bool((zero == -32768).any())
    assert ref[0x7e - 64, 64].item() == 448.0                  # group 2 of block 0 (exponent 127): byte 0x7e at 2^0


@pytest.mark.parametrize('M', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 640, 7168])        # one dword; the second pass holds 128 columns; the workload's
def test_mx_cast_back_shapes(M, H):
    rng = np.random.default_rng(M * 10007 + H)
    codes = rng.integers(0, 256, size=(M, H), dtype=np.uint8)
    exp = np.asarray(EXPONENTS[:6], dtype=np.uint8)[rng.integers(0, 6, size=(M, H // 32))]
    _check_back(_fp8(codes), _bytes(exp))


def test_mx_cast_back_of_the_mx_cast_equals_the_reference_cast_back():
    import deepep_amd
    x = _cast_input(67, 640)
    q, sf = deepep_amd.per_token_cast_to_fp8(x.cuda(), round_scale=True, use_ue8m0=True, group_size=32)
    q_ref, sf_ref = mx_pair(x)
    torch.cuda.synchronize()
    ref = _check_back(q.cpu(), sf.cpu())
    assert _same(ref, mx_back_ref(q_ref, sf_ref))
    assert bool((ref[0, :32] == 0).all())


def test_mx_cast_back_strided_rows_column_major_and_e8m0_typed_scales():
    M, H = 37, 640
    rng = np.random.default_rng(9)
    q = _fp8(rng.integers(0, 256, size=(M, H), dtype=np.uint8))
    sf = _bytes(np.asarray(EXPONENTS[:6], dtype=np.uint8)[rng.integers(0, 6, size=(M, H // 32))])
    wide = torch.zeros((M, H + 16), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    wide.view(torch.uint8)[:, :H] = q.view(torch.uint8).cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 16 and not view.is_contiguous()
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
    # torch's own MX scale dtype
    _check_back(q, sf, sf_gpu=sf.cuda().view(torch.float8_e8m0fnu))
    _check_back(q, sf, sf_gpu=col.view(torch.float8_e8m0fnu))


def test_mx_cast_back_no_rows_and_wrapper_rejections(kern):
    import deepep_amd
    out = deepep_amd.per_token_cast_back(torch.empty((0, 128), dtype=torch.float8_e4m3fn, device='cuda'),
                                         torch.empty((0, 4), dtype=torch.uint8, device='cuda'))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 128)
    q = torch.zeros((4, 256), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    sf = torch.full((4, 8), 0x7f, dtype=torch.uint8, device='cuda')
    out = torch.full((4, 256), 7.0, dtype=torch.bfloat16, device='cuda')
    odd = torch.zeros((4, 9), dtype=torch.uint8, device='cuda')[:, :8]      # contiguous columns, rows 9 bytes apart
    bad = [dict(sf=sf[:, :2]), dict(sf=sf[:2]), dict(sf=sf.cpu()), dict(sf=sf.to(torch.int8)), dict(sf=odd),
           dict(sf=torch.zeros((4, 2), dtype=torch.uint8, device='cuda')),           # the per-128 shape
           dict(out=out.float()), dict(out=out.t())]
    for kw in bad:
        args = dict(dict(q=q, sf=sf, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.cast_back_fp8(args['q'], args['sf'], args['out'])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    kern.cast_back_fp8(q, sf, out)
    torch.cuda.synchronize()
    assert _same(out, torch.zeros((4, 256), dtype=torch.bfloat16))


# ----------------------------------------------------------------------------- dispatch at EP = 1
T1, K1, E1 = 129, 3, 8                # 129 rows: two 128-row receive blocks


def _buffer(group, T, H, K, kernels=None, **kw):
    """kernels: the provider the spy forwards to (default: HipKernels())."""
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, **kw)
    buf._kernels = Spy(HipKernels() if kernels is None else kernels)
    return buf


def _mx_inputs(seed, tokens, H, K, E):
    """_inputs with rows whose 32-column groups differ by binades (so the per-128 bytes would be other bytes)."""
    x, idx, w = _inputs(seed, tokens, H, K, E)
    g = torch.Generator().manual_seed(seed + 1000)
    scale = torch.exp2(torch.randint(-6, 6, (tokens, H // 32, 1), generator=g).float()).expand(tokens, H // 32, 32)
    return (x.float().cpu() * scale.reshape(tokens, H)).to(torch.bfloat16).cuda(), idx, w


@pytest.mark.parametrize('H', [128, 2560])             # one dword; one 2 KiB output chunk + a quarter
def test_keyword_equals_tuple_dispatch_one_rank(H):
    buf = _buffer(_group1(), T1, H, K1)
    fails = mx_cases(buf, _mx_inputs(H, T1, H, K1, E1), _mx_inputs(H + 1, 0, H, K1, E1), E1)
    torch.cuda.synchronize()
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names


def test_one_rank_dispatch_stores_inside_its_outputs():
    """The reduced and the expanded casting copy under guard bands."""
    from deepep_amd.kernels import HipKernels
    from tests.guard import Guard
    H = 2560
    guard = Guard(HipKernels())
    buf = _buffer(_group1(), T1, H, K1, kernels=guard)
    x, idx, w = _mx_inputs(5, T1, H, K1, E1)
    for more in (dict(), dict(do_expand=True, expert_alignment=16, do_zero_padding=True)):
        got = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, **more, **MX)
        want = buf.dispatch(mx_pair(x), topk_idx=idx, topk_weights=w, num_experts=E1, **more)
        assert not packed_differences(got, want), more
    assert guard.verify() > 0
    assert 'dispatch_copy_cast' in buf.kernels.names()


def test_cached_mx_dispatch_never_syncs_and_captures_into_a_graph():
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(7, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    handle = buf.dispatch(x, **base)[3]
    others = [_mx_inputs(70 + i, T1, H, K1, E1)[0] for i in range(2)]
    pairs = [mx_pair(x)] + [mx_pair(o) for o in others]
    torch.cuda.synchronize()
    before = len(buf.kernels.calls)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, **MX)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    launches = [c[0] for c in buf.kernels.calls[before:]]
    before = len(buf.kernels.calls)
    buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, cast_to_fp8=True, fp8_round_scale=True,
                 fp8_use_ue8m0=True)
    assert launches == [c[0] for c in buf.kernels.calls[before:]]              # the per-128 call's launches
    want = buf.dispatch(pairs[0], handle=handle, topk_weights=w, do_expand=True)
    assert not packed_differences(got, want)
    # one capture of the cached MX dispatch, replayed twice with x rewritten in between
    xs = x.clone()

    def call():
        return buf.dispatch(xs, handle=handle, topk_weights=w, do_expand=True, **MX)

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


def test_mx_dispatch_under_a_cu_budget():
    H = 128
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(13, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    for mode in (dict(num_sms=16), dict(num_sms=16, async_with_compute_stream=True)):
        fresh = (x * 1) * 1                                    # produced on the compute stream right before the call
        got = buf.dispatch(fresh, **mode, **MX, **base)
        want = buf.dispatch(mx_pair(x), **mode, **base)
        if mode.get('async_with_compute_stream'):
            got[4].current_stream_wait()
            want[4].current_stream_wait()
        bad = packed_differences(got, want)
        assert not bad, (mode, bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('col_major', [False, True])
def test_mx_dispatch_cast_back_combine_round_trip(col_major):
    """dispatch(the MX flags) -> per_token_cast_back -> combine == the combine of the CPU-cast-back rows; the pair
    itself is no combine input."""
    import deepep_amd
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _mx_inputs(11, T1, H, K1, E1)
    (q, sf), _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                                               use_tma_aligned_col_major_sf=col_major, **MX)
    assert sf.dtype == torch.uint8 and sf.shape[1] == H // 32 and sf.is_contiguous() != col_major
    with pytest.raises(RuntimeError, match='per_token_cast_back'):
        buf.combine((q, sf), handle, topk_weights=ex_w)
    y = deepep_amd.per_token_cast_back(q, sf)
    out, out_w, _ = buf.combine(y, handle, topk_weights=ex_w)
    y_ref = mx_back_ref(q, sf).cuda()
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
        fails = mx_cases(buf, inputs, empty, E4)
        torch.cuda.synchronize()
        names = buf.kernels.names()
        if 'dispatch_pack_cast' not in names or 'dispatch_copy_cast' in names or 'cast_fp8' in names:
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
        fails = mx_cases(buf, _mx_inputs(60 + rank, T4, H4, K4, E4),
                         _mx_inputs(65 + rank, 0 if rank == 1 else T4, H4, K4, E4), E4)
        torch.cuda.synchronize()
        buf._sym.check()
        if 'dispatch_pack_cast' not in buf.kernels.names():
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
