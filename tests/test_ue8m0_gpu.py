"""Packed UE8M0 scale factors on the GPU, bitwise: the packed cast (deepep_cast_fp8_ue8m0) against
(cast_ref q, pack_ref sf); the packed cast back (deepep_cast_back_fp8_ue8m0) against the torch cast back of the
unpacked factors and against the fp32 kernel; and dispatch(..., cast_to_fp8=True, fp8_round_scale=True,
fp8_use_ue8m0=True) against the same build's tuple dispatch of (cast_ref q, pack_ref sf) -- at EP = 1 (the casting
copy), over 4 thread ranks (the casting pack: local bypass on / off, the padded exchange) and over xGMI windows in two
processes.  Thread ranks and processes are started and time-limited as in tests/test_cast_keyword_gpu.py."""
import os
import sys
import threading
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fp8_oracle_kernels import Spy
from tests.test_cast_back_gpu import back_ref
from tests.test_cast_keyword_gpu import _free_port, _group1, _inputs
from tests.test_fp8_cast_gpu import _same, _u8, cast_ref
from tests.ue8m0_ref import UE8M0, pack_ref, packed_differences, ue8m0_cases, ue8m0_pair, unpack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BF16_MAX = torch.finfo(torch.bfloat16).max


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


# ----------------------------------------------------------------------------- the packed cast
def _cast_input(T: int, H: int) -> torch.Tensor:
    """Random rows whose groups span the exponent range: in every row, group 0 below the 1e-4 clamp (row 0: all
    zeros), group 1 with amax an exact power of two times 448 (the mantissa-zero branch of the ceil), group 2 with
    the largest finite bf16; the other groups random over many binades."""
    g = torch.Generator().manual_seed(T * 10007 + H)
    x = torch.randn((T, H), generator=g) * torch.exp2(torch.randint(-20, 20, (T, H // 128, 1), generator=g).float()
                                                      ).expand(T, H // 128, 128).reshape(T, H)
    x[:, :128] = torch.randn((T, 128), generator=g) * 1e-6
    x[0, :128] = 0
    x[:, 128:256] = x[:, 128:256].clamp(-1, 1)
    x[:, 128 + 5] = 448.0 * torch.exp2(torch.arange(T).float() % 9 - 4)
    x[:, 256:384] = x[:, 256:384].clamp(-1, 1)
    x[:, 256 + 77] = -BF16_MAX
    return x.to(torch.bfloat16)


def _check_packed_cast(kern, x_cpu: torch.Tensor, x_gpu=None):
    import deepep_amd
    T, H = x_cpu.shape
    x_gpu = x_cpu.cuda() if x_gpu is None else x_gpu
    q_ref, sf_ref = cast_ref(x_cpu, True)
    packed_ref = pack_ref(sf_ref)
    q = torch.full((T, H), 1.0, dtype=torch.float32, device='cuda').to(torch.float8_e4m3fn)      # poison: 0x38
    sf = torch.full((T, H // 512), -7, dtype=torch.int32, device='cuda')
    kern.cast_fp8(x_gpu, q, sf, True, ue8m0=True)
    q_pub, sf_pub = deepep_amd.per_token_cast_to_fp8(x_gpu, round_scale=True, use_ue8m0=True)
    q_rs, _ = deepep_amd.per_token_cast_to_fp8(x_gpu, round_scale=True)
    torch.cuda.synchronize()
    bad = (sf.cpu() != packed_ref).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} packed scale factors differ, first at {bad[0].tolist()}: ' \
                             f'{sf.cpu()[tuple(bad[0])].item():#x} != {packed_ref[tuple(bad[0])].item():#x}'
    assert torch.equal(_u8(q), _u8(q_ref)) and _same(q, q_rs)          # the round_scale bytes, unchanged
    assert _same(q_pub, q) and _same(sf_pub, sf) and sf_pub.dtype == torch.int32 and sf_pub.is_contiguous()
    return packed_ref


@pytest.mark.parametrize('T', [1, 5, 129])
@pytest.mark.parametrize('H', [512, 1536, 7168])       # one dword and one pass; an odd number of packs; the workload's
def test_packed_cast(kern, T, H):
    x = _cast_input(T, H)
    packed = _check_packed_cast(kern, x)
    exp = packed.view(torch.uint8).view(T, H // 128)
    assert int(exp[0, 0]) == 105 and int(exp[:, 2].max()) == 247 and int(exp.min()) >= 105
    assert int(exp[0, 1]) == 127 - 4                           # 448 * 2^-4: exactly a power of two, no round up


def test_packed_cast_strided_rows_and_wrapper_rejections(kern):
    T, H = 37, 1536
    x = _cast_input(T, H)
    wide = torch.zeros((T, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x.cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 64 and not view.is_contiguous()
    _check_packed_cast(kern, x, x_gpu=view)
    xg = x.cuda()
    q = torch.zeros((T, H), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    sf = torch.full((T, H // 512), 7, dtype=torch.int32, device='cuda')
    for what, args, kw in (('without round_scale', (xg, q, sf, False), dict(ue8m0=True)),
                           ('fp32 scale factors', (xg, q, torch.zeros((T, H // 128), device='cuda'), True),
                            dict(ue8m0=True)),
                           ('the fp32 shape', (xg, q, torch.zeros((T, H // 128), dtype=torch.int32, device='cuda'),
                                               True), dict(ue8m0=True)),
                           ('H % 512 != 0', (xg[:, :1280].contiguous(), q[:, :1280].contiguous(),
                                             sf[:, :2].contiguous(), True), dict(ue8m0=True)),
                           ('int32 scale factors without ue8m0', (xg, q, sf, True), dict())):
        with pytest.raises(RuntimeError):
            kern.cast_fp8(*args, **kw)
    torch.cuda.synchronize()
    assert bool((sf == 7).all()), 'a rejected call launched'


# ----------------------------------------------------------------------------- the packed cast back
EXPONENTS = (1, 105, 127, 128, 247, 254, 0)            # byte 0: the factor +0.0f, signed zeros


def _fp8(codes: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)


def _pack_bytes(exp: np.ndarray) -> torch.Tensor:
    """uint8 [M, G] exponent bytes -> int32 [M, G / 4]."""
    return torch.from_numpy(np.ascontiguousarray(exp, dtype=np.uint8)).view(torch.int32)


def _check_back(q_cpu, sf_cpu, q_gpu=None, sf_gpu=None):
    """per_token_cast_back(q, packed sf) on the GPU == the torch cast back of (q, unpack_ref(sf)) on the CPU, and ==
    the fp32 kernel on the unpacked factors; NaN bytes compared as NaN."""
    import deepep_amd
    q_gpu = q_cpu.cuda() if q_gpu is None else q_gpu
    sf_gpu = sf_cpu.cuda() if sf_gpu is None else sf_gpu
    out = deepep_amd.per_token_cast_back(q_gpu, sf_gpu)
    out_fp32 = deepep_amd.per_token_cast_back(q_gpu, unpack_ref(sf_cpu).cuda())
    torch.cuda.synchronize()
    ref = back_ref(q_cpu, unpack_ref(sf_cpu))
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == ref.shape
    got = out.cpu()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan) and torch.equal(out_fp32.cpu().isnan(), nan)
    bad = ((got.view(torch.int16) != ref.view(torch.int16)) & ~nan).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} values differ, first at {bad[0].tolist()}: ' \
                             f'{got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}'
    assert bool(((got.view(torch.int16) == out_fp32.cpu().view(torch.int16)) | nan).all())
    return ref


def test_packed_cast_back_exhaustive():
    """All 256 bytes in every column position of a group, against each exponent byte: seven blocks of 256 rows; in a
    block a group keeps one exponent while each of its columns runs through all 256 bytes; over the blocks every
    group of the 1024 columns (two dwords, all four byte positions) meets every exponent."""
    n, H = len(EXPONENTS), 1024
    r, c = np.arange(256 * n).reshape(-1, 1), np.arange(H).reshape(1, H)
    q = _fp8((r + c) % 256)
    exp = np.asarray(EXPONENTS, dtype=np.uint8)[(r // 256 + np.arange(H // 128).reshape(1, -1)) % n]
    ref = _check_back(q, _pack_bytes(exp))
    assert int(ref.isnan().sum()) == n * 2 * H                 # 0x7f and 0xff once per column and block
    zero = ref[6 * 256:7 * 256, :128].view(torch.int16)        # block 6, group 0: exponent byte 0
    finite = ~ref[6 * 256:7 * 256, :128].isnan()
    assert bool(((zero == 0) | (zero == -32768))[finite].all()) and bool((zero == -32768).any())
    assert ref[0x7e, 256].item() == 448.0                      # row 0x7e, group 2 (exponent 127): byte 0x7e at 2^0


@pytest.mark.parametrize('M', [1, 5, 129])
@pytest.mark.parametrize('H', [512, 1536, 7168])       # 1536: the second pass holds 512 columns, half a pass
def test_packed_cast_back_shapes(M, H):
    rng = np.random.default_rng(M * 10007 + H)
    codes = rng.integers(0, 256, size=(M, H), dtype=np.uint8)
    exp = np.asarray(EXPONENTS[:6], dtype=np.uint8)[rng.integers(0, 6, size=(M, H // 128))]
    _check_back(_fp8(codes), _pack_bytes(exp))


def test_packed_cast_back_of_the_packed_cast_equals_the_fp32_cast_back():
    import deepep_amd
    x = _cast_input(67, 1536)
    q, sf = deepep_amd.per_token_cast_to_fp8(x.cuda(), round_scale=True, use_ue8m0=True)
    q_ref, sf_ref = cast_ref(x, True)
    torch.cuda.synchronize()
    ref = _check_back(q.cpu(), sf.cpu())
    assert _same(ref, back_ref(q_ref, sf_ref))
    assert bool((ref[0, :128] == 0).all())


def test_packed_cast_back_strided_rows_and_column_major_scales():
    M, H = 37, 1536
    rng = np.random.default_rng(9)
    q = _fp8(rng.integers(0, 256, size=(M, H), dtype=np.uint8))
    sf = _pack_bytes(np.asarray(EXPONENTS[:6], dtype=np.uint8)[rng.integers(0, 6, size=(M, H // 128))])
    wide = torch.zeros((M, H + 16), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    wide.view(torch.uint8)[:, :H] = q.view(torch.uint8).cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 16 and not view.is_contiguous()
    _check_back(q, sf, q_gpu=view)
    # the column-major packed tensor of use_tma_aligned_col_major_sf: read in place, no copy
    col = torch.empty_strided((M, H // 512), (1, 40), dtype=torch.int32, device='cuda')
    col.copy_(sf.cuda())
    assert col.stride() == (1, 40)
    _check_back(q, sf, sf_gpu=col)
    _check_back(q, sf, q_gpu=view, sf_gpu=col)


def test_packed_cast_back_no_rows_and_wrapper_rejections(kern):
    import deepep_amd
    out = deepep_amd.per_token_cast_back(torch.empty((0, 512), dtype=torch.float8_e4m3fn, device='cuda'),
                                         torch.empty((0, 1), dtype=torch.int32, device='cuda'))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 512)
    q = torch.zeros((4, 1024), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    sf = torch.full((4, 2), 0x7f7f7f7f, dtype=torch.int32, device='cuda')
    out = torch.full((4, 1024), 7.0, dtype=torch.bfloat16, device='cuda')
    bad = [dict(sf=sf[:, :1]), dict(sf=sf[:2]), dict(sf=sf.cpu()), dict(sf=sf.to(torch.int64)),
           dict(sf=torch.zeros((4, 8), dtype=torch.int32, device='cuda')),
           dict(q=q[:, :256].contiguous(), out=out[:, :256].contiguous()),          # H = 256 with int32 [4, 2]
           dict(q=q[:, :640].contiguous(), sf=sf[:, :1], out=out[:, :640].contiguous()),
           dict(out=out.float()), dict(out=out.t())]
    for kw in bad:
        args = dict(dict(q=q, sf=sf, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.cast_back_fp8(args['q'], args['sf'], args['out'])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    kern.cast_back_fp8(q, sf, out)
    torch.cuda.synchronize()
    assert _same(out, torch.zeros((4, 1024), dtype=torch.bfloat16))


# ----------------------------------------------------------------------------- dispatch at EP = 1
T1, K1, E1 = 129, 3, 8                # 129 rows: two 128-row receive blocks


def _buffer(group, T, H, K, kernels=None, **kw):
    """kernels: the provider the spy forwards to (default: HipKernels())."""
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, **kw)
    buf._kernels = Spy(HipKernels() if kernels is None else kernels)
    return buf


@pytest.mark.parametrize('H', [512, 2560])             # one dword; one 2 KiB output chunk + a quarter (five dwords)
def test_keyword_equals_tuple_dispatch_one_rank(H):
    buf = _buffer(_group1(), T1, H, K1)
    fails = ue8m0_cases(buf, _inputs(H, T1, H, K1, E1), _inputs(H + 1, 0, H, K1, E1), E1)
    torch.cuda.synchronize()
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names


def test_cached_packed_dispatch_never_syncs_and_captures_into_a_graph():
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(7, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    handle = buf.dispatch(x, **base)[3]
    pairs = [ue8m0_pair(x)] + [ue8m0_pair(_inputs(70 + i, T1, H, K1, E1)[0]) for i in range(2)]
    torch.cuda.synchronize()
    before = len(buf.kernels.calls)
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, **UE8M0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    launches = [c[0] for c in buf.kernels.calls[before:]]
    before = len(buf.kernels.calls)
    buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, cast_to_fp8=True, fp8_round_scale=True)
    assert launches == [c[0] for c in buf.kernels.calls[before:]]              # no launch added
    want = buf.dispatch(pairs[0], handle=handle, topk_weights=w, do_expand=True)
    assert not packed_differences(got, want)
    # one capture of the cached packed dispatch, replayed twice with x rewritten in between
    xs = x.clone()

    def call():
        return buf.dispatch(xs, handle=handle, topk_weights=w, do_expand=True, **UE8M0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in (1, 2):
        xs.copy_(_inputs(70 + i - 1, T1, H, K1, E1)[0])
        graph.replay()
        torch.cuda.synchronize()
        want = buf.dispatch(pairs[i], handle=handle, topk_weights=w, do_expand=True)
        assert not packed_differences(out, want), f'replay {i}'
    assert not _same(pairs[1][0], pairs[2][0])                 # the two replays carried different rows
    del graph


def test_packed_dispatch_under_a_cu_budget():
    H = 512
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(13, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    for mode in (dict(num_sms=16), dict(num_sms=16, async_with_compute_stream=True)):
        fresh = (x * 1) * 1                                    # produced on the compute stream right before the call
        got = buf.dispatch(fresh, **mode, **UE8M0, **base)
        want = buf.dispatch(ue8m0_pair(x), **mode, **base)
        if mode.get('async_with_compute_stream'):
            got[4].current_stream_wait()
            want[4].current_stream_wait()
        bad = packed_differences(got, want)
        assert not bad, (mode, bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('col_major', [False, True])
def test_packed_dispatch_cast_back_combine_round_trip(col_major):
    """dispatch(all three flags) -> per_token_cast_back -> combine == the combine of the CPU-cast-back rows."""
    import deepep_amd
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(11, T1, H, K1, E1)
    (q, sf), _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                                               use_tma_aligned_col_major_sf=col_major, **UE8M0)
    assert sf.dtype == torch.int32 and sf.shape[1] == H // 512 and sf.is_contiguous() != col_major
    y = deepep_amd.per_token_cast_back(q, sf)
    out, out_w, _ = buf.combine(y, handle, topk_weights=ex_w)
    y_ref = back_ref(q, unpack_ref(sf.cpu())).cuda()
    ref, ref_w, _ = buf.combine(y_ref, handle, topk_weights=ex_w)
    torch.cuda.synchronize()
    assert _same(y, y_ref) and _same(out, ref) and _same(out_w, ref_w)
    assert bool((out.float().abs().sum(dim=1)[idx.ge(0).any(dim=1)] > 0).all())      # routed tokens came back


# ----------------------------------------------------------------------------- EP = 4, thread ranks
T4, H4, K4, E4 = 33, 512, 4, 8


def _rank_thread(rank, comm, bypass, leaving, results):
    from tests.sim import FakeGroup
    buf = inputs = empty = None
    try:
        torch.cuda.set_device(0)
        buf = _buffer(FakeGroup(rank, comm.n, comm), T4, H4, K4)
        comm.install(buf, rank)
        buf.local_bypass = bypass
        inputs = _inputs(40 + rank, T4, H4, K4, E4)
        empty = _inputs(50 + rank, 0 if rank == 1 else T4, H4, K4, E4)
        # every mode, the padded exchange of do_cpu_sync=False and a rank without tokens among them
        fails = ue8m0_cases(buf, inputs, empty, E4)
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
        fails = ue8m0_cases(buf, _inputs(60 + rank, T4, H4, K4, E4), _inputs(65 + rank, 0 if rank == 1 else T4,
                                                                             H4, K4, E4), E4)
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
