"""ElasticBuffer.dispatch(..., cast_to_fp8=True) on the GPU: the keyword dispatch of a bf16 x returns, bit for
bit, what the same build's tuple dispatch of the CPU-cast pair (tests/test_fp8_cast_gpu.cast_ref) returns -- rows,
scale factors, routing, weights and every handle field -- at EP = 1 (the casting copy), over 4 thread ranks
(the casting pack: local bypass on / off, the padded exchange) and over xGMI windows in two processes.  It adds
no host synchronisation and captures into a HIP graph where the plain dispatch does; with
deepep_amd.per_token_cast_back the round trip dispatch -> cast back -> combine needs no torch chain."""
import os
import socket
import sys
import threading
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from tests.fp8_oracle_kernels import Spy, cast_pair, dispatch_differences, keyword_cases
from tests.test_cast_back_gpu import back_ref
from tests.test_fp8_cast_gpu import _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _group1():
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29574')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(seed: int, tokens: int, H: int, K: int, E: int):
    """bf16 rows, masked routing with one token routed nowhere, weights -- on the GPU."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((tokens, H), generator=g) * 3).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x.cuda(), idx.to(topk_idx_t).cuda(), w.cuda()


def _buffer(group, T, H, K, kernels=None, **kw):
    """kernels: the provider the spy forwards to (default: HipKernels())."""
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, **kw)
    buf._kernels = Spy(HipKernels() if kernels is None else kernels)
    return buf


# ----------------------------------------------------------------------------- EP = 1
T1, K1, E1 = 129, 3, 8                # 129 rows: two 128-row receive blocks


@pytest.mark.parametrize('H', [384, 2176])      # three groups (under one 2 KiB output chunk); one chunk + one group
def test_keyword_equals_tuple_dispatch_one_rank(H):
    buf = _buffer(_group1(), T1, H, K1)
    fails = keyword_cases(buf, _inputs(H, T1, H, K1, E1), _inputs(H + 1, 0, H, K1, E1), E1)
    torch.cuda.synchronize()
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names


def test_cached_casting_dispatch_never_syncs_and_captures_into_a_graph():
    H = 384
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(7, T1, H, K1, E1)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    handle = buf.dispatch(x, **base)[3]
    pairs = [cast_pair(x)] + [cast_pair(_inputs(70 + i, T1, H, K1, E1)[0]) for i in range(2)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = buf.dispatch(x, handle=handle, topk_weights=w, do_expand=True, cast_to_fp8=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = buf.dispatch(pairs[0], handle=handle, topk_weights=w, do_expand=True)
    assert not dispatch_differences(got, want)
    # one capture of the cached casting dispatch, replayed twice with x rewritten in between
    xs = x.clone()

    def call():
        return buf.dispatch(xs, handle=handle, topk_weights=w, do_expand=True, cast_to_fp8=True)

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
        assert not dispatch_differences(out, want), f'replay {i}'
    assert not _same(pairs[1][0], pairs[2][0])                 # the two replays carried different rows
    del graph


def test_keyword_composes_with_stream_modes_and_a_cu_budget():
    """The stream / event modes of the reference test (tests/elastic/test_ep.py:34-41) and an explicit num_sms: x is
    produced on the compute stream right before the call, so a comm-stream kernel that did not wait would read
    unfinished rows."""
    H = 384
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(13, T1, H, K1, E1)
    pair = cast_pair(x)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    modes = [dict(async_with_compute_stream=True), dict(allocate_on_comm_stream=True),
             dict(async_with_compute_stream=True, allocate_on_comm_stream=True),
             dict(previous_event=True, allocate_on_comm_stream=True),
             dict(previous_event=True, async_with_compute_stream=True, allocate_on_comm_stream=True),
             dict(num_sms=16), dict(num_sms=16, async_with_compute_stream=True)]

    def launch(xin, mode, **kw):
        mode = dict(mode)
        if mode.pop('previous_event', False):
            mode['previous_event'] = buf.capture()
        out = buf.dispatch(xin, **mode, **kw, **base)
        if mode.get('async_with_compute_stream'):
            out[4].current_stream_wait()
        return out

    for mode in modes:
        fresh = (x * 1) * 1
        got = launch(fresh, mode, cast_to_fp8=True)
        want = launch(pair, mode)
        bad = dispatch_differences(got, want)
        assert not bad, (mode, bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize('col_major', [False, True])
def test_dispatch_cast_back_combine_round_trip(col_major):
    """dispatch(cast_to_fp8) -> per_token_cast_back -> combine == the combine of the CPU-cast-back rows."""
    import deepep_amd
    H = 2176
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = _inputs(11, T1, H, K1, E1)
    (q, sf), _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                                               cast_to_fp8=True, use_tma_aligned_col_major_sf=col_major)
    assert sf.is_contiguous() != col_major
    y = deepep_amd.per_token_cast_back(q, sf)
    out, out_w, _ = buf.combine(y, handle, topk_weights=ex_w)
    y_ref = back_ref(q, sf).cuda()
    ref, ref_w, _ = buf.combine(y_ref, handle, topk_weights=ex_w)
    torch.cuda.synchronize()
    assert _same(y, y_ref) and _same(out, ref) and _same(out_w, ref_w)
    assert bool((out.float().abs().sum(dim=1)[idx.ge(0).any(dim=1)] > 0).all())      # routed tokens came back


# ----------------------------------------------------------------------------- EP = 4, thread ranks
T4, H4, K4, E4 = 33, 256, 4, 8


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
        fails = keyword_cases(buf, inputs, empty, E4)
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
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


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
        fails = keyword_cases(buf, _inputs(60 + rank, T4, H4, K4, E4), _inputs(65 + rank, 0 if rank == 1 else T4,
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
