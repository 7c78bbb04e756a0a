"""EP_NUM_TOPK_IDX_BITS=32 (deep_ep.topk_idx_t = int32) on the CPU: gloo ranks plus the oracle stand-in.

The variable is read when deepep_amd is imported, so every 32-bit run is a fresh process: the spawned
gloo workers of tests/test_buffer_cpu.py (they inherit the environment set here before the spawn and
report the topk_idx_t they saw) or tests/idx_bits_child.py.  The bodies are the 64-bit suite's own
(`_worker`, `dispatch_mode_checks`): the routing is cast to deep_ep.topk_idx_t where it is built, the
results stay bitwise against the golden fixtures, and recv_topk_idx must come back in that dtype.

The stand-in (tests/oracle_kernels.py) asserts what the HIP wrappers require of the routing --
contiguous int64 -- so a host path that hands the caller's int32 tensor to a kernel wrapper fails here,
at build_local_plan (EP = 1, non-expanded combine) or plan_source (EP > 1 combine), without a GPU.
"""
import pytest
import torch
import torch.multiprocessing as mp

from tests.idx_bits_child import run_child
from tests.test_buffer_cpu import _free_port, _modes_worker, _worker


def _spawn32(monkeypatch, target, world, args_of):
    """Run target(rank, world, port, *args_of(queue)) on `world` spawned processes that see
    EP_NUM_TOPK_IDX_BITS=32 before they import deepep_amd; returns {rank: (failures, topk_idx_t)}."""
    monkeypatch.setenv('EP_NUM_TOPK_IDX_BITS', '32')
    for var in ('HIP_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'):
        monkeypatch.setenv(var, '-1')         # CPU ranks: they open no GPU where one is present
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args_of(queue))) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, failures, dtype = queue.get(timeout=240)
            results[rank] = (failures, dtype)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return results


def _check(results, world):
    assert len(results) == world, results
    bad = {r: f for r, (f, _) in results.items() if f}
    assert not bad, bad
    # a run in which the variable did not take effect must not pass
    assert {d for _, d in results.values()} == {'torch.int32'}, results


@pytest.mark.parametrize('fixture,world', [
    ('f1_ep1_t128_h1024_k2.npz', 1),
    ('f4_ep4_t96_h256_k2.npz', 4),          # R > K: the top-k layout
    ('f2_ep8_t64_h256_k8.npz', 8),          # R <= K: the rank layout
])
def test_golden_fixtures_with_int32_routing(fixture, world, monkeypatch):
    """Dispatch in both layouts, then combine with bias 0/1/2, multiple and single reduction, plain and
    gating-weighted, bitwise against the fixtures -- with int32 routing."""
    _check(_spawn32(monkeypatch, _worker, world, lambda q: (fixture, q, None, True)), world)


@pytest.mark.parametrize('world,alignment,do_cpu_sync,do_handle_copy', [(1, 8, False, True), (4, 4, True, False)])
def test_dispatch_modes_with_int32_routing(world, alignment, do_cpu_sync, do_handle_copy, monkeypatch):
    """tests/helpers.py::dispatch_mode_checks (cached, cached expanded, handle copy / alias, counters, and
    without a CPU sync the worst-case shapes and the combines over such a handle) with int32 routing."""
    _check(_spawn32(monkeypatch, _modes_worker, world,
                    lambda q: (alignment, do_cpu_sync, do_handle_copy, q, 0, True)), world)


def test_ep1_case_with_int32_routing():
    """The GPU suite's EP = 1 case (tests/idx_bits_child.py::case_ep1) through the stand-in: the host path
    of every dispatch / combine flavour it drives hands the kernels int64 routing."""
    report = run_child('ep1', device='cpu')
    assert report['topk_idx_t'] == 'torch.int32' and report['device'] == 'cpu', report
    assert report['failures'] == [] and list(report['seconds']) == ['ep1'], report


def test_routing_of_the_other_width_is_rejected():
    """int64 routing with EP_NUM_TOPK_IDX_BITS=32 (a child) and int32 routing by default (here) both
    fail the dispatch's deep_ep.topk_idx_t assertion."""
    report = run_child('reject', device='cpu')
    assert report['topk_idx_t'] == 'torch.int32', report
    assert report['failures'] == [] and list(report['seconds']) == ['reject'], report
    buf, x, idx, _ = _default_mode_buffer()
    with pytest.raises(RuntimeError, match='deep_ep.topk_idx_t'):
        buf.dispatch(x, topk_idx=idx.to(torch.int32), num_experts=8)


def _default_mode_buffer():
    """A one-rank CPU buffer on the stand-in, in this process: the default (64-bit) mode."""
    import deepep_amd
    from tests.oracle_kernels import OracleKernels
    from tests.sim import FakeGroup, ThreadComm
    assert deepep_amd.topk_idx_t == torch.int64, 'this test needs the default EP_NUM_TOPK_IDX_BITS'
    T, H, K, E = 33, 64, 3, 8
    buf = deepep_amd.ElasticBuffer(FakeGroup(0, 1, ThreadComm(1)), num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = OracleKernels()
    buf.use_cuda, buf.device = False, torch.device('cpu')      # CPU tensors: no streams, where a GPU is present too
    g = torch.Generator().manual_seed(2)
    w, idx = torch.topk(torch.rand((T, E), generator=g), K, dim=-1, sorted=False)
    idx[torch.rand(idx.shape, generator=g) < 0.3] = -1
    x = torch.randn((T, H), generator=g).to(torch.bfloat16)
    return buf, x, idx, w.masked_fill(idx < 0, 0)


class _Spy:
    """Forwards to a kernel provider and records the topk_idx every routing-reading wrapper was given."""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        pos = {'build_local_plan': 7, 'plan_source': 0, 'dispatch_notify': 0, 'dispatch_pack': 2}   # of topk_idx
        if name not in pos:
            return fn

        def wrapped(*args, **kw):
            self.seen.append((name, kw['topk_idx'] if 'topk_idx' in kw else args[pos[name]]))
            return fn(*args, **kw)
        return wrapped


@pytest.mark.parametrize('do_handle_copy', [True, False])
def test_default_mode_routing_is_the_handle_tensor(do_handle_copy):
    """With int64 routing nothing is converted or copied for the kernels: the handle's int64 routing IS
    handle.topk_idx (which aliases the caller's tensor with do_handle_copy=False), and that very tensor is
    what the combine plan and a cached dispatch hand to the kernel wrappers."""
    buf, x, idx, w = _default_mode_buffer()
    recv_x, recv_idx, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=8,
                                                       do_handle_copy=do_handle_copy)
    assert handle.topk_idx.dtype == torch.int64 and recv_idx.dtype == torch.int64
    assert handle.routing_idx64() is handle.topk_idx
    assert handle.routing_idx64().data_ptr() == handle.topk_idx.data_ptr()
    assert (handle.topk_idx.data_ptr() == idx.data_ptr()) == (not do_handle_copy)
    assert torch.equal(handle.topk_idx, idx)
    spy = buf._kernels = _Spy(buf._kernels)
    out, out_w, _ = buf.combine(torch.randn(recv_x.shape).to(torch.bfloat16), handle, topk_weights=recv_w)
    buf.dispatch(x, handle=handle)
    assert [n for n, _ in spy.seen] == ['build_local_plan', 'dispatch_pack'], spy.seen
    assert all(t is handle.topk_idx for _, t in spy.seen), spy.seen
    assert torch.equal(out_w, w)


def test_hand_built_handle_converts_its_routing_once():
    """A handle this build's dispatch did not create (int32 routing, no stored int64 form) converts on
    the first use and keeps the result; cache=False (a HIP graph capture) keeps nothing."""
    from deepep_amd.handle import EPHandle
    idx = torch.tensor([[0, -1, 3], [2, 1, -1]], dtype=torch.int32)
    none = torch.empty((0,), dtype=torch.int32)
    handle = EPHandle(False, 4, 1, 2, 4, idx, 2, 2, [], none, none, none, none, none, None, None)
    a = handle.routing_idx64(cache=False)
    assert a.dtype == torch.int64 and a.is_contiguous() and torch.equal(a, idx.to(torch.int64))
    assert handle._idx64 is None and handle.topk_idx is idx
    b = handle.routing_idx64()
    assert b is not a and handle.routing_idx64() is b and handle.routing_idx64(cache=False) is b
    strided = torch.arange(12, dtype=torch.int64).view(2, 6)[:, ::2]
    handle = EPHandle(False, 4, 1, 2, 4, strided, 2, 2, [], none, none, none, none, none, None, None)
    c = handle.routing_idx64()
    assert c.is_contiguous() and torch.equal(c, strided) and c is not strided
