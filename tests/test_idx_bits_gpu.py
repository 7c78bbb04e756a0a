"""EP_NUM_TOPK_IDX_BITS=32 (deep_ep.topk_idx_t = int32) on the GPU, end to end and bitwise.

The kernels read the routing as int64 (include/deepep_amd.h); with int32 routing the host converts it
once per handle (EPHandle.routing_idx64).  The variable is read when deepep_amd is imported, so the
cases run in fresh children (tests/idx_bits_child.py, one at a time, never retried) that report the
topk_idx_t they saw; a child in which the variable did not take effect fails the test.  The cases are
grouped into three children because a child's start-up (importing torch, opening the GPU) costs more
than a case:

  ep1, graph                                    EP = 1 at T=129, H=520, K=3, E=9 against the 64-bit oracle
                                                (the non-expanded combine's weight pass-through reads the
                                                routing on the device); HIP graph capture at T=130;
  golden_ep1, golden_ep4, golden_ep4_chunks3    the 64-bit suite's _buffer_case over the fixtures: plan_source
  golden_ep8                                    and plan_expert with a 32-bit handle, top-k (R > K) and rank
                                                (R <= K) layouts, multiple and single reduction.
Every child is one process with the GPU open (thread ranks, tests/sim.py).
"""
import pytest
import torch

from tests.idx_bits_child import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('cases', [
    ('ep1', 'graph'),
    ('golden_ep1', 'golden_ep4', 'golden_ep4_chunks3'),
    ('golden_ep8',),
], ids=lambda c: '+'.join(c))
def test_int32_routing_end_to_end(cases):
    report = run_child(list(cases))
    print(report)
    assert report['topk_idx_t'] == 'torch.int32', report      # the variable took effect in the child
    assert report['device'] == 'cuda', report
    assert report['failures'] == [], report['failures']
    assert list(report['seconds']) == list(cases), report      # every case ran to its end


def test_build_local_plan_rejects_int32_routing():
    """The wrapper refuses routing the kernel would misread (4-byte entries read as 8-byte ones, past the
    end of the tensor) before any launch -- as the other wrappers' 'topk_idx int64' checks."""
    from deepep_amd.kernels import HipKernels
    kern = HipKernels()
    T, K = 5, 3
    meta = torch.full((T, K + 2), -1, dtype=torch.int32, device='cuda')
    plan = torch.full((T, 1), -7, dtype=torch.int32, device='cuda')
    wtable = torch.full((T, K), -7, dtype=torch.int32, device='cuda')
    idx64 = torch.zeros((T, K), dtype=torch.int64, device='cuda')
    for bad in (idx64.to(torch.int32), idx64.cpu(), torch.zeros((T, 2 * K), dtype=torch.int64, device='cuda')[:, ::2],
                None):
        with pytest.raises(RuntimeError, match='topk_idx int64'):
            kern.build_local_plan(meta, T, K, T, False, plan, T, bad, wtable)
    torch.cuda.synchronize()
    assert bool((plan == -7).all()) and bool((wtable == -7).all())      # nothing was launched
    # without a weight table the routing is not read: any dtype (or none) is accepted, as before
    kern.build_local_plan(meta, T, K, T, False, plan, T, idx64.to(torch.int32), None)
    kern.build_local_plan(meta, T, K, T, False, plan, T, idx64, wtable)
    torch.cuda.synchronize()
    assert bool((plan == -1).all()) and bool((wtable == -1).all())      # metadata -1: no received rows
