"""The expanded copy's inverse slot map on the GPU: the duplicate-routing case of tests/test_slot_map_cpu.py at
EP = 1 through the HIP kernels.  slots_kernel writes inv[slot] for every local lane of a received row, so every
slot the handle's metadata holds must lie inside the map the dispatch allocated -- checked by arithmetic on the
map's size, and in its general form by the same dispatch under the guard (tests/guard.py): no kernel of it stores
outside the outputs its wrapper declares."""
import os

import pytest
import torch

from tests.fp8_oracle_kernels import Spy

pytestmark = pytest.mark.gpu


def duplicate_routing_case(kernels=None):
    """kernels: the provider the spy forwards to (default: HipKernels())."""
    import torch.distributed as dist
    from deepep_amd import ElasticBuffer, topk_idx_t
    from deepep_amd.kernels import HipKernels
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29573')
        dist.init_process_group('gloo', rank=0, world_size=1)
    T, H, K, E = 8, 128, 4, 2
    buf = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    spy = Spy(HipKernels() if kernels is None else kernels)
    buf._kernels = spy
    idx = torch.tensor([[0, 0, 1, 1]] * T, dtype=topk_idx_t, device='cuda')
    x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    for alignment in (1, 16):
        del spy.tensors[:]
        _, _, _, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=torch.rand((T, K), device='cuda'),
                                          num_experts=E, do_expand=True, do_cpu_sync=True,
                                          expert_alignment=alignment)
        torch.cuda.synchronize()
        inv = [kw['inv'] for name, _, kw in spy.tensors if name == 'dispatch_receive']
        assert len(inv) == 1 and inv[0] is not None
        slots = handle.recv_src_metadata[:, 2:]
        assert inv[0].numel() >= T * K + (alignment - 1) * E
        # 16 lanes per expert: expert 1's rows start at slot 16 -- past a map of T * min(K, local experts) entries
        assert T * min(K, E) <= int(slots.max()) < inv[0].numel()


def test_duplicate_routing_stays_inside_the_inverse_slot_map():
    duplicate_routing_case()


def test_duplicate_routing_stores_nothing_outside_its_outputs():
    from deepep_amd.kernels import HipKernels
    from tests.guard import Guard
    guard = Guard(HipKernels())
    duplicate_routing_case(guard)
    assert guard.guarded_calls >= 4 and guard.verify() >= 4
