"""The expanded copy's inverse slot map holds every lane of every received row (no GPU).

dispatch_slots writes inv[slot] for every local lane of a received row, and the scan counts lanes, not distinct
experts: routing that names an expert twice in a token (tests/test_window_bounds_gpu.py does so on purpose) gives
a row more local lanes than min(K, local experts).  The map is therefore sized N * K + (alignment - 1) * local
experts; sized by min(K, local experts) the HIP kernel stored past the tensor, and the CPU stand-in -- which
indexes the same tensor -- raised IndexError."""
import os

import pytest
import torch
import torch.distributed as dist

from tests.fp8_oracle_kernels import Spy
from tests.oracle_kernels import OracleKernels


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29571')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


T, H, K, E = 8, 128, 4, 2


def _dispatch(group, expert_alignment):
    from deepep_amd import ElasticBuffer, topk_idx_t
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    spy = Spy(OracleKernels())
    buf._kernels = spy
    idx = torch.tensor([[0, 0, 1, 1]] * T, dtype=topk_idx_t)
    x = torch.randn((T, H), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    out = buf.dispatch(x, topk_idx=idx, topk_weights=torch.rand((T, K)), num_experts=E, do_expand=True,
                       do_cpu_sync=True, expert_alignment=expert_alignment)
    inv = [kw['inv'] for name, _, kw in spy.tensors if name == 'dispatch_receive']
    assert len(inv) == 1 and inv[0] is not None
    return out, inv[0]


def test_duplicate_routing_fits_the_inverse_slot_map(group):
    (recv_x, _, recv_w, handle, _), inv = _dispatch(group, 1)
    N = handle.num_recv_tokens
    assert N == T and inv.numel() >= N * K
    assert recv_x.shape[0] == 32 and handle.num_expanded_tokens == 32       # every lane counted: 8 rows x 4 lanes
    slots = handle.recv_src_metadata[:, 2:]
    assert int(slots.max()) == 31 and int(slots.max()) < inv.numel()


def test_inverse_slot_map_holds_every_lane_with_expert_alignment(group):
    (recv_x, _, _, handle, _), inv = _dispatch(group, 16)
    N = handle.num_recv_tokens
    assert inv.numel() >= N * K + (16 - 1) * E
    assert int(handle.recv_src_metadata[:, 2:].max()) < inv.numel()
    assert recv_x.shape[0] == 32 and handle.num_recv_tokens_per_expert_list == [16, 16]
