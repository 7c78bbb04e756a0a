"""The FP8 cast kernels on the GPU: deepep_cast_fp8 (HipKernels.cast_fp8, deepep_amd.per_token_cast_to_fp8)
and deepep_dispatch_pack_cast (HipKernels.dispatch_pack_cast) against a torch restatement of the cast run on
the CPU -- bitwise.

The default mode restates per_token_cast_to_fp8 (workloads.py; the reference's deep_ep/utils/math.py:30-39),
round_scale restates calculate_fp8_scales(round_scale=true) (csrc/kernels/legacy/utils.cuh:494-503).
The casting pack is compared with the existing pack kernel fed the CPU-cast pair of the same x."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from workloads import per_token_cast_to_fp8  # noqa: E402

pytestmark = pytest.mark.gpu


def cast_ref(x: torch.Tensor, round_scale: bool = False):
    """(q float8_e4m3fn [T, H], sf float32 [T, H / 128]) of a bf16 x, computed on the CPU."""
    x = x.cpu()
    assert x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0
    m, n = x.shape
    if m == 0:
        return torch.empty((0, n), dtype=torch.float8_e4m3fn), torch.empty((0, n // 128), dtype=torch.float32)
    if not round_scale:
        return per_token_cast_to_fp8(x)
    view = x.view(m, -1, 128)
    amax = view.abs().float().amax(dim=2).clamp(1e-4)
    bits = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    sf = ((e + 127) << 23).view(torch.float32)
    scale = ((127 - e) << 23).view(torch.float32)
    q = (view.float() * scale.unsqueeze(2)).to(torch.float8_e4m3fn).view(m, n).contiguous()
    return q, sf.contiguous()


def _bf16_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.uint8).cpu()


def _same(a, b) -> bool:
    """Bitwise equality of tensors / tuples of tensors / None (dtype and shape included)."""
    if isinstance(a, tuple) or isinstance(b, tuple):
        return isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b) and \
            all(_same(p, q) for p, q in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_u8(a), _u8(b))


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


def _gpu_cast(kern, x: torch.Tensor, round_scale: bool):
    T, H = x.shape
    q = torch.full((T, H), 1.0, dtype=torch.float32, device='cuda').to(torch.float8_e4m3fn)     # poison: 0x38
    sf = torch.full((T, H // 128), -7.0, dtype=torch.float32, device='cuda')
    kern.cast_fp8(x, q, sf, round_scale)
    torch.cuda.synchronize()
    return q, sf


def _check_cast(kern, x_cpu: torch.Tensor, round_scale: bool, x_gpu=None):
    q_ref, sf_ref = cast_ref(x_cpu, round_scale)
    q, sf = _gpu_cast(kern, x_cpu.cuda() if x_gpu is None else x_gpu, round_scale)
    bad_q = (_u8(q) != _u8(q_ref)).nonzero()
    bad_sf = (sf.cpu().view(torch.int32) != sf_ref.view(torch.int32)).nonzero()
    assert bad_sf.numel() == 0, f'{bad_sf.shape[0]} scale factors differ, first at {bad_sf[0].tolist()}: ' \
                                f'{sf.cpu()[tuple(bad_sf[0])]} != {sf_ref[tuple(bad_sf[0])]}'
    assert bad_q.numel() == 0, f'{bad_q.shape[0]} fp8 codes differ, first at {bad_q[0].tolist()}: ' \
                               f'{_u8(q)[tuple(bad_q[0])]:#x} != {_u8(q_ref)[tuple(bad_q[0])]:#x} ' \
                               f'(x = {x_cpu[tuple(bad_q[0])].item()})'
    return q_ref, sf_ref


# ----------------------------------------------------------------------------- 1. the kernel, exhaustive
def _exhaustive_matrix() -> torch.Tensor:
    """Every finite bf16 with |x| <= 448 (0x0000..0x43e0, both signs: 34,754 values), 127 per 128-column
    group behind a leading 448.0 anchor (default-mode factor 448 / 448 = 1), zero-padded to [92, 384]."""
    mag = np.arange(0x43e0 + 1, dtype=np.uint16)
    vals = np.concatenate([mag, mag | np.uint16(0x8000)])
    assert vals.size == 34754
    groups = 92 * 3
    body = np.zeros((groups * 127,), np.uint16)
    body[:vals.size] = vals
    mat = np.concatenate([np.full((groups, 1), 0x43e0, np.uint16), body.reshape(groups, 127)], axis=1)
    return _bf16_bits(mat.reshape(92, 384))


@pytest.mark.parametrize('round_scale', [False, True])
def test_cast_kernel_exhaustive(kern, round_scale):
    x = _exhaustive_matrix()
    q_ref, sf_ref = _check_cast(kern, x, round_scale)
    if not round_scale:
        # the expected values themselves: factor 1, so the cast is the plain fp32 -> e4m3fn conversion
        assert torch.equal(_u8(q_ref), _u8(x.float().to(torch.float8_e4m3fn)))
        assert not bool(((_u8(q_ref) & 0x7f) == 0x7f).any())             # no NaN code
        assert torch.equal(sf_ref, torch.ones_like(sf_ref))


# ----------------------------------------------------------------------------- 2. shapes and edges
@pytest.mark.parametrize('round_scale', [False, True])
@pytest.mark.parametrize('T', [1, 3, 65])
@pytest.mark.parametrize('H', [128, 384, 7168])
def test_cast_kernel_shapes(kern, T, H, round_scale):
    g = torch.Generator().manual_seed(T * 10007 + H)
    x = (torch.randn((T, H), generator=g) * 3).to(torch.bfloat16)
    _check_cast(kern, x, round_scale)


@pytest.mark.parametrize('round_scale', [False, True])
def test_cast_kernel_edge_rows(kern, round_scale):
    g = torch.Generator().manual_seed(2)
    H = 384
    x = (torch.randn((5, H), generator=g) * 3).to(torch.bfloat16)
    x[0, 128:256] = 0                                                    # an all-zero group: the 1e-4 clamp
    x[1, :128] = 0
    x[1, 7] = _bf16_bits(np.array([0x7f7f], np.uint16))[0]               # the largest finite bf16 ...
    x[1, 100] = -1.0                                                     # ... and -1.0: underflows to -0
    den = np.arange(1, 129, dtype=np.uint16)                             # bf16 denormals, both signs
    den[1::2] |= 0x8000
    x[2, 256:] = _bf16_bits(den)
    x[3, :128] = _bf16_bits(np.array([0x8000], np.uint16))[0]            # a group of -0
    q_ref, sf_ref = _check_cast(kern, x, round_scale)
    # what the expected values are at the edges (so the comparison above checked what it should)
    assert _u8(q_ref)[1, 100].item() == 0x80 and bool((_u8(q_ref)[3, :128] == 0x80).all())
    if not round_scale:
        assert _u8(q_ref)[1, 7].item() == 0x7e                            # amax itself: 448
        clamp = (torch.tensor(1e-4, dtype=torch.float32) / 448.0).item()
        assert sf_ref[0, 1].item() == clamp and sf_ref[2, 2].item() == clamp and sf_ref[3, 0].item() == clamp
    # an input whose row stride is larger than H * 2 bytes
    wide = torch.zeros((5, H + 8), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x.cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 8 and not view.is_contiguous()
    _check_cast(kern, x, round_scale, x_gpu=view)
    # no rows: nothing to do
    q0, sf0 = _gpu_cast(kern, torch.empty((0, H), dtype=torch.bfloat16, device='cuda'), round_scale)
    assert q0.shape == (0, H) and sf0.shape == (0, 3)


def test_cast_wrapper_rejects_bad_arguments(kern):
    x = torch.zeros((4, 192), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(RuntimeError):
        kern.cast_fp8(x, torch.empty((4, 192), dtype=torch.float8_e4m3fn, device='cuda'),
                      torch.empty((4, 1), dtype=torch.float32, device='cuda'))
    x = torch.zeros((4, 128), dtype=torch.float32, device='cuda')
    with pytest.raises(RuntimeError):
        kern.cast_fp8(x, torch.empty((4, 128), dtype=torch.float8_e4m3fn, device='cuda'),
                      torch.empty((4, 1), dtype=torch.float32, device='cuda'))


# ----------------------------------------------------------------------------- 3. the public function
@pytest.mark.parametrize('round_scale', [False, True])
def test_public_cast_function(round_scale):
    import deepep_amd
    g = torch.Generator().manual_seed(77)
    x = (torch.randn((67, 384), generator=g) * 3).to(torch.bfloat16)
    q_ref, sf_ref = cast_ref(x, round_scale)
    wide = torch.zeros((67, 400), dtype=torch.bfloat16, device='cuda')
    wide[:, :384] = x.cuda()
    for xin in (x.cuda(), wide[:, :384]):                               # contiguous, and rows 800 bytes apart
        q, sf = deepep_amd.per_token_cast_to_fp8(xin, round_scale=round_scale)
        torch.cuda.synchronize()
        assert q.dtype == torch.float8_e4m3fn and q.is_contiguous() and sf.dtype == torch.float32
        assert _same(q, q_ref) and _same(sf, sf_ref)
    q0, sf0 = deepep_amd.per_token_cast_to_fp8(torch.empty((0, 256), dtype=torch.bfloat16, device='cuda'))
    assert q0.shape == (0, 256) and sf0.shape == (0, 2)


# ----------------------------------------------------------------------------- 4. the casting pack
def _routes(T, K, E, R, seed):
    """topk_idx with -1 entries and a token routed nowhere; dst_slot [T, R] (rank among the earlier tokens
    routed to r, else -1), send_offsets [R] (exclusive prefix of the per-rank counts), total rows."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)])
    idx[torch.rand((T, K), generator=g) < 0.2] = -1
    idx[T // 2] = -1
    w = torch.rand((T, K), generator=g) * (idx >= 0)
    epr = E // R
    rank_of = torch.where(idx >= 0, idx // epr, torch.full_like(idx, -1))
    is_to = (rank_of.unsqueeze(-1) == torch.arange(R).view(1, 1, R)).any(dim=1)
    dst_slot = torch.where(is_to, torch.cumsum(is_to.to(torch.int64), 0) - 1, torch.full(is_to.shape, -1)).to(torch.int32)
    counts = is_to.sum(dim=0)
    send_offsets = (torch.cumsum(counts, 0) - counts).to(torch.int32)
    return idx, w, dst_slot, send_offsets, int(counts.sum())


@pytest.mark.parametrize('round_scale', [False, True])
@pytest.mark.parametrize('peer', [False, True])
@pytest.mark.parametrize('T,H,K', [(33, 256, 4), (3, 7168, 8), (70, 640, 2)])
def test_pack_cast_equals_pack_of_the_cpu_cast(kern, T, H, K, peer, round_scale):
    """deepep_dispatch_pack_cast(x) writes the rows deepep_dispatch_pack writes for the CPU-cast (q, sf) of the
    same x: fp8 bytes, scale factors, top-k indices, weights and source index, for every destination; in one
    local buffer and (peer) through per-destination base addresses with system-scope stores.  H = 640: the
    last 1 KiB step of a row is partial (5 groups); T = 70: more than one wave's worth of rows per rank."""
    from deepep_amd.kernels import RowLayout
    R, E = 4, 16
    dev = torch.device('cuda')
    idx, w, dst_slot, send_offsets, rows = _routes(T, K, E, R, seed=T * 31 + H)
    x = _payload(T, H, T + H)
    q, sf = cast_ref(x, round_scale)
    layout = RowLayout.make(H, H // 128 * 4, K)
    idx, w, dst_slot, send_offsets = idx.to(dev), w.to(dev), dst_slot.to(dev), send_offsets.to(dev)
    ref = torch.zeros((rows + 2, layout.row_bytes), dtype=torch.uint8, device=dev)      # 2 canary rows behind
    got = torch.zeros_like(ref)
    kern.dispatch_pack(q.to(dev).view(torch.uint8), sf.to(dev).view(torch.uint8).view(T, -1), idx, w, 1000, dst_slot,
                       send_offsets, ref[:rows], layout)
    x_bytes = x.to(dev).view(torch.uint8).view(T, 2 * H)
    if peer:
        bases = torch.full((R,), got.data_ptr(), dtype=torch.int64, device=dev)
        kern.dispatch_pack_cast(x_bytes, idx, w, 1000, dst_slot, send_offsets, None, layout, round_scale=round_scale,
                                dest_bases=bases, dest_rows=rows)
    else:
        kern.dispatch_pack_cast(x_bytes, idx, w, 1000, dst_slot, send_offsets, got[:rows], layout,
                                round_scale=round_scale)
    torch.cuda.synchronize()
    assert bool((ref[:rows, :H] != 0).any())                             # the reference rows were written
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} bytes differ, first at row/byte {bad[0].tolist()} ' \
                             f'(sf at {layout.sf_off}, idx at {layout.idx_off})'


def _payload(T, H, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((T, H), generator=g) * scale).to(torch.bfloat16)
