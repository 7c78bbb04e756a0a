"""deepep_dispatch_copy_cast (HipKernels.dispatch_copy_cast) on the GPU: the one-rank dispatch copy with the FP8
cast on the way, against the same build's dispatch_copy(x_direct = q, sf_direct = sf) fed the pair cast on the
CPU (workloads.per_token_cast_to_fp8; round_scale: tests/test_fp8_cast_gpu.py::cast_ref) -- bitwise, whole
pre-poisoned output buffers, in the row form, the blocked destination-major expanded form and the source-major
expanded form."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_fp8_cast_gpu import cast_ref  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_X, POISON_SF, POISON_W = 0x38, -7.0, -3.0


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


def _bf16_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _payload(H: int, round_scale: bool):
    """300 finite bf16 rows and their CPU cast (computed once per H and mode; tests take leading rows).
    Row 0: every group's amax sits in its last column; row 1: all zero (the 1e-4 clamp); rows 2 / 3 hold 448.0 /
    -448.0; row 4: denormals of both signs."""
    g = torch.Generator().manual_seed(H)
    x = (torch.randn((300, H), generator=g) * 3).to(torch.bfloat16)
    x[0, 127::128] = 100.0
    x[1] = 0
    x[2, 5], x[3, H - 3] = 448.0, -448.0
    den = np.arange(1, H + 1, dtype=np.uint16) % 127 + 1
    den[1::2] |= 0x8000
    x[4] = _bf16_bits(den)
    assert bool(x.float().isfinite().all())
    q, sf = cast_ref(x, round_scale)
    return x, q, sf


def _routing(T, K, E, kind, seed):
    """plain: top-k of uniform scores; masked: 20 % of the entries -1 and one token routed nowhere; skew: only
    the first half of the experts is used (the others stay empty) and expert 0 takes nearly every token."""
    g = torch.Generator().manual_seed(seed)
    scores = torch.rand((T, E), generator=g)
    if kind == 'skew':
        used = max(K, E // 2)
        scores[:, used:] = -1.0
        scores[:, 0] += 2.0
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    if kind == 'masked':
        first = int(idx[0, 0])
        idx[torch.rand(idx.shape, generator=g) < 0.2] = -1
        if T > 1:
            idx[T // 2] = -1
        idx[0, 0] = first                                      # at least one row is received
    return idx.to(torch.int64), w.masked_fill(idx < 0, 0)


def _tables(kern, idx, w, E, expanded, alignment):
    """The one-rank receive-side tables of this routing, by the HIP kernels: metadata-only packed rows, metadata,
    and (expanded) the slots' inverse map with the per-block offsets."""
    from deepep_amd._lib import DISPATCH_BLOCK_ROWS
    from deepep_amd.kernels import RowLayout
    T, K = idx.shape
    dev = idx.device
    layout = RowLayout.make(0, 0, K)
    dst = torch.empty((T, 1), dtype=torch.int32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    kern.dispatch_route(idx, E, 1, dst, cnt)
    n = int(cnt.item())
    assert n > 0
    packed = torch.zeros((n, layout.row_bytes), dtype=torch.uint8, device=dev)
    kern.dispatch_pack(torch.zeros((T, 16), dtype=torch.uint8, device=dev)[:, :0], None, idx, w, 0, dst,
                       torch.zeros((1,), dtype=torch.int32, device=dev), packed, layout)
    meta = torch.full((n, K + 2), -7, dtype=torch.int32, device=dev)
    bc = torch.empty(((n + DISPATCH_BLOCK_ROWS - 1) // DISPATCH_BLOCK_ROWS, E), dtype=torch.int32, device=dev)
    kern.dispatch_count(packed, layout, n, 0, E, torch.tensor([n], dtype=torch.int32, device=dev), meta, None, bc)
    ec = torch.empty((E,), dtype=torch.int32, device=dev)
    pe = torch.empty((E,), dtype=torch.int32, device=dev)
    kern.dispatch_scan(bc, E, alignment, expanded, ec, pe)
    inv, rows = None, n
    if expanded:
        rows = sum((int(c) + alignment - 1) // alignment * alignment for c in ec.tolist())
        inv = torch.full((max(rows, 1),), -9, dtype=torch.int32, device=dev)
        kern.dispatch_slots(packed, layout, n, 0, E, bc, meta, inv=inv)
    else:
        meta[:, 2:] = -1
    return dict(layout=layout, packed=packed, n=n, meta=meta, bc=bc, pe=pe, inv=inv, rows=rows, ec=ec)


def _outputs(rows, n, H, K, expanded, dev):
    return (torch.full((rows, H), POISON_X, dtype=torch.uint8, device=dev),
            torch.full((rows, H // 128), POISON_SF, dtype=torch.float32, device=dev),
            torch.full((rows,) if expanded else (n, K), POISON_W, dtype=torch.float32, device=dev))


def _compare_copy(kern, x_gpu, q, sf, idx, w, E, T_max, form, alignment, round_scale, tag):
    """dispatch_copy_cast(x) against dispatch_copy(the CPU-cast pair) into pre-poisoned outputs, whole buffers."""
    expanded = form != 'rows'
    t = _tables(kern, idx, w, E, expanded, alignment)
    T, K = idx.shape
    H = q.shape[1]
    blocked = dict(inv=t['inv'], block_offsets=t['bc'], expert_end=t['pe']) if form == 'blocked' else {}
    rx, rsf, rw = _outputs(t['rows'], t['n'], H, K, expanded, idx.device)
    kern.dispatch_copy(t['packed'], t['layout'], t['n'], t['meta'], expanded, rx, rsf.view(torch.uint8), rw,
                       x_direct=q.view(torch.uint8), sf_direct=sf.view(torch.uint8).view(T, -1),
                       num_max_tokens=T_max, **blocked)
    gx, gsf, gw = _outputs(t['rows'], t['n'], H, K, expanded, idx.device)
    kern.dispatch_copy_cast(t['packed'], t['layout'], t['n'], t['meta'], expanded, gx, gsf.view(torch.uint8), gw,
                            x_direct=x_gpu.view(torch.uint8), num_max_tokens=T_max, round_scale=round_scale,
                            **blocked)
    torch.cuda.synchronize()
    assert bool((rx != POISON_X).any()), tag                   # the reference rows were written
    bad = (gx != rx).nonzero()
    assert bad.numel() == 0, f'{tag}: {bad.shape[0]} fp8 bytes differ, first at row/column {bad[0].tolist()}'
    bad = (gsf.view(torch.int32) != rsf.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f'{tag}: {bad.shape[0]} scale factors differ, first at {bad[0].tolist()}'
    assert torch.equal(gw.view(torch.int32), rw.view(torch.int32)), f'{tag}: weights'
    return t


# T: 129 and 300 cross the 128-row receive block, 1 and 5 straddle the four rows in flight; K and E with
# masked (-1) entries and a skewed routing (empty experts, one expert with far more than 4 rows of a block)
CASES = [(1, 1, 1, 'plain'), (5, 3, 8, 'masked'), (5, 8, 8, 'plain'), (129, 1, 8, 'masked'), (129, 8, 64, 'masked'),
         (129, 3, 64, 'skew'), (300, 3, 8, 'skew'), (300, 8, 64, 'skew'), (300, 1, 1, 'plain')]


# H: one group (48 idle lanes of a 64-lane half), a partial wave, exactly one 2 KiB chunk, one group spilling
# into a second chunk, and the flagship 7168 (three and a half chunks)
@pytest.mark.parametrize('round_scale', [False, True])
@pytest.mark.parametrize('H', [128, 384, 2048, 2176, 7168])
def test_copy_cast_equals_copy_of_the_cpu_cast(kern, H, round_scale):
    x, q, sf = _payload(H, round_scale)
    x_gpu, q_gpu, sf_gpu = x.cuda(), q.cuda(), sf.cuda()
    skew_seen = False
    for T, K, E, kind in CASES:
        idx, w = _routing(T, K, E, kind, seed=T * 100 + K * 10 + E)
        idx, w = idx.cuda(), w.cuda()
        for form, alignment in (('rows', 1), ('blocked', 1), ('blocked', 4), ('source-major', 1)):
            t = _compare_copy(kern, x_gpu[:T], q_gpu[:T], sf_gpu[:T], idx, w, E, T + 3, form, alignment, round_scale,
                              f'T={T} K={K} E={E} {kind} {form} alignment={alignment}')
            if kind == 'skew' and E > 1 and form == 'blocked':
                ec = t['ec'].tolist()
                assert min(ec) == 0 and max(ec) > 4 * 8, ec     # empty experts, and one far above 4 rows a block
                skew_seen = True
    assert skew_seen


@pytest.mark.parametrize('round_scale', [False, True])
def test_copy_cast_strided_input_and_no_rows(kern, round_scale):
    H, T, K, E = 384, 129, 3, 8
    x, q, sf = _payload(H, round_scale)
    wide = torch.zeros((T, H + 8), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x[:T].cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 8 and not view.is_contiguous()
    idx, w = _routing(T, K, E, 'masked', seed=9)
    for form in ('rows', 'blocked'):
        _compare_copy(kern, view, q[:T].cuda(), sf[:T].cuda(), idx.cuda(), w.cuda(), E, T, form, 1, round_scale,
                      f'strided {form}')
    # no received rows: nothing is launched, nothing is written
    from deepep_amd.kernels import RowLayout
    layout = RowLayout.make(0, 0, K)
    gx, gsf, gw = _outputs(4, 0, H, K, False, 'cuda')
    kern.dispatch_copy_cast(torch.zeros((0, layout.row_bytes), dtype=torch.uint8, device='cuda'), layout, 0,
                            torch.zeros((0, K + 2), dtype=torch.int32, device='cuda'), False, gx, gsf.view(torch.uint8),
                            gw, x_direct=view.view(torch.uint8), num_max_tokens=T, round_scale=round_scale)
    torch.cuda.synchronize()
    assert bool((gx == POISON_X).all()) and bool((gsf == POISON_SF).all())


def test_copy_cast_wrapper_rejects_bad_arguments(kern):
    from deepep_amd.kernels import RowLayout
    T, H, K = 4, 128, 2
    layout = RowLayout.make(0, 0, K)
    dev = 'cuda'
    packed = torch.zeros((T, layout.row_bytes), dtype=torch.uint8, device=dev)
    meta = torch.full((T, K + 2), -1, dtype=torch.int32, device=dev)      # no received rows: nothing would be stored
    xb = torch.zeros((T, 2 * H), dtype=torch.uint8, device=dev)
    gx, gsf, gw = _outputs(T, T, H, K, False, dev)
    args = (packed, layout, T, meta, False)

    def call(rx=gx, rsf=gsf.view(torch.uint8), **kw):
        kern.dispatch_copy_cast(*args, rx, rsf, gw, **dict(dict(x_direct=xb, num_max_tokens=T), **kw))

    call()                                                                # the good call is accepted
    with pytest.raises(RuntimeError, match='x_direct'):
        call(x_direct=None)
    with pytest.raises(RuntimeError, match='sf_direct'):
        call(sf_direct=torch.zeros((T, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='128'):
        call(x_direct=torch.zeros((T, 384), dtype=torch.uint8, device=dev))           # hidden = 192
    with pytest.raises(RuntimeError, match='bf16'):
        call(x_direct=torch.zeros((T, H), dtype=torch.bfloat16, device=dev))          # not the byte view
    with pytest.raises(RuntimeError, match='outputs'):
        call(rsf=None)
    with pytest.raises(RuntimeError, match='outputs'):
        call(rx=torch.zeros((T, 2 * H), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='stride'):                                 # rows 2 * H + 8 bytes apart
        call(x_direct=torch.zeros((T, 2 * H + 8), dtype=torch.uint8, device=dev)[:, :2 * H])
    with pytest.raises(RuntimeError, match='blocked copy tables'):
        call(inv=torch.zeros((T,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert bool((gx == POISON_X).all())
