"""Rows more than 2^31 and 2^32 bytes from their base pointer: every wrapper argument whose C-ABI entry takes a
row stride is given a view into one large uninitialised allocation whose twenty rows lie 240 MiB apart, so that the
rows a case touches lie on both sides of 2^31 and of 2^32 bytes from the view's base (a 32k-token, top-8 batch at
H = 7168 has 3.76 GB of expanded rows).  Only the rows are initialised; the expected values are the CPU oracle's
over a compact copy of the same rows; everything is compared bit for bit.

One allocation of 4.55 GiB per test, released before the test returns; a test skips only when that allocation
itself runs out of memory."""
import pytest
import torch

from tests.fp8_combine_ref import Fp8CombineOracleKernels
from tests.oracle_kernels import OracleKernels
from tests.test_fp8_cast_gpu import cast_ref
from tests.ue8m0_ref import Ue8m0OracleKernels, pack_ref

pytestmark = pytest.mark.gpu

ROWS = 20
STRIDE = 240 << 20                           # bytes between rows: row 9 is the first past 2^31, row 18 past 2^32
SIDE = 64 << 20                              # a second far view of the same rows starts here (scale factors)
TOTAL = (ROWS - 1) * STRIDE + SIDE + (32 << 20)
UNITS, WIDTH = 40, 3
MODE_LOCAL, MODE_EPILOGUE, MODE_FUSED = 0, 1, 2

assert 8 * STRIDE < 2 ** 31 <= 9 * STRIDE and 17 * STRIDE < 2 ** 32 <= 18 * STRIDE and TOTAL <= 5 << 30


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


@pytest.fixture
def far():
    """view(dtype, columns, offset=0, row_stride=STRIDE, col_stride=None): a [ROWS, columns] view of the one large
    allocation, rows `row_stride` bytes apart from byte `offset` on."""
    try:
        big = torch.empty((TOTAL,), dtype=torch.uint8, device='cuda')
    except torch.OutOfMemoryError:
        pytest.skip(f'torch.OutOfMemoryError from the one allocation of {TOTAL} bytes the far-row cases need')
    views = []

    def view(dtype, columns, offset=0, row_stride=STRIDE, col_stride=None):
        size = torch.empty((), dtype=dtype).element_size()
        col = 1 if col_stride is None else col_stride // size
        v = torch.as_strided(big.view(dtype), (ROWS, columns), (row_stride // size, col), offset // size)
        assert v.data_ptr() == big.data_ptr() + offset
        views.append(v)
        return v

    yield view
    del views[:]
    del big, view
    torch.cuda.empty_cache()


def _sides(rows) -> None:
    """The rows a case touches lie below 2^31, between 2^31 and 2^32, and above 2^32 bytes from the base."""
    rows = sorted({int(r) for r in rows})
    at = [r * STRIDE for r in rows]
    assert any(a < 2 ** 31 for a in at) and any(2 ** 31 <= a < 2 ** 32 for a in at) and any(a >= 2 ** 32 for a in at), rows


def _rows(H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((ROWS, H), generator=g) * 3).to(torch.bfloat16)


def _table(seed):
    """[UNITS, WIDTH] slots into the ROWS rows: a fifth masked, unit 0 empty, and units that name the rows 0, 8, 9,
    17, 18 and 19 -- the last rows before and the first after 2^31 and 2^32 bytes."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, ROWS, (UNITS, WIDTH), generator=g, dtype=torch.int32)
    t[torch.rand((UNITS, WIDTH), generator=g) < 0.2] = -1
    t[0] = -1
    t[1] = torch.tensor([0, 9, 18])
    t[2] = torch.tensor([19, 8, 17])
    _sides(t[t >= 0].tolist())
    return t


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, f'{what}: {bad.shape[0]} bytes differ, first at {bad[0].tolist()}'


# ----------------------------------------------------------------------------- combine
@pytest.mark.parametrize('H', [520, 2560])
def test_combine_reduce_far_source_rows_and_far_output_rows(kern, far, H):
    x = _rows(H, H)
    src = far(torch.bfloat16, H)
    src.copy_(x.cuda())
    table = _table(H)
    g = torch.Generator().manual_seed(H + 1)
    row_w = torch.rand((ROWS,), generator=g)
    bias = torch.randn((UNITS, H), generator=g).to(torch.bfloat16)
    for mode, weighted, b in ((MODE_FUSED, False, None), (MODE_FUSED, True, bias), (MODE_LOCAL, True, None),
                              (MODE_EPILOGUE, False, bias)):
        out = torch.zeros((UNITS, H), dtype=torch.bfloat16, device='cuda')
        kern.combine_reduce(mode, src, out, UNITS, table=table.cuda(), row_weights=row_w.cuda() if weighted else None,
                            bias0=None if b is None else b.cuda())
        want = torch.zeros((UNITS, H), dtype=torch.bfloat16)
        OracleKernels().combine_reduce(mode, x, want, UNITS, table=table, row_weights=row_w if weighted else None,
                                       bias0=b)
        torch.cuda.synchronize()
        _same(out, want, f'far source rows, mode {mode}, weighted {weighted}')
    # the output rows far apart (one unit per row), the source rows compact; the view shares the allocation
    table20 = table[:ROWS].clone()
    table20[9], table20[18] = torch.tensor([3, -1, 5]), torch.tensor([7, 7, 1])
    _sides(range(ROWS))
    out = far(torch.bfloat16, H, offset=SIDE)
    out.copy_(torch.full((ROWS, H), 7.0, dtype=torch.bfloat16, device='cuda'))
    for mode in (MODE_FUSED, MODE_LOCAL):
        kern.combine_reduce(mode, x.cuda(), out, ROWS, table=table20.cuda())
        want = torch.zeros((ROWS, H), dtype=torch.bfloat16)
        OracleKernels().combine_reduce(mode, x, want, ROWS, table=table20)
        torch.cuda.synchronize()
        _same(out, want, f'far output rows, mode {mode}')


@pytest.mark.parametrize('H', [128, 2560])
def test_fp8_combine_far_source_rows_and_far_scale_factors(kern, far, H):
    x = _rows(H, H + 2)
    table = _table(H + 3)
    oracle = Fp8CombineOracleKernels()
    q, sf = cast_ref(x, False)
    forms = [('fp32, rows far apart', q, sf, dict())]
    if H // 128 >= ROWS:                      # 20 factors a row: the columns far apart instead (column-major factors)
        forms.append(('fp32, columns far apart', q, sf, dict(row_stride=4, col_stride=STRIDE)))
    if H % 512 == 0:
        q2, sf2 = cast_ref(x, True)
        forms.append(('packed UE8M0, rows far apart', q2, pack_ref(sf2), dict()))
    for label, qc, sfc, strides in forms:
        src = far(torch.float8_e4m3fn, H)
        src.view(torch.uint8).copy_(qc.view(torch.uint8).cuda())
        if 'col_stride' in strides:
            assert sfc.shape == (ROWS, ROWS)
        src_sf = far(sfc.dtype, sfc.shape[1], offset=SIDE, **strides)
        src_sf.copy_(sfc.cuda())
        for mode in (MODE_FUSED, MODE_LOCAL):
            out = torch.zeros((UNITS, H), dtype=torch.bfloat16, device='cuda')
            kern.combine_reduce(mode, src, out, UNITS, table=table.cuda(), src_sf=src_sf)
            want = torch.zeros((UNITS, H), dtype=torch.bfloat16)
            oracle.combine_reduce(mode, qc, want, UNITS, table=table, src_sf=sfc)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(want.float()).all())
            _same(out, want, f'{label}, mode {mode}')


@pytest.mark.parametrize('H,fp8', [(520, False), (2560, False), (128, True), (2560, True)])
def test_combine_reduce_scatter_far_source_rows(kern, far, H, fp8):
    """Phase A of the xGMI transport over far source rows; its output rows go to a small window of their own."""
    x = _rows(H, H + 4)
    table = _table(H + 5)
    g = torch.Generator().manual_seed(H + 6)
    row_w = torch.rand((ROWS,), generator=g)
    if fp8:
        q, sf = cast_ref(x, False)
        src = far(torch.float8_e4m3fn, H)
        src.view(torch.uint8).copy_(q.view(torch.uint8).cuda())
        src_sf = far(torch.float32, H // 128, offset=SIDE)
        src_sf.copy_(sf.cuda())
        kw, cpu_src, cpu_kw = dict(src_sf=src_sf), q, dict(src_sf=sf)
    else:
        src = far(torch.bfloat16, H)
        src.copy_(x.cuda())
        kw, cpu_src, cpu_kw = dict(), x, dict()
    row_bytes = H * 2 + 64
    win = torch.zeros((UNITS * row_bytes,), dtype=torch.uint8, device='cuda')
    addr = torch.arange(UNITS, dtype=torch.int64, device='cuda') * row_bytes + win.data_ptr()
    kern.combine_reduce_scatter(src, UNITS, addr, table=table.cuda(), row_weights=row_w.cuda(),
                                windows=(torch.tensor([win.data_ptr()], device='cuda'), win.numel()), **kw)
    want = torch.zeros((UNITS, H), dtype=torch.bfloat16)
    Fp8CombineOracleKernels().combine_reduce(MODE_LOCAL, cpu_src, want, UNITS, table=table, row_weights=row_w, **cpu_kw)
    torch.cuda.synchronize()
    got = win.cpu().view(UNITS, row_bytes)[:, :H * 2].contiguous().view(torch.bfloat16)
    _same(got, want, 'scattered rows')


# ----------------------------------------------------------------------------- casts
@pytest.mark.parametrize('H', [128, 2560])
def test_cast_fp8_far_input_rows(kern, far, H):
    x = _rows(H, H + 7)
    xs = far(torch.bfloat16, H)
    xs.copy_(x.cuda())
    _sides(range(ROWS))
    for round_scale in (False, True):
        q = torch.zeros((ROWS, H), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
        sf = torch.zeros((ROWS, H // 128), device='cuda')
        kern.cast_fp8(xs, q, sf, round_scale)
        torch.cuda.synchronize()
        q_ref, sf_ref = cast_ref(x, round_scale)
        _same(q, q_ref, f'fp8 bytes, round_scale {round_scale}')
        _same(sf, sf_ref, f'scale factors, round_scale {round_scale}')
    if H % 512 == 0:
        q = torch.zeros((ROWS, H), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
        sf = torch.zeros((ROWS, H // 512), dtype=torch.int32, device='cuda')
        kern.cast_fp8(xs, q, sf, True, ue8m0=True)
        torch.cuda.synchronize()
        q_ref, sf_ref = cast_ref(x, True)
        _same(q, q_ref, 'fp8 bytes, UE8M0')
        _same(sf, pack_ref(sf_ref), 'packed scale factors')


@pytest.mark.parametrize('H', [128, 2560])
def test_cast_back_fp8_far_rows_and_far_scale_factors(kern, far, H):
    from tests.test_cast_back_gpu import back_ref
    x = _rows(H, H + 8)
    q, sf = cast_ref(x, False)
    _sides(range(ROWS))
    forms = [('fp32, rows far apart', q, sf, sf, dict())]
    if H // 128 >= ROWS:
        forms.append(('fp32, columns far apart', q, sf, sf, dict(row_stride=4, col_stride=STRIDE)))
    if H % 512 == 0:
        q2, sf2 = cast_ref(x, True)
        forms.append(('packed UE8M0, rows far apart', q2, pack_ref(sf2), sf2, dict()))
    for label, qc, sfc, sf_fp32, strides in forms:
        qs = far(torch.float8_e4m3fn, H)
        qs.view(torch.uint8).copy_(qc.view(torch.uint8).cuda())
        sfs = far(sfc.dtype, sfc.shape[1], offset=SIDE, **strides)
        sfs.copy_(sfc.cuda())
        out = torch.zeros((ROWS, H), dtype=torch.bfloat16, device='cuda')
        kern.cast_back_fp8(qs, sfs, out)
        torch.cuda.synchronize()
        want = back_ref(qc, sf_fp32)
        assert bool(torch.isfinite(want.float()).all())
        _same(out, want, label)


# ----------------------------------------------------------------------------- dispatch
def _routing(K, E, seed):
    """ROWS tokens: a fifth of the entries masked, token 5 routed nowhere, the tokens on each side of 2^31 and 2^32
    bytes routed somewhere."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(ROWS)])
    keep = idx[:, 0].clone()
    idx[torch.rand((ROWS, K), generator=g) < 0.2] = -1
    idx[:, 0] = keep
    idx[5] = -1
    w = torch.rand((ROWS, K), generator=g) * (idx >= 0)
    _sides((idx >= 0).any(dim=1).nonzero().view(-1).tolist())
    return idx.to(torch.int64), w


@pytest.mark.parametrize('H', [128, 2560])
def test_dispatch_pack_and_pack_cast_far_token_rows(kern, far, H):
    from deepep_amd.kernels import RowLayout
    K, E, R = 3, 8, 2
    x = _rows(H, H + 9)
    idx, w = _routing(K, E, H + 10)
    cpu = Ue8m0OracleKernels()
    dst, cnt = torch.empty((ROWS, R), dtype=torch.int32), torch.empty((R,), dtype=torch.int32)
    cpu.dispatch_route(idx, E, R, dst, cnt)
    offs = (torch.cumsum(cnt, 0) - cnt).to(torch.int32)
    rows = int(cnt.sum())
    xs = far(torch.bfloat16, H)
    xs.copy_(x.cuda())
    q, sf = cast_ref(x, False)
    sf_bytes = sf.view(torch.uint8).view(ROWS, -1)
    sfs = far(torch.uint8, sf_bytes.shape[1], offset=SIDE)
    sfs.copy_(sf_bytes.cuda())
    gpu = [t.cuda() for t in (idx, w, dst, offs)]

    def both(call, layout):
        got = torch.zeros((rows, layout.row_bytes), dtype=torch.uint8, device='cuda')
        want = torch.zeros((rows, layout.row_bytes), dtype=torch.uint8)
        call(kern, got, *gpu)
        call(cpu, want, idx, w, dst, offs)
        torch.cuda.synchronize()
        return got, want

    # the bf16 rows and (as the FP8 tuple dispatch sends them) byte rows with far scale factors beside them
    layout = RowLayout.make(2 * H, sf_bytes.shape[1], K)
    x_cpu_bytes = x.view(torch.uint8).view(ROWS, 2 * H)
    got, want = both(lambda k, packed, i, ww, d, o: k.dispatch_pack(
        xs.view(torch.uint8) if packed.is_cuda else x_cpu_bytes, sfs if packed.is_cuda else sf_bytes, i, ww, 1000, d, o,
        packed, layout), layout)
    _same(got, want, 'dispatch_pack')
    for round_scale, ue8m0 in ((False, False), (True, False)) + (((True, True),) if H % 512 == 0 else ()):
        layout = RowLayout.make(H, H // 128 * (1 if ue8m0 else 4), K)
        kw = dict(round_scale=round_scale, **(dict(ue8m0=True) if ue8m0 else {}))
        got, want = both(lambda k, packed, i, ww, d, o: k.dispatch_pack_cast(
            xs.view(torch.uint8) if packed.is_cuda else x_cpu_bytes, i, ww, 1000, d, o, packed, layout, **kw), layout)
        _same(got, want, f'dispatch_pack_cast {kw}')


@pytest.mark.parametrize('H', [128, 2560])
def test_direct_copies_far_sender_rows(kern, far, H):
    """The one-rank copies that read the sender's rows in place: dispatch_copy(x_direct, sf_direct) and
    dispatch_copy_cast(x_direct), row form and blocked expanded form."""
    from tests.test_fp8_dispatch_gpu import _tables
    K, E = 3, 8
    x = _rows(H, H + 11)
    idx, w = _routing(K, E, H + 12)
    cpu = Ue8m0OracleKernels()
    q, sf = cast_ref(x, False)
    q_bytes, sf_bytes = q.view(torch.uint8), sf.view(torch.uint8).view(ROWS, -1)
    xs = far(torch.bfloat16, H)
    xs.copy_(x.cuda())
    qs = far(torch.uint8, H, offset=SIDE)
    qs.copy_(q_bytes.cuda())
    sfs = far(torch.uint8, sf_bytes.shape[1], offset=SIDE + (16 << 20))
    sfs.copy_(sf_bytes.cuda())
    x_cpu_bytes = x.view(torch.uint8).view(ROWS, 2 * H)
    for expanded in (False, True):
        t = _tables(kern, idx.cuda(), w.cuda(), E, expanded, 4 if expanded else 1)
        torch.cuda.synchronize()
        _sides((t['meta'][:, 0].cpu() % ROWS).tolist())
        blocked = dict(inv=t['inv'], block_offsets=t['bc'], expert_end=t['pe']) if expanded else {}
        host = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}
        blocked_cpu = dict(inv=host['inv'], block_offsets=host['bc'], expert_end=host['pe']) if expanded else {}
        cases = [('dispatch_copy', 4, lambda k, dev: dict(x_direct=qs if dev else q_bytes,
                                                         sf_direct=sfs if dev else sf_bytes))]
        for round_scale, ue8m0 in ((False, False), (True, False)) + (((True, True),) if H % 512 == 0 else ()):
            kw = dict(round_scale=round_scale, **(dict(ue8m0=True) if ue8m0 else {}))
            cases.append(('dispatch_copy_cast', 1 if ue8m0 else 4,
                          lambda k, dev, kw=kw: dict(x_direct=xs.view(torch.uint8) if dev else x_cpu_bytes, **kw)))
        for name, sf_width, args in cases:
            outs = []
            for k, dev, tab, blk in ((kern, 'cuda', t, blocked), (cpu, 'cpu', host, blocked_cpu)):
                rx = torch.zeros((tab['rows'], H), dtype=torch.uint8, device=dev)
                rsf = torch.zeros((tab['rows'], H // 128 * sf_width), dtype=torch.uint8, device=dev)
                rw = torch.zeros((tab['rows'],) if expanded else (tab['n'], K), dtype=torch.float32, device=dev)
                getattr(k, name)(tab['packed'], tab['layout'], tab['n'], tab['meta'], expanded, rx, rsf, rw,
                                 num_max_tokens=ROWS, **blk, **args(k, dev == 'cuda'))
                outs.append((rx, rsf, rw))
            torch.cuda.synchronize()
            for got, want, what in zip(outs[0], outs[1], ('rows', 'scale factors', 'weights')):
                _same(got, want, f'{name} expanded={expanded} {what}')
            assert bool((outs[1][0] != 0).any())
