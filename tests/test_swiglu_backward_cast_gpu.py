"""swiglu_backward_cast_to_mx on the GPU, over the three formats.  Rule 1: dh = [dgate | dup] against the formula in
fp64, each element within 2^-7 |ref| + 2^-126 (one bf16 ulp plus a flushed subnormal).  Rule 2: every pair bit for bit
the library's own cast of that dh -- compared on bytes.  Inputs are randn * 4 in bf16, fixed seeds."""
import pytest
import torch

pytestmark = pytest.mark.gpu
formats = pytest.mark.parametrize('fmt', ('fp8', 'fp6', 'fp4'))
SENTINEL = 0xa5


def _inputs(N, I, seed, wide_h=0, wide_dact=0):
    """h [N, 2 * I] and dact [N, I]; wide_*: as a column slice of a tensor that many columns wider (strided rows)."""
    g = torch.Generator().manual_seed(seed)
    new = lambda cols, wide: (torch.randn((N, cols + wide), generator=g) * 4).to(torch.bfloat16).cuda()[
        :, wide // 2:wide // 2 + cols]
    return new(2 * I, wide_h), new(I, wide_dact)


def _check_dh(h, dact, dh):
    """Rule 1."""
    I = dact.shape[1]
    g, u, da = h[:, :I].double(), h[:, I:].double(), dact.double()
    s = torch.sigmoid(g)
    ref = torch.cat([da * u * s * (1 + g * (1 - s)), da * g * s], dim=1)
    err, bound = (dh.double() - ref).abs(), 2.0 ** -7 * ref.abs() + 2.0 ** -126
    print('largest error / bound:', float((err / bound).max()))
    assert dh.dtype == torch.bfloat16 and tuple(dh.shape) == tuple(h.shape) and bool((err <= bound).all())


def _rowwise(fmt, dh):
    import deepep_amd
    if fmt == 'fp8':
        return deepep_amd.per_token_cast_to_fp8(dh, round_scale=True, use_ue8m0=True, group_size=32)
    return getattr(deepep_amd, f'per_token_cast_to_{fmt}')(dh)


def _same(got, want):
    return got.shape == want.shape and torch.equal(got.view(torch.uint8), want.view(torch.uint8))


@formats
@pytest.mark.parametrize('N,I,wide_h,wide_dact', [(1, 128, 0, 0), (17, 384, 0, 0), (131, 128, 0, 0), (131, 384, 0, 0),
                                                  (17, 128, 64, 0), (17, 128, 0, 32)])
def test_the_row_wise_kernel(fmt, N, I, wide_h, wide_dact):
    import deepep_amd
    h, dact = _inputs(N, I, N + I, wide_h, wide_dact)
    assert h.is_contiguous() == (wide_h == 0) and dact.is_contiguous() == (wide_dact == 0)
    q, sf, dh = deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, return_dh=True)
    _check_dh(h, dact, dh)
    want = _rowwise(fmt, dh)
    assert q.dtype == want[0].dtype and _same(q, want[0]) and _same(sf, want[1])
    q2, sf2 = deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt)         # the same bits without dh
    assert _same(q2, q) and _same(sf2, sf)


@formats
@pytest.mark.parametrize('N,I', [(128, 128), (128, 384), (640, 128), (640, 384), (512, 128)])    # 512: 16-byte sf_t
def test_the_tile_kernel(fmt, N, I):
    import deepep_amd
    h, dact = _inputs(N, I, N + I)
    (q, sf), (q_t, sf_t), dh = deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, with_transposed=True, return_dh=True)
    _check_dh(h, dact, dh)
    (wq, wsf), (wq_t, wsf_t) = getattr(deepep_amd, f'cast_to_mx{fmt}_transposed')(dh, with_rowwise=True)
    assert _same(q, wq) and _same(sf, wsf) and _same(q_t, wq_t) and _same(sf_t, wsf_t)
    rq, rsf, rdh = deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, return_dh=True)
    assert _same(q, rq) and _same(sf, rsf) and _same(dh, rdh)


@formats
@pytest.mark.parametrize('with_transposed', [False, True])
def test_rows_past_the_last_experts_aligned_end_are_neither_read_nor_written(fmt, with_transposed):
    """expert_ends = [100, 130] at alignment 128: rows 0-255 are live, rows 256-383 of h and of dact are NaN and every
    byte of theirs in the outputs keeps its sentinel."""
    from deepep_amd import kernels
    N, I, live = 384, 256, 256
    mx = next(m for m in kernels.MX_FORMATS if m.name == fmt)
    h, dact = _inputs(N, I, 7)
    h[live:] = float('nan')
    dact[live:] = float('nan')
    ends = torch.tensor([100, 130], dtype=torch.int32, device='cuda')

    def run(h, dact, ends):
        n = h.shape[0]
        new = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.uint8, device='cuda')
        out = dict(q=new(n, mx.row_bytes(2 * I)).view(mx.out_dtype), sf=new(n, I // 16),
                   dh=new(n, 4 * I).view(torch.bfloat16))
        if with_transposed:
            out.update(q_t=new(2 * I, mx.row_bytes(n)).view(mx.out_dtype), sf_t=new(2 * I, n // 32))
        kernels.HipKernels().swiglu_backward_cast_mx(mx, h, dact, expert_ends=ends, expert_alignment=128, **out)
        return {k: v.view(torch.uint8) for k, v in out.items()}

    got, want = run(h, dact, ends), run(h[:live], dact[:live], None)
    for k in got:
        cut = want[k].shape[0] if k in ('q', 'sf', 'dh') else None
        head, tail = (got[k][:cut], got[k][cut:]) if cut else (got[k][:, :want[k].shape[1]], got[k][:, want[k].shape[1]:])
        assert torch.equal(head, want[k]), k
        assert tail.numel() == got[k].numel() // 3 and bool((tail == SENTINEL).all()), k
    assert not bool((want['q'] == SENTINEL).all())


@formats
def test_no_rows(fmt):
    import deepep_amd
    from deepep_amd import kernels
    mx = next(m for m in kernels.MX_FORMATS if m.name == fmt)
    h = torch.empty((0, 256), dtype=torch.bfloat16, device='cuda')
    (q, sf), (q_t, sf_t), dh = deepep_amd.swiglu_backward_cast_to_mx(h, h[:, :128], mx, with_transposed=True,
                                                                     return_dh=True)
    assert tuple(q.shape) == (0, mx.row_bytes(256)) and tuple(sf.shape) == (0, 8) and tuple(dh.shape) == (0, 256)
    assert tuple(q_t.shape) == (256, 0) and tuple(sf_t.shape) == (256, 0) and q.dtype == q_t.dtype == mx.out_dtype
    assert sf.dtype == sf_t.dtype == torch.uint8 and dh.dtype == torch.bfloat16
