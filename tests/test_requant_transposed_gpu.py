"""requant_mxfp8_transposed / requant_mxfp4_transposed / requant_mxfp6_transposed on the GPU, all five forms (an FP8
pair with fp32, packed UE8M0 or per-32 exponent-byte factors; an MXFP4 pair; an MXFP6 pair), bit for bit against
tests/requant_t_ref (the transposed cast's reference of the cast back's reference): the shapes at which the tiling has
tails, strided code rows, column-major factors, the dtype views, every finite code in every token position, padding
rows, the independence of a block from its neighbours, the inverse, a graph capture, the rows of a casting dispatch and
the empty input.  Every comparison is on bytes."""
import functools

import pytest
import torch

from tests.requant_t_ref import ALL, BY_NAME, as_bytes, col_major, pair_and_ref
from tests.mxt_ref import mxt_input

pytestmark = pytest.mark.gpu
forms = pytest.mark.parametrize('form', ALL, ids=repr)

N_MAX = 1024


def _requant(form, q, sf):
    import deepep_amd
    return getattr(deepep_amd, form.public)(q, sf)


def _composition(form, q, sf):
    """The two-launch route of the same build: the transposed cast of the cast back."""
    import deepep_amd
    return getattr(deepep_amd, form.transposed_cast)(getattr(deepep_amd, form.cast_back)(q, sf))


def _prefix(form, N, H, first=0):
    """The pair and the reference of tokens [first, first + N) of the shared input of N_MAX tokens: a prefix of whole
    blocks of tokens has the prefix of the reference (a row's pair and a block's output depend on nothing else)."""
    (q, sf), (q_t, sf_t) = pair_and_ref(form, N_MAX, H)
    want = (q_t[:, form.row_bytes(first):form.row_bytes(first + N)].contiguous(),
            sf_t[:, first // 32:(first + N) // 32].contiguous())
    return (q[first:first + N], sf[first:first + N]), want


def _check(form, got, want, N, H):
    q_t, sf_t = got
    assert q_t.dtype == (torch.uint8 if form.fmt else torch.float8_e4m3fn)
    assert tuple(q_t.shape) == (H, form.row_bytes(N)) and q_t.is_contiguous() and q_t.is_cuda
    assert sf_t.dtype == torch.uint8 and tuple(sf_t.shape) == (H, N // 32) and sf_t.is_contiguous() and sf_t.is_cuda
    assert torch.equal(as_bytes(sf_t), as_bytes(want[1])), 'transposed exponent bytes'
    assert torch.equal(as_bytes(q_t), as_bytes(want[0])), 'transposed codes'


def _hiddens(form, *hs):
    return [h for h in hs if h % form.h_multiple == 0]


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize('N', [128, 384, 640, 1024])     # one tile; a run with a tail; a run + 1; whole runs (16-byte sf_t)
@pytest.mark.parametrize('form,H', [(f, h) for f in ALL for h in _hiddens(f, 128, 512, 640, 1024)],
                         ids=lambda v: repr(v))
def test_shapes_against_the_cpu_reference(form, H, N):
    (q, sf), want = _prefix(form, N, H)
    _check(form, _requant(form, q.cuda(), sf.cuda()), want, N, H)


@functools.lru_cache(maxsize=None)
def _wide_pair(form):
    """The pair of mxt_input(N_MAX, 7168) in this form, cast on the GPU by the package's own casts."""
    import deepep_amd
    x = mxt_input(N_MAX, 7168, N_MAX + 7168).cuda()
    if form.fmt:
        return getattr(deepep_amd, form.fmt.rowwise_cast)(x)
    kw = {'fp32': dict(), 'ue8m0': dict(round_scale=True, use_ue8m0=True),
          'mx': dict(round_scale=True, use_ue8m0=True, group_size=32)}[form.name]
    return deepep_amd.per_token_cast_to_fp8(x, **kw)


@pytest.mark.parametrize('N', [128, 384, 640, 1024])
@forms
def test_the_workloads_row_against_the_two_launch_route(form, N):
    """H = 7168 (56 column blocks): the same build's cast back followed by its transposed cast, both pinned to their
    CPU references by their own tests."""
    q, sf = _wide_pair(form)
    q, sf = q[:N], sf[:N]
    _check(form, _requant(form, q, sf), _composition(form, q, sf), N, 7168)


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('layout', ['padded', 'double'])
@forms
def test_strided_code_rows(form, layout):
    N, H = 384, 1024
    (q, sf), want = _prefix(form, N, H)
    width = q.shape[1] + 64 if layout == 'padded' else 2 * q.shape[1]
    wide = torch.full((N, width), 0x7f, dtype=torch.uint8, device='cuda').view(q.dtype)
    wide[:, :q.shape[1]] = q.cuda()
    rows = wide[:, :q.shape[1]]
    assert rows.stride() == (width, 1)
    _check(form, _requant(form, rows, sf.cuda()), want, N, H)


@forms
def test_column_major_and_strided_factors(form):
    """The column-major tensor of use_tma_aligned_col_major_sf is read in place; so is a view of a wider tensor."""
    N, H = 384, 1024
    (q, sf), want = _prefix(form, N, H)
    cm = col_major(sf.cuda())
    assert cm.stride(0) == 1 and cm.stride(1) >= N
    _check(form, _requant(form, q.cuda(), cm), want, N, H)
    wide = torch.zeros((N, sf.shape[1] + 3), dtype=sf.dtype, device='cuda')
    wide[:, 1:1 + sf.shape[1]] = sf.cuda()
    view = wide[:, 1:1 + sf.shape[1]]
    assert not view.is_contiguous()
    _check(form, _requant(form, q.cuda(), view), want, N, H)


@pytest.mark.parametrize('name', ['mx', 'fp4', 'fp6'])
def test_the_dtype_views(name):
    form = BY_NAME[name]
    N, H = 128, 640
    (q, sf), want = _prefix(form, N, H)
    q, sf = q.cuda(), sf.cuda()
    _check(form, _requant(form, q, sf.view(torch.float8_e8m0fnu)), want, N, H)
    if name == 'fp4':
        _check(form, _requant(form, q.view(torch.float4_e2m1fn_x2), sf), want, N, H)
        _check(form, _requant(form, q.view(torch.float4_e2m1fn_x2), col_major(sf).view(torch.float8_e8m0fnu)), want, N, H)


# ----------------------------------------------------------------------------- every code, every token position
def _finite_codes(form):
    if form.fmt is None:
        return torch.tensor([b for b in range(256) if (b & 0x7f) != 0x7f], dtype=torch.int64)      # 254: no NaN byte
    return torch.arange(1 << form.bits, dtype=torch.int64)                                         # 16 / 64: all finite


def _pack(form, codes):
    """int64 [N, H] codes -> the rows as stored."""
    from tests.fp4_ref import fp4_pack
    from tests.fp6_ref import fp6_pack
    c = codes.to(torch.uint8)
    if form.fmt is None:
        return c.view(torch.float8_e4m3fn)
    return fp4_pack(c) if form.bits == 4 else fp6_pack(c)


@forms
def test_every_finite_code_in_every_token_position(form):
    """One launch.  Row n = 32 m + r holds in column c the code number (m + 8 r + c) mod K of the K finite codes, and
    there are K blocks, so every (token position r, column c) meets every code; the 32 tokens of a block hold codes 8
    apart, so the blocks' amax differ.  Exponent bytes run over 127 +- 20; fp32 factors over 2^-20 .. 2^20 times
    1 + j / 64, so that the cast back's product is no bf16 and its rounding is part of what is compared."""
    table = _finite_codes(form)
    K = table.numel()
    N, H = 32 * ((K + 3) // 4 * 4), form.h_multiple
    assert N % 128 == 0 and N // 32 >= K
    n = torch.arange(N).view(N, 1)
    m, r = n // 32, n % 32
    idx = (m + 8 * r + torch.arange(H).view(1, H)) % K
    for pos in (0, 13, 31):                                  # the construction: every code at a position, per column
        assert torch.equal(idx[pos::32, 5][:K].sort().values, torch.arange(K))
    q = _pack(form, table[idx])
    groups = H // (32 if form.name not in ('fp32', 'ue8m0') else 128)
    e = (3 * m + r + torch.arange(groups).view(1, groups)) % 41 - 20
    if form.name == 'fp32':
        sf = (torch.exp2(e.float()) * (1 + (n % 7).float() / 64)).contiguous()
    elif form.name == 'ue8m0':
        from tests.ue8m0_ref import pack_ref
        sf = pack_ref(torch.exp2(e.float()).contiguous())
    else:
        sf = (e + 127).to(torch.uint8).contiguous()
    back = form.back(q, sf)
    assert torch.isfinite(back.float()).all()
    assert back.float().abs().max() > 2.0 ** 10 and (back.float().abs() < 2.0 ** -10).any()
    want = form.transposed(back)
    _check(form, _requant(form, q.cuda(), sf.cuda()), want, N, H)


# ----------------------------------------------------------------------------- padding rows, neighbours
def _zero_rows(form, q, sf, rows):
    q, sf = q.clone(), sf.clone()
    as_u8 = q.view(torch.uint8)
    as_u8[rows] = 0
    sf[rows] = 0
    return q, sf


@forms
def test_padding_rows_become_zero_rows(form):
    """Zero codes with exponent byte 0 (factor +0.0) -- the padding rows of a casting dispatch -- beside rows with
    tokens in one block (rows 100 .. 127) and as whole blocks (rows 256 .. 383)."""
    N, H = 384, 1024
    (q, sf), _ = _prefix(form, N, H)
    rows = torch.zeros(N, dtype=torch.bool)
    rows[100:128] = True
    rows[256:384] = True
    q, sf = _zero_rows(form, q, sf, rows)
    back = form.back(q, sf)
    assert not back[rows].float().abs().any() and back[~rows].float().abs().any()
    want = form.ref(q, sf)
    got = _requant(form, q.cuda(), sf.cuda())
    _check(form, got, want, N, H)
    codes = form.unpack(as_bytes(got[0]) if form.fmt else got[0])
    assert not (codes[:, rows] & ((1 << (form.bits - 1)) - 1)).any()       # zero magnitudes where the rows are zero
    _check(form, got, _composition(form, q.cuda(), sf.cuda()), N, H)


@forms
def test_a_block_depends_on_its_own_rows_only(form):
    """Tokens 128 .. 255 hold NaN codes (FP8) and 0xff exponent bytes / NaN factors (the uninitialised rows behind a
    worst-case handle's valid ones): the other blocks' bytes are the reference's."""
    N, H = 384, 1024
    (q, sf), want = _prefix(form, N, H)
    q, sf = q.clone(), sf.clone()
    if form.fmt is None:
        junk = torch.tensor([0x7f, 0xff], dtype=torch.uint8)
        q.view(torch.uint8)[128:256] = junk[torch.randint(0, 2, (128, H), generator=torch.Generator().manual_seed(3))]
    if form.name == 'fp32':
        sf[128:256] = float('nan')
    else:
        sf.view(torch.uint8)[128:256] = 0xff
    q_t, sf_t = _requant(form, q.cuda(), sf.cuda())
    q_t, sf_t = as_bytes(q_t), as_bytes(sf_t)
    a, b = form.row_bytes(128), form.row_bytes(256)
    assert torch.equal(q_t[:, :a], want[0][:, :a]) and torch.equal(q_t[:, b:], want[0][:, b:])
    assert torch.equal(sf_t[:, :4], want[1][:, :4]) and torch.equal(sf_t[:, 8:], want[1][:, 8:])


@forms
def test_the_existing_cast_back_is_the_inverse(form):
    import deepep_amd
    N, H = 384, 640 if form.name != 'ue8m0' else 512
    (q, sf), want = _prefix(form, N, H)
    q_t, sf_t = _requant(form, q.cuda(), sf.cuda())
    back = getattr(deepep_amd, form.cast_back)(q_t, sf_t)
    inverse = BY_NAME['mx'] if form.fmt is None else form      # the output of every FP8 form is an MXFP8 pair
    want_q = want[0].view(torch.float8_e4m3fn) if form.fmt is None else want[0]
    ref = inverse.back(want_q, want[1])
    assert tuple(back.shape) == (H, N) and back.dtype == torch.bfloat16
    assert torch.equal(back.cpu().view(torch.int16), ref.view(torch.int16))


# ----------------------------------------------------------------------------- graph capture
@forms
def test_capture_and_no_host_synchronisation(form):
    """One call under torch.cuda.graph, replayed twice over fresh inputs: the bytes follow the inputs; the call itself
    never synchronises the host (sync debug mode 'error')."""
    from deepep_amd.kernels import HipKernels
    HipKernels()                                            # the library is loaded before the watched calls
    N, H = 384, 1024
    cases = [_prefix(form, N, H), _prefix(form, N, H, N_MAX - N)]
    staged = [(q.cuda(), sf.cuda()) for (q, sf), _ in cases]
    q, sf = torch.zeros_like(staged[0][0]), torch.zeros_like(staged[0][1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        eager = _requant(form, *staged[0])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    _check(form, eager, cases[0][1], N, H)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.cuda.set_sync_debug_mode('error')
        try:
            got = _requant(form, q, sf)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    for (sq, ssf), (_, want) in zip(staged, cases):
        q.copy_(sq)
        sf.copy_(ssf)
        graph.replay()
        torch.cuda.synchronize()
        _check(form, got, want, N, H)


# ----------------------------------------------------------------------------- through a dispatch
@pytest.mark.parametrize('name', ['mx', 'fp4', 'fp6'])
def test_the_rows_of_a_casting_dispatch(name):
    """dispatch(cast_to_*=True, do_expand=True, expert_alignment=128, do_zero_padding=True) returns the pair, the row
    count the requantisation needs and experts that start on multiples of 128, so no block of 32 tokens holds rows of
    two experts; the requantised recv_x equals the reference of the received pair."""
    import deepep_amd
    from tests.mx_ref import MX
    from tests.test_cast_keyword_gpu import _group1
    from tests.test_mx_gpu import _mx_inputs
    form = BY_NAME[name]
    T, H, K, E = 64, 256, 2, 4
    buf = deepep_amd.ElasticBuffer(_group1(), num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    x, idx, w = _mx_inputs(11, T, H, K, E)
    flags = MX if name == 'mx' else {form.fmt.dispatch_keyword: True}
    (q, sf), _, _, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True,
                                            expert_alignment=128, do_zero_padding=True, **flags)
    N = q.shape[0]
    assert N % 128 == 0 and N > 0
    ends = [int(v) for v in handle.psum_num_recv_tokens_per_expert.tolist()]
    owner = torch.full((N,), -1, dtype=torch.int64)
    start = 0
    for e, end in enumerate(ends):
        start = (start + 127) // 128 * 128
        assert start <= end <= N
        owner[start:end] = e
        start = end
    assert sum(int((owner == e).any()) for e in range(E)) >= 2, 'several experts must receive rows'
    blocks = owner.view(N // 32, 32)
    for row in blocks.tolist():
        assert len({e for e in row if e >= 0}) <= 1, 'a block of 32 tokens holds rows of two experts'
    valid = owner >= 0
    assert valid.any() and (~valid).any()
    assert not as_bytes(q)[~valid].any() and not as_bytes(sf)[~valid].any()      # padding: zero codes, zero bytes
    got = _requant(form, q, sf)
    _check(form, got, form.ref(q.cpu(), sf.cpu()), N, H)
    _check(form, got, _composition(form, q, sf), N, H)


# ----------------------------------------------------------------------------- no rows
@forms
def test_no_rows_no_launch(form, monkeypatch):
    from deepep_amd.kernels import RequantTransposedKernels
    calls = []
    inner = getattr(RequantTransposedKernels, form.wrapper)
    monkeypatch.setattr(RequantTransposedKernels, form.wrapper,
                        lambda self, *a, **k: (calls.append(a[0].shape), inner(self, *a, **k))[1])
    H = 512
    (q, sf), _ = _prefix(form, 128, H)
    q_t, sf_t = _requant(form, q[:0].cuda(), sf[:0].cuda())
    assert tuple(q_t.shape) == (H, 0) and tuple(sf_t.shape) == (H, 0)
    assert q_t.dtype == (torch.uint8 if form.fmt else torch.float8_e4m3fn) and sf_t.dtype == torch.uint8
    assert q_t.is_cuda and sf_t.is_cuda
    assert not calls
    _requant(form, q.cuda(), sf.cuda())
    assert calls == [q.shape]                               # the spy does see a launch
