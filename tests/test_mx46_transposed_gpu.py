"""cast_to_mxfp4_transposed / cast_to_mxfp6_transposed on the GPU, bit for bit against tests/mxt46_ref (fp4_pair /
fp6_pair of the transposed matrix): the shapes at which the kernel's tiling has tails, strided rows, every token
position of a group, every finite bf16 pattern, the independence of a block from its neighbours' rows, the inverse, a
graph capture, the rows of an expanded dispatch and the empty input.  Every comparison is on bytes.

No new cast back is needed: the result is an ordinary MXFP4 / MXFP6 pair of the transposed matrix, and the existing
per_token_cast_back_fp4 / _fp6 is its inverse (test_the_existing_cast_back_is_the_inverse)."""
import functools

import pytest
import torch

from tests.mxt46_ref import FORMATS, FP4
from tests.mxt_ref import mxt_input

pytestmark = pytest.mark.gpu
fmts = pytest.mark.parametrize('fmt', FORMATS, ids=repr)

N_MAX = 640


@functools.lru_cache(maxsize=None)
def _case(fmt, H):
    """One input per hidden size and its two references, computed once: a prefix of whole blocks of tokens has the
    prefix of the references (a block's bytes depend on its own 32 rows only)."""
    x = mxt_input(N_MAX, H, 1000 + H)
    return x, fmt.transposed_pair(x), fmt.rowwise_pair(x)


def _prefix(fmt, case, N, first=0):
    """The references of tokens [first, first + N) of a _case."""
    _, (qt_all, sft_all), (q_all, sf_all) = case
    want_t = (qt_all[:, fmt.row_bytes(first):fmt.row_bytes(first + N)].contiguous(),
              sft_all[:, first // 32:(first + N) // 32].contiguous())
    return want_t, (q_all[first:first + N], sf_all[first:first + N])


def _bytes(t):
    return t.cpu().view(torch.uint8)


def _cast(fmt, x, **kw):
    import deepep_amd
    return getattr(deepep_amd, fmt.public)(x, **kw)


def _check(fmt, x_gpu, got, want_t, want_row=None):
    """got: what the public function returned for x_gpu; the references on the CPU."""
    N, H = x_gpu.shape
    if want_row is not None:
        (q, sf), (q_t, sf_t) = got
        assert q.dtype == torch.uint8 and tuple(q.shape) == (N, fmt.row_bytes(H)) and q.is_contiguous()
        assert sf.dtype == torch.uint8 and tuple(sf.shape) == (N, H // 32) and sf.is_contiguous()
        assert torch.equal(_bytes(q), want_row[0]), 'row-wise codes'
        assert torch.equal(_bytes(sf), want_row[1]), 'row-wise exponent bytes'
    else:
        q_t, sf_t = got
    assert q_t.dtype == torch.uint8 and tuple(q_t.shape) == (H, fmt.row_bytes(N)) and q_t.is_contiguous()
    assert sf_t.dtype == torch.uint8 and tuple(sf_t.shape) == (H, N // 32) and sf_t.is_contiguous()
    assert torch.equal(_bytes(sf_t), want_t[1]), 'transposed exponent bytes'
    assert torch.equal(_bytes(q_t), want_t[0]), 'transposed codes'


@pytest.mark.parametrize('with_rowwise', [False, True])
@pytest.mark.parametrize('H', [128, 640, 7168])          # one tile; tiles; the workload's row (56 column blocks)
@pytest.mark.parametrize('N', [128, 384, 640])           # one tile; a run with a tail (dword scale factors); a run + 1
@fmts
def test_shapes(fmt, N, H, with_rowwise):
    import deepep_amd
    case = _case(fmt, H)
    if (N, H) == (N_MAX, 640):
        fmt.self_check(case[0])
    x = case[0][:N].cuda()
    want_t, want_row = _prefix(fmt, case, N)
    got = _cast(fmt, x, with_rowwise=with_rowwise)
    _check(fmt, x, got, want_t, want_row if with_rowwise else None)
    if with_rowwise:
        q, sf = getattr(deepep_amd, fmt.rowwise_cast)(x)
        assert torch.equal(_bytes(got[0][0]), _bytes(q)) and torch.equal(_bytes(got[0][1]), _bytes(sf))


@fmts
def test_runs_of_four_tiles_store_vectors_of_scale_factors(fmt):
    """N % 512 == 0: a column's 16 exponent bytes of a run leave as one 16-byte store (N = 1024: two runs)."""
    x_cpu = mxt_input(1024, 256, 7)
    x = x_cpu.cuda()
    want_t, want_row = fmt.transposed_pair(x_cpu), fmt.rowwise_pair(x_cpu)
    _check(fmt, x, _cast(fmt, x, with_rowwise=True), want_t, want_row)
    _check(fmt, x, _cast(fmt, x), want_t)


@pytest.mark.parametrize('with_rowwise', [False, True])
def test_two_tiles_share_a_line_of_fp4_codes(with_rowwise):
    """N = 256: a column's 128 bytes of q_t are one 128-byte line, half from each of the run's two tiles."""
    x_cpu = mxt_input(256, 384, 8)
    x = x_cpu.cuda()
    _check(FP4, x, _cast(FP4, x, with_rowwise=with_rowwise), FP4.transposed_pair(x_cpu),
           FP4.rowwise_pair(x_cpu) if with_rowwise else None)


@pytest.mark.parametrize('with_rowwise', [False, True])
@pytest.mark.parametrize('layout', ['padded', 'double'])
@fmts
def test_strided_rows(fmt, layout, with_rowwise):
    N, H = 384, 640
    case = _case(fmt, H)
    width = H + 64 if layout == 'padded' else 2 * H
    wide = torch.full((N, width), float('nan'), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = case[0][:N].cuda()
    x = wide[:, :H]
    assert x.stride() == (width, 1)
    want_t, want_row = _prefix(fmt, case, N)
    _check(fmt, x, _cast(fmt, x, with_rowwise=with_rowwise), want_t, want_row if with_rowwise else None)


@fmts
def test_every_token_position_reaches_its_own_place(fmt):
    """One launch, 1024 x 128: x[n, c] is non-zero only where n % 32 == (c + n / 32) % 32, so every (column, block)
    holds exactly one token, every token position r of a block is met by four columns of every block, and the
    non-zero code must stand in column c's row at nibble / 6-bit field r and nowhere else.  The values differ from
    one position to the next (magnitudes 1, 1.5, 2, 3 times a power of two per block, the sign from the position), so
    a swapped pair of tokens, a rotated field or a crossed column shows in the codes or in the exponent bytes."""
    N, H = 1024, 128
    n = torch.arange(N).view(N, 1)
    c = torch.arange(H).view(1, H)
    r = n % 32
    where = r == (c + n // 32) % 32
    mant = torch.tensor([1.0, 1.5, 2.0, 3.0])[(r % 4).expand(N, H)]
    value = mant * torch.exp2(((n // 32) % 5 - 2).float()) * torch.where((r // 4) % 2 == 0, 1.0, -1.0)
    x_cpu = torch.where(where, value, torch.zeros(())).to(torch.bfloat16)
    want_t = fmt.transposed_pair(x_cpu)
    # the reference itself: one non-zero code per (column, block), at the token the construction names
    codes = fmt.unpack(want_t[0]).view(H, N // 32, 32)
    hit = (codes & ((1 << (fmt.bits - 1)) - 1)) != 0
    assert torch.equal(hit.sum(dim=2), torch.ones((H, N // 32), dtype=torch.int64))
    assert torch.equal(hit, where.t().contiguous().view(H, N // 32, 32))
    x = x_cpu.cuda()
    _check(fmt, x, _cast(fmt, x, with_rowwise=True), want_t, fmt.rowwise_pair(x_cpu))
    _check(fmt, x, _cast(fmt, x), want_t)


@pytest.mark.parametrize('seed', [0, 1])
@fmts
def test_every_finite_bf16_pattern(fmt, seed):
    """The 65280 finite patterns (and 256 zeros) in a random order over 512 x 128: the 32 tokens of a block, and the
    32 columns of a row-wise group, are random patterns, so a pattern meets the scale of its block's amax here and of
    another block's under the second permutation; both halves against the CPU reference."""
    bits = torch.arange(65536, dtype=torch.int32)
    finite = bits[(bits & 0x7f80) != 0x7f80]
    assert finite.numel() == 65280
    padded = torch.zeros(512 * 128, dtype=torch.int32)
    padded[:65280] = finite
    perm = torch.randperm(512 * 128, generator=torch.Generator().manual_seed(seed))
    x_cpu = padded[perm].to(torch.int16).view(torch.bfloat16).view(512, 128)
    x = x_cpu.cuda()
    _check(fmt, x, _cast(fmt, x, with_rowwise=True), fmt.transposed_pair(x_cpu), fmt.rowwise_pair(x_cpu))
    # the same patterns sorted by magnitude, so that a pattern also meets the scale of its own binade: along the token
    # axis (a block's 32 tokens are neighbours in that order; the row-wise groups stay mixed), or along the columns
    # (the row-wise groups are neighbours; the blocks stay mixed)
    ordered = padded[(padded & 0x7fff).argsort(stable=True)].to(torch.int16).view(torch.bfloat16)
    y_cpu = ordered.view(128, 512).t().contiguous() if seed == 0 else ordered.view(512, 128)
    y = y_cpu.cuda()
    _check(fmt, y, _cast(fmt, y, with_rowwise=True), fmt.transposed_pair(y_cpu), fmt.rowwise_pair(y_cpu))


@fmts
def test_a_block_depends_on_its_own_rows_only(fmt):
    """Tokens 128 .. 255 hold NaN, +Inf and -Inf (the uninitialised rows behind a worst-case handle's valid ones): the
    bytes of the other tokens are those the kernel gives for the clean input, which are the reference's."""
    N, H = 384, 640
    case = _case(fmt, H)
    clean = case[0][:N]
    x_cpu = clean.clone()
    junk = torch.tensor([float('nan'), float('inf'), float('-inf')], dtype=torch.bfloat16)
    x_cpu[128:256] = junk[torch.randint(0, 3, (128, H), generator=torch.Generator().manual_seed(3))]
    (cq, csf), (cq_t, csf_t) = [[_bytes(t) for t in pair] for pair in _cast(fmt, clean.cuda(), with_rowwise=True)]
    want_t, want_row = _prefix(fmt, case, N)
    assert torch.equal(cq_t, want_t[0]) and torch.equal(csf_t, want_t[1])
    assert torch.equal(cq, want_row[0]) and torch.equal(csf, want_row[1])
    (q, sf), (q_t, sf_t) = _cast(fmt, x_cpu.cuda(), with_rowwise=True)
    q_t2, sf_t2 = _cast(fmt, x_cpu.cuda())
    a, b = fmt.row_bytes(128), fmt.row_bytes(256)
    for qt, sft in ((q_t, sf_t), (q_t2, sf_t2)):
        qt, sft = _bytes(qt), _bytes(sft)
        assert torch.equal(qt[:, :a], cq_t[:, :a]) and torch.equal(qt[:, b:], cq_t[:, b:])
        assert torch.equal(sft[:, :4], csf_t[:, :4]) and torch.equal(sft[:, 8:], csf_t[:, 8:])
    q, sf = _bytes(q), _bytes(sf)
    assert torch.equal(q[:128], cq[:128]) and torch.equal(q[256:], cq[256:])
    assert torch.equal(sf[:128], csf[:128]) and torch.equal(sf[256:], csf[256:])


@fmts
def test_the_existing_cast_back_is_the_inverse(fmt):
    """per_token_cast_back_fp4 / _fp6 takes the transposed pair as it stands: it is an ordinary pair of x^T."""
    import deepep_amd
    case = _case(fmt, 640)
    x = case[0][:384].cuda()
    q_t, sf_t = _cast(fmt, x)
    back = getattr(deepep_amd, fmt.cast_back)(q_t, sf_t)
    want_t, _ = _prefix(fmt, case, 384)
    ref = fmt.back_ref(*want_t)
    assert tuple(back.shape) == (640, 384) and back.dtype == torch.bfloat16
    assert torch.equal(back.cpu().view(torch.int16), ref.view(torch.int16))
    back_e8 = getattr(deepep_amd, fmt.cast_back)(q_t, sf_t.view(torch.float8_e8m0fnu))
    assert torch.equal(back_e8.view(torch.int16), back.view(torch.int16))


@pytest.mark.parametrize('with_rowwise', [False, True])
@fmts
def test_capture_and_no_host_synchronisation(fmt, with_rowwise):
    """One call under torch.cuda.graph (one stream, no branches), replayed twice over a changed input: the bytes
    follow the input; the call itself never synchronises the host (sync debug mode 'error')."""
    from deepep_amd.kernels import HipKernels
    HipKernels()                                            # the library is loaded before the watched calls
    N, H = 384, 640
    case = _case(fmt, H)
    refs = [_prefix(fmt, case, N), _prefix(fmt, case, N, N_MAX - N)]
    x = torch.zeros((N, H), dtype=torch.bfloat16, device='cuda')
    staged = [case[0][:N].cuda(), case[0][N_MAX - N:].cuda()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        eager = _cast(fmt, staged[0], with_rowwise=with_rowwise)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    _check(fmt, staged[0], eager, refs[0][0], refs[0][1] if with_rowwise else None)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.cuda.set_sync_debug_mode('error')
        try:
            got = _cast(fmt, x, with_rowwise=with_rowwise)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    for src, (want_t, want_row) in zip(staged, refs):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _check(fmt, x, got, want_t, want_row if with_rowwise else None)


@fmts
def test_the_expanded_rows_of_a_dispatch(fmt):
    """dispatch(do_expand=True, expert_alignment=128, do_zero_padding=True) gives the row count the cast needs and
    experts that start on multiples of 128, so no group of 32 tokens holds rows of two experts; both pairs of the
    received rows equal the references, and the row-wise half is what the casting dispatch returns on the same handle
    -- on the rows that hold tokens; on padding rows the codes only (the dispatch leaves its padding rows' scale
    factors zero, the cast gives a zero row the exponent byte of 1e-4; the codes of padding rows are zero in both)."""
    import deepep_amd
    from tests.test_cast_keyword_gpu import _group1
    from tests.test_mx_gpu import _mx_inputs
    T, H, K, E = 64, 256, 2, 4
    buf = deepep_amd.ElasticBuffer(_group1(), num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    x, idx, w = _mx_inputs(11, T, H, K, E)
    kw = dict(do_expand=True, expert_alignment=128, do_zero_padding=True)
    recv_x, _, _, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, **kw)
    N = recv_x.shape[0]
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
    (q, sf), (q_t, sf_t) = _cast(fmt, recv_x, with_rowwise=True)
    _check(fmt, recv_x, ((q, sf), (q_t, sf_t)), fmt.transposed_pair(recv_x.cpu()), fmt.rowwise_pair(recv_x.cpu()))
    (dq, dsf), _, _, _, _ = buf.dispatch(x, handle=handle, **{fmt.dispatch_keyword: True}, **kw)
    valid = owner >= 0
    assert valid.any() and (~valid).any()
    assert torch.equal(_bytes(q), _bytes(dq))
    assert torch.equal(_bytes(sf)[valid], _bytes(dsf)[valid])
    assert not _bytes(q)[~valid].any()


@fmts
def test_no_rows_no_launch(fmt, monkeypatch):
    from deepep_amd.kernels import TransposedFp4Fp6Kernels
    calls = []
    inner = getattr(TransposedFp4Fp6Kernels, fmt.wrapper)
    monkeypatch.setattr(TransposedFp4Fp6Kernels, fmt.wrapper,
                        lambda self, *a, **k: (calls.append(a[0].shape), inner(self, *a, **k))[1])
    x = torch.empty((0, 256), dtype=torch.bfloat16, device='cuda')
    q_t, sf_t = _cast(fmt, x)
    assert tuple(q_t.shape) == (256, 0) and tuple(sf_t.shape) == (256, 0)
    (q, sf), (q_t, sf_t) = _cast(fmt, x, with_rowwise=True)
    assert tuple(q.shape) == (0, fmt.row_bytes(256)) and tuple(sf.shape) == (0, 8)
    assert q.dtype == q_t.dtype == sf.dtype == sf_t.dtype == torch.uint8
    assert q.is_cuda and q_t.is_cuda and sf.is_cuda and sf_t.is_cuda
    assert not calls
    _cast(fmt, torch.zeros((128, 128), dtype=torch.bfloat16, device='cuda'))
    assert calls == [torch.Size((128, 128))]               # the spy does see a launch
