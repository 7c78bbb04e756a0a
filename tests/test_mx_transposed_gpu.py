"""cast_to_mxfp8_transposed on the GPU, bit for bit against tests/mxt_ref (mx_pair of the transposed matrix): the shapes
at which the kernel's tiling has tails, strided rows, every token position of a group, every finite bf16 pattern, the
independence of a block from its neighbours' rows, the inverse, a graph capture, the rows of an expanded dispatch and
the empty input.  Every comparison is on bytes.

No new cast back is needed: the result is an ordinary MXFP8 pair of the transposed matrix, and the existing
per_token_cast_back is its inverse (test_the_existing_cast_back_is_the_inverse)."""
import functools

import pytest
import torch

from tests.mx_ref import MX, mx_back_ref
from tests.mxt_ref import mxt_input, mxt_pair, rowwise_pair, self_check

pytestmark = pytest.mark.gpu

MXKW = dict(round_scale=True, use_ue8m0=True, group_size=32)
N_MAX = 640


@functools.lru_cache(maxsize=None)
def _case(H):
    """One input per hidden size and its two references, computed once: a prefix of whole blocks of tokens has the
    prefix of the references (a block's bytes depend on its own 32 rows only)."""
    x = mxt_input(N_MAX, H, 1000 + H)
    return x, mxt_pair(x), rowwise_pair(x)


def _bytes(t):
    return t.cpu().view(torch.uint8)


def _check(x_gpu, got, want_t, want_row=None):
    """got: what cast_to_mxfp8_transposed returned for x_gpu; the references on the CPU."""
    if want_row is not None:
        (q, sf), (q_t, sf_t) = got
        N, H = x_gpu.shape
        assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (N, H) and q.is_contiguous()
        assert sf.dtype == torch.uint8 and tuple(sf.shape) == (N, H // 32) and sf.is_contiguous()
        assert torch.equal(_bytes(q), want_row[0]), 'row-wise e4m3fn bytes'
        assert torch.equal(_bytes(sf), want_row[1]), 'row-wise exponent bytes'
    else:
        q_t, sf_t = got
    N, H = x_gpu.shape
    assert q_t.dtype == torch.float8_e4m3fn and tuple(q_t.shape) == (H, N) and q_t.is_contiguous()
    assert sf_t.dtype == torch.uint8 and tuple(sf_t.shape) == (H, N // 32) and sf_t.is_contiguous()
    assert torch.equal(_bytes(q_t), want_t[0]), 'transposed e4m3fn bytes'
    assert torch.equal(_bytes(sf_t), want_t[1]), 'transposed exponent bytes'


@pytest.mark.parametrize('with_rowwise', [False, True])
@pytest.mark.parametrize('H', [128, 640, 7168])          # one tile; tiles; the workload's row (56 column blocks)
@pytest.mark.parametrize('N', [128, 384, 640])           # one tile; a run with a tail (dword scale factors); a run + 1
def test_shapes(N, H, with_rowwise):
    import deepep_amd
    x_all, (qt_all, sft_all), (q_all, sf_all) = _case(H)
    if (N, H) == (N_MAX, 640):
        self_check(x_all)
    x = x_all[:N].cuda()
    want_t = (qt_all[:, :N].contiguous(), sft_all[:, :N // 32].contiguous())
    want_row = (q_all[:N], sf_all[:N]) if with_rowwise else None
    got = deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=with_rowwise)
    _check(x, got, want_t, want_row)
    if with_rowwise:
        q, sf = deepep_amd.per_token_cast_to_fp8(x, **MXKW)
        assert torch.equal(_bytes(got[0][0]), _bytes(q)) and torch.equal(_bytes(got[0][1]), _bytes(sf))


def test_runs_of_four_tiles_store_vectors_of_scale_factors():
    """N % 512 == 0: a column's 16 exponent bytes of a run leave as one 16-byte store (N = 1024: two runs)."""
    import deepep_amd
    x_cpu = mxt_input(1024, 256, 7)
    x = x_cpu.cuda()
    _check(x, deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True), mxt_pair(x_cpu), rowwise_pair(x_cpu))
    _check(x, deepep_amd.cast_to_mxfp8_transposed(x), mxt_pair(x_cpu))


@pytest.mark.parametrize('with_rowwise', [False, True])
@pytest.mark.parametrize('layout', ['padded', 'double'])
def test_strided_rows(layout, with_rowwise):
    import deepep_amd
    N, H = 384, 640
    x_all, (qt_all, sft_all), (q_all, sf_all) = _case(H)
    width = H + 64 if layout == 'padded' else 2 * H
    wide = torch.full((N, width), float('nan'), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x_all[:N].cuda()
    x = wide[:, :H]
    assert x.stride() == (width, 1)
    want_t = (qt_all[:, :N].contiguous(), sft_all[:, :N // 32].contiguous())
    want_row = (q_all[:N], sf_all[:N]) if with_rowwise else None
    _check(x, deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=with_rowwise), want_t, want_row)


def test_every_token_position_reaches_its_own_column():
    """128 cases of 128 x 128 in one launch: 2^-8 everywhere but one 3.0 at token r, column 37 r mod 128.  Every row
    index of every group must raise its column's exponent byte, and no other column's."""
    import deepep_amd
    x_cpu = torch.full((128 * 128, 128), 2.0 ** -8, dtype=torch.bfloat16)
    r = torch.arange(128)
    x_cpu[128 * r + r, (37 * r) % 128] = 3.0
    q_t_ref, sf_t_ref = mxt_pair(x_cpu)
    # the reference itself: exactly one raised byte per case, at (column, group of r)
    low, high = int(sf_t_ref[1, 0]), int(sf_t_ref[0, 0])
    assert high > low
    want = torch.full((128, 128 * 4), low, dtype=torch.uint8)
    want[(37 * r) % 128, 4 * r + r // 32] = high
    assert torch.equal(sf_t_ref, want)
    x = x_cpu.cuda()
    _check(x, deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True), (q_t_ref, sf_t_ref), rowwise_pair(x_cpu))


@pytest.mark.parametrize('seed', [0, 1])
def test_every_finite_bf16_pattern(seed):
    import deepep_amd
    bits = torch.arange(65536, dtype=torch.int32)
    finite = bits[(bits & 0x7f80) != 0x7f80]
    assert finite.numel() == 65280
    padded = torch.zeros(512 * 128, dtype=torch.int32)
    padded[:65280] = finite
    perm = torch.randperm(512 * 128, generator=torch.Generator().manual_seed(seed))
    x_cpu = padded[perm].to(torch.int16).view(torch.bfloat16).view(512, 128)
    x = x_cpu.cuda()
    _check(x, deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True), mxt_pair(x_cpu), rowwise_pair(x_cpu))


def test_a_block_depends_on_its_own_rows_only():
    """Tokens 128 .. 255 hold NaN, +Inf and -Inf (the uninitialised rows behind a worst-case handle's valid ones): the
    bytes of the other tokens are those of the clean input."""
    import deepep_amd
    N, H = 384, 640
    x_all, (qt_all, sft_all), (q_all, sf_all) = _case(H)
    x_cpu = x_all[:N].clone()
    junk = torch.tensor([float('nan'), float('inf'), float('-inf')], dtype=torch.bfloat16)
    x_cpu[128:256] = junk[torch.randint(0, 3, (128, H), generator=torch.Generator().manual_seed(3))]
    (q, sf), (q_t, sf_t) = deepep_amd.cast_to_mxfp8_transposed(x_cpu.cuda(), with_rowwise=True)
    q_t2, sf_t2 = deepep_amd.cast_to_mxfp8_transposed(x_cpu.cuda())
    for qt, sft in ((q_t, sf_t), (q_t2, sf_t2)):
        qt, sft = _bytes(qt), _bytes(sft)
        assert torch.equal(qt[:, :128], qt_all[:, :128]) and torch.equal(qt[:, 256:], qt_all[:, 256:N])
        assert torch.equal(sft[:, :4], sft_all[:, :4]) and torch.equal(sft[:, 8:], sft_all[:, 8:N // 32])
    q, sf = _bytes(q), _bytes(sf)
    assert torch.equal(q[:128], q_all[:128]) and torch.equal(q[256:], q_all[256:N])
    assert torch.equal(sf[:128], sf_all[:128]) and torch.equal(sf[256:], sf_all[256:N])


def test_the_existing_cast_back_is_the_inverse():
    """per_token_cast_back takes the transposed pair as it stands: it is an MXFP8 pair of x^T.  No new cast back."""
    import deepep_amd
    x_all, _, _ = _case(640)
    x = x_all[:384].cuda()
    q_t, sf_t = deepep_amd.cast_to_mxfp8_transposed(x)
    back = deepep_amd.per_token_cast_back(q_t, sf_t)
    ref = mx_back_ref(q_t, sf_t)
    assert tuple(back.shape) == (640, 384)
    assert torch.equal(back.cpu().view(torch.int16), ref.view(torch.int16))
    back_e8 = deepep_amd.per_token_cast_back(q_t, sf_t.view(torch.float8_e8m0fnu))
    assert torch.equal(back_e8.view(torch.int16), back.view(torch.int16))
    # and it is close to x^T (calc_diff of the round trip: 3.5e-4 on such inputs)
    a, b = back.float().cpu().double(), x_all[:384].t().double()
    assert 1 - 2 * (a * b).sum() / ((a * a).sum() + (b * b).sum()) < 1e-3


@pytest.mark.parametrize('with_rowwise', [False, True])
def test_capture_and_no_host_synchronisation(with_rowwise):
    """One call under torch.cuda.graph (one stream, no branches), replayed twice over a changed input: the bytes
    follow the input; the call itself never synchronises the host (sync debug mode 'error')."""
    import deepep_amd
    from deepep_amd.kernels import HipKernels
    HipKernels()                                            # the library is loaded before the watched calls
    N, H = 384, 640
    x_all, (qt_all, sft_all), (q_all, sf_all) = _case(H)
    first, second = x_all[:N], x_all[N_MAX - N:]
    refs = [((qt_all[:, :N].contiguous(), sft_all[:, :N // 32].contiguous()), (q_all[:N], sf_all[:N])),
            ((qt_all[:, N_MAX - N:].contiguous(), sft_all[:, (N_MAX - N) // 32:].contiguous()),
             (q_all[N_MAX - N:], sf_all[N_MAX - N:]))]
    x = torch.zeros((N, H), dtype=torch.bfloat16, device='cuda')
    staged = [first.cuda(), second.cuda()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        eager = deepep_amd.cast_to_mxfp8_transposed(staged[0], with_rowwise=with_rowwise)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    _check(staged[0], eager, refs[0][0], refs[0][1] if with_rowwise else None)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.cuda.set_sync_debug_mode('error')
        try:
            got = deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=with_rowwise)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    for src, (want_t, want_row) in zip(staged, refs):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _check(x, got, want_t, want_row if with_rowwise else None)


def test_the_expanded_rows_of_a_dispatch():
    """dispatch(do_expand=True, expert_alignment=128, do_zero_padding=True) gives the row count the cast needs and
    experts that start on multiples of 128, so no group of 32 tokens holds rows of two experts; both pairs of the
    received rows equal the references, and the row-wise half is what the MXFP8 casting dispatch returns on the same
    handle (on the rows that hold tokens: the dispatch leaves its padding rows' scale factors zero, the cast gives a
    zero row the exponent byte of 1e-4; the e4m3fn bytes of padding rows are zero in both)."""
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
    groups = owner.view(N // 32, 32)
    for g in groups:
        assert len(set(g[g >= 0].tolist())) <= 1, 'a group of 32 tokens holds rows of two experts'
    (q, sf), (q_t, sf_t) = deepep_amd.cast_to_mxfp8_transposed(recv_x, with_rowwise=True)
    _check(recv_x, ((q, sf), (q_t, sf_t)), mxt_pair(recv_x.cpu()), rowwise_pair(recv_x.cpu()))
    (dq, dsf), _, _, _, _ = buf.dispatch(x, handle=handle, **MX, **kw)
    valid = owner >= 0
    assert torch.equal(_bytes(q), _bytes(dq))
    assert torch.equal(_bytes(sf)[valid], _bytes(dsf)[valid])
    assert not _bytes(q)[~valid].any()


def test_no_rows_no_launch(monkeypatch):
    import deepep_amd
    from deepep_amd.kernels import TransposedCastKernels
    calls = []
    inner = TransposedCastKernels.cast_fp8_mx_transposed
    monkeypatch.setattr(TransposedCastKernels, 'cast_fp8_mx_transposed',
                        lambda self, *a, **k: (calls.append(a[0].shape), inner(self, *a, **k))[1])
    x = torch.empty((0, 256), dtype=torch.bfloat16, device='cuda')
    q_t, sf_t = deepep_amd.cast_to_mxfp8_transposed(x)
    assert tuple(q_t.shape) == (256, 0) and tuple(sf_t.shape) == (256, 0)
    (q, sf), (q_t, sf_t) = deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True)
    assert tuple(q.shape) == (0, 256) and tuple(sf.shape) == (0, 8)
    assert q.dtype == q_t.dtype == torch.float8_e4m3fn and sf.dtype == sf_t.dtype == torch.uint8
    assert not calls
    deepep_amd.cast_to_mxfp8_transposed(torch.zeros((128, 128), dtype=torch.bfloat16, device='cuda'))
    assert calls == [torch.Size((128, 128))]               # the spy does see a launch
