"""route_topk on the GPU against its definition in fp64 on the CPU (`_gate`: a stable descending sort gives the tie
rule).  Float32 logits are randn * 1.5, the bias randn * 0.1, fixed seeds; bfloat16 rows (E <= 256) are permutations of
(i - E / 2) / 32, exact and distinct in bf16.

Selection: per row the chosen set equals the reference's, and the fp64 sel in the kernel's order does not increase.  A
row whose deciding gap (last kept group against first dropped, K-th expert against (K+1)-th) is below 2^-16 of the
larger value is left out of the set comparison -- fp32 scoring cannot resolve it -- and at most 5 % of a case's rows
may be.  With the reference alone on the CPU, 4096 rows a shape, both score functions, with and without a bias, the
largest share of such rows over the six shapes was 0.83 % (E = 1024, sigmoid, no bias).

Weights, at the kernel's own indices: |w - ref| <= c 2^-23 |ref|, c = max(8, 4 x the largest error of the eager
fp32 formula against fp64 on the same inputs, in units of 2^-23 |ref|).  On an MI355X the eager error was 0.29 to
5.54 units over the cases, so c = 8 to 22.1, and the kernel's largest error over the bound 0.234.

EP_NUM_TOPK_IDX_BITS=32 fixes deep_ep.topk_idx_t at import, and tests/idx_bits_child.py runs a closed list of cases:
int32 indices are checked here through the kernels.RouterKernels wrapper, which takes either width."""
import pytest
import torch

pytestmark = pytest.mark.gpu
MARGIN, ULP = 2.0 ** -16, 2.0 ** -23
SCALE = 2.5
# T, E, K, groups, kept groups, group score
CASES = [(1, 8, 2, 1, 1, 'top2_sum'), (5, 64, 6, 1, 1, 'top2_sum'), (67, 256, 8, 8, 4, 'top2_sum'),
         (67, 384, 8, 1, 1, 'top2_sum'), (33, 1024, 64, 64, 8, 'top2_sum'), (4, 160, 6, 8, 3, 'max')]
RUNS = [(c, dtype, f, b) for c in CASES for dtype in (torch.float32, torch.bfloat16) for f in ('sigmoid', 'softmax')
        for b in (False, True) if dtype == torch.float32 or c[1] <= 256]


def _inputs(T, E, dtype, with_bias, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        x = torch.randn((T, E), generator=g) * 1.5
    else:
        x = torch.stack([(torch.randperm(E, generator=g) - E // 2) / 32 for _ in range(T)]).to(dtype)
    return x, (torch.randn((E,), generator=g) * 0.1 if with_bias else None)


def _scores(x, score_func):
    return torch.sigmoid(x) if score_func == 'sigmoid' else torch.softmax(x, dim=-1)


def _gap(hi, lo):
    """Is hi above lo by the margin?  (lo = -inf: nothing competes.)"""
    return hi - lo >= MARGIN * torch.maximum(hi.abs(), lo.abs().clamp(max=1e300))


def _gate(x, K, score_func, bias, G, kept, group_score):
    """The definition in fp64 -> (s, sel, the chosen indices, which rows are decided by more than the margin)."""
    s = _scores(x.double(), score_func)
    sel = s if bias is None else s + bias.double()
    T, E = sel.shape
    decided, open_sel = torch.ones(T, dtype=torch.bool), sel
    if G > 1:
        by_group = sel.view(T, G, E // G)
        score = by_group.topk(2, dim=-1).values.sum(-1) if group_score == 'top2_sum' else by_group.amax(-1)
        ranked = torch.sort(score, dim=-1, descending=True, stable=True)
        keep = torch.zeros((T, G), dtype=torch.bool).scatter_(1, ranked.indices[:, :kept], True)
        open_sel = sel.masked_fill(~keep.repeat_interleave(E // G, dim=1), float('-inf'))
        if kept < G:
            decided &= _gap(ranked.values[:, kept - 1], ranked.values[:, kept])
    ranked = torch.sort(open_sel, dim=-1, descending=True, stable=True)
    if K < E:
        decided &= _gap(ranked.values[:, K - 1], ranked.values[:, K])
    return s, sel, ranked.indices[:, :K], decided


def _weights(s, idx, norm=True, scale=SCALE):
    w = s.gather(1, idx)
    return (w / w.sum(-1, keepdim=True) if norm else w) * scale


def _units(w, ref):
    return float(((w.double() - ref).abs() / (ULP * ref.abs())).nan_to_num(nan=0.0).max())     # 0 against 0: no error


def _check(case, x, bias, score_func):
    import deep_ep
    T, E, K, G, kept, group_score = case
    kw = dict(score_func=score_func, num_groups=G, num_topk_groups=kept, group_score=group_score)
    idx, w = deep_ep.route_topk(x.cuda(), K, bias=None if bias is None else bias.cuda(), routed_scaling_factor=SCALE, **kw)
    assert idx.dtype == deep_ep.topk_idx_t and w.dtype == torch.float32 and idx.is_contiguous() and w.is_contiguous()
    assert tuple(idx.shape) == tuple(w.shape) == (T, K)
    idx, w = idx.cpu().long(), w.cpu()
    s, sel, ref_idx, decided = _gate(x, K, score_func, bias, G, kept, group_score)
    # selection: in range, no repeats, the reference's set, descending
    ordered = idx.sort(-1).values
    assert int(idx.min()) >= 0 and int(idx.max()) < E and bool((ordered[:, 1:] != ordered[:, :-1]).all())
    left_out = 1 - decided.double().mean()
    print('rows left out:', float(left_out))
    assert left_out <= 0.05
    assert torch.equal(ordered[decided], ref_idx.sort(-1).values[decided])
    mine = sel.gather(1, idx)
    assert bool((mine[:, 1:] <= mine[:, :-1] + MARGIN * mine[:, :-1].abs()).all())
    # weights at the kernel's own indices
    ref = _weights(s, idx)
    eager = _units(_weights(_scores(x.float(), score_func), idx), ref)
    c = max(8.0, 4 * eager)
    print(f'eager error {eager:.2f}, c {c:.2f}, kernel error over the bound {_units(w, ref) / c:.3f}')
    assert bool(((w.double() - ref).abs() <= c * ULP * ref.abs()).all())
    assert bool(((w.double().sum(-1) - SCALE).abs() <= K * c * ULP * SCALE).all())


@pytest.mark.parametrize('case,dtype,score_func,with_bias', RUNS)
def test_selection_and_weights(case, dtype, score_func, with_bias):
    _check(case, *_inputs(case[0], case[1], dtype, with_bias, seed=case[1] + case[2]), score_func)


@pytest.mark.parametrize('score_func', ['sigmoid', 'softmax'])
def test_infinite_and_huge_logits(score_func):
    """-inf (an expert masked out) and -3e38 score exactly 0 -- the bias may still choose them, with the weight 0 --
    and under the sigmoid +inf and 3e38 score exactly 1.  No weight is NaN (a NaN fails the bound)."""
    x, bias = _inputs(CASES[2][0], CASES[2][1], torch.float32, True, seed=3)
    x[:, 3::16], x[:, 7] = float('-inf'), -3e38
    if score_func == 'sigmoid':
        x[:, 40], x[:, 90] = float('inf'), 3e38
    _check(CASES[2], x, bias, score_func)


@pytest.mark.parametrize('score_func', ['sigmoid', 'softmax'])
def test_strided_rows_and_plain_weights(score_func):
    """Rows 16 bytes further apart than E floats, and w = s * 1 without the normalisation."""
    import deep_ep
    T, E, K, G, kept, group_score = CASES[2]
    wide = _inputs(T, E + 4, torch.float32, False, seed=5)[0]
    x, x_gpu = wide[:, :E], wide.cuda()[:, :E]
    assert not x_gpu.is_contiguous()
    idx, w = deep_ep.route_topk(x_gpu, K, score_func=score_func, num_groups=G, num_topk_groups=kept, norm_topk_prob=False)
    s, _, ref_idx, decided = _gate(x, K, score_func, None, G, kept, group_score)
    assert bool(decided.all()) and torch.equal(idx.cpu().long(), ref_idx)
    ref = _weights(s, ref_idx, norm=False, scale=1.0)
    c = max(8.0, 4 * _units(_weights(_scores(x.float(), score_func), ref_idx, norm=False, scale=1.0), ref))
    assert bool(((w.cpu().double() - ref).abs() <= c * ULP * ref.abs()).all())


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('score_func', ['sigmoid', 'softmax'])
@pytest.mark.parametrize('bias_value', [None, 0.25])
def test_ties_go_to_the_lower_index(case, score_func, bias_value):
    import deep_ep
    T, E, K, G, kept, group_score = case
    x = torch.full((T, E), 0.75, device='cuda')
    bias = None if bias_value is None else torch.full((E,), bias_value, device='cuda')
    idx, w = deep_ep.route_topk(x, K, score_func=score_func, bias=bias, num_groups=G, num_topk_groups=kept,
                                group_score=group_score)
    assert torch.equal(idx.cpu().long(), torch.arange(K).expand(T, K))   # the first K experts of the first `kept` groups
    assert bool((w == w[0, 0]).all()) and abs(float(w[0, 0]) * K - 1) <= K * 8 * ULP


@pytest.mark.parametrize('case', [CASES[0], CASES[2]])
def test_counts_and_no_stray_stores(case):
    """counts against torch.bincount of the returned indices (T = 1 and T = 67), and the wrapper writing into views of
    sentinel-filled buffers: int64 and int32 indices, the same values, nothing outside the views."""
    import deep_ep
    from deepep_amd import kernels
    T, E, K, G, kept, group_score = case
    x, bias = _inputs(T, E, torch.float32, True, seed=11)
    x, bias = x.cuda(), bias.cuda()
    kw = dict(bias=bias, num_groups=G, num_topk_groups=kept, group_score=group_score)
    idx, w, counts = deep_ep.route_topk(x, K, return_counts=True, **kw)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (E,)
    assert torch.equal(counts.long(), torch.bincount(idx.flatten().long(), minlength=E))
    for dtype in (torch.int64, torch.int32):
        new = lambda rows, cols, size: torch.full((rows, cols * size), 0xa5, dtype=torch.uint8, device='cuda')
        raw = dict(idx=new(T + 2, K, dtype.itemsize), w=new(T + 2, K, 4), counts=new(3, E, 4))
        kernels.HipKernels().route_topk(x, raw['idx'][1:-1].view(dtype), raw['w'][1:-1].view(torch.float32),
                                        counts=raw['counts'][1].view(torch.int32), **kw)
        assert torch.equal(raw['idx'][1:-1].view(dtype).long(), idx.long())
        assert torch.equal(raw['w'][1:-1].view(torch.float32), w)
        assert torch.equal(raw['counts'][1].view(torch.int32), counts)
        assert all(bool((t[0] == 0xa5).all()) and bool((t[-1] == 0xa5).all()) for t in raw.values())


def test_graph_replays_and_no_tokens():
    """Captured with counts (the clearing kernel is part of the graph): three replays on new logits equal the eager
    call.  T == 0: empty outputs and zero counts."""
    import deep_ep
    T, E, K, G, kept, _ = CASES[2]
    x = torch.zeros((T, E), device='cuda')
    run = lambda: deep_ep.route_topk(x, K, num_groups=G, num_topk_groups=kept, return_counts=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for seed in range(3):
        x.copy_(_inputs(T, E, torch.float32, False, seed)[0])
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, run()))
    idx, w, counts = deep_ep.route_topk(x[:0], K, return_counts=True)
    assert tuple(idx.shape) == tuple(w.shape) == (0, K) and idx.dtype == deep_ep.topk_idx_t
    assert tuple(counts.shape) == (E,) and int(counts.abs().sum()) == 0
