"""route_topk against the route a caller has without it, one JSON line (also written to `--out`): for each case
T x E (K = 8, sigmoid with a bias; E = 256 in 8 groups of which 4 stay, E = 384 without groups; T = 8192, a prefill
step, and T = 128, a decoding step), in one process on the same float32 logits,
  (a) fused    route_topk(logits, 8, bias=..., num_groups=..., num_topk_groups=..., routed_scaling_factor=2.5)
  (e) eager    the gate as a DeepSeek-V3 style model writes it in torch (`eager_gate` below: sigmoid, bias add, group
               view, topk(2).sum, topk over groups, scatter mask, masked_fill, topk, gather, sum, divide, scale);
               timed twice a round (`_again`): the ratio of its two medians is the same-route spread of the run

Device events after `--warmup` calls; `--rounds` rounds alternating the routes, `--iters` calls a round; medians with
the min-max of the rounds.  Before any timing the two routes are compared on the whole shape: the share of rows with
the same set of experts (near-ties may differ: torch.topk has no tie rule) and the largest weight difference on them.

Three more forms of the fused call are timed in the same rounds, without an eager counterpart: at T = 8192, E = 256
with `return_counts` and with bfloat16 logits under the softmax, and at the bounds the function accepts, T = 8192,
E = 1024 in 64 groups of which 8 stay, K = 64.

Reported, not gated (nobody has measured a number before this tool): the ratio (a) / (e), whether the fused call beats
the eager route by more than the same-route spread, and the algorithmic bytes of (a) -- 4 T E read, 12 T K written
(int64 indices and float32 weights) -- over its median."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, SCALE = 8, 2.5
# T, E, groups, kept groups
CASES = [(8192, 256, 8, 4), (128, 256, 8, 4), (8192, 384, 1, 1), (128, 384, 1, 1)]


def eager_gate(logits, bias, G, kept):
    T, E = logits.shape
    scores = logits.sigmoid()
    sel = scores + bias
    if G > 1:
        group_scores = sel.view(T, G, -1).topk(2, dim=-1)[0].sum(dim=-1)
        group_idx = torch.topk(group_scores, k=kept, dim=-1, sorted=False)[1]
        group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1)
        score_mask = group_mask.unsqueeze(-1).expand(T, G, E // G).reshape(T, E)
        sel = sel.masked_fill(~score_mask.bool(), float('-inf'))
    idx = torch.topk(sel, k=K, dim=-1, sorted=False)[1]
    w = scores.gather(1, idx)
    return idx, w / w.sum(dim=-1, keepdim=True) * SCALE


def timed(fn, iters: int) -> float:
    """Microseconds per call of fn over `iters` back-to-back calls (device events)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def bench(args):
    import deepep_amd
    variants, out = {}, {}
    for T, E, G, kept in CASES:
        g = torch.Generator(device='cuda').manual_seed(T + E)
        logits = torch.randn((T, E), device='cuda', generator=g) * 1.5
        bias = torch.randn((E,), device='cuda', generator=g) * 0.1
        fused = lambda logits=logits, bias=bias, G=G, kept=kept: deepep_amd.route_topk(
            logits, K, bias=bias, num_groups=G, num_topk_groups=kept, routed_scaling_factor=SCALE)
        eager = lambda logits=logits, bias=bias, G=G, kept=kept: eager_gate(logits, bias, G, kept)
        (idx, w), (e_idx, e_w) = fused(), eager()
        order, e_order = idx.sort(dim=-1), e_idx.sort(dim=-1)
        same = (order.values == e_order.values).all(dim=-1)
        diff = (w.gather(1, order.indices) - e_w.gather(1, e_order.indices)).abs().max(dim=-1).values
        name = f't{T}_e{E}'
        out[name + '_rows_with_the_same_experts'] = round(float(same.double().mean()), 6)
        out[name + '_largest_weight_difference'] = float(diff[same].max())
        assert out[name + '_rows_with_the_same_experts'] > 0.99 and out[name + '_largest_weight_difference'] < 1e-5, name
        variants.update({name + '_fused': fused, name + '_eager': eager, name + '_eager_again': eager})

    g = torch.Generator(device='cuda').manual_seed(1)
    x256 = torch.randn((8192, 256), device='cuda', generator=g) * 1.5
    x256_bf16, x1024 = x256.bfloat16(), torch.randn((8192, 1024), device='cuda', generator=g) * 1.5
    variants.update({
        't8192_e256_counts_fused': lambda: deepep_amd.route_topk(x256, K, num_groups=8, num_topk_groups=4,
                                                                 return_counts=True),
        't8192_e256_bf16_softmax_fused': lambda: deepep_amd.route_topk(x256_bf16, K, score_func='softmax', num_groups=8,
                                                                       num_topk_groups=4),
        't8192_e1024_g64_k64_fused': lambda: deepep_amd.route_topk(x1024, 64, num_groups=64, num_topk_groups=8)})

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():                # alternating: one round of each, then the next round
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    for T, E, _, _ in CASES:
        p = f't{T}_e{E}_'
        nbytes = 4 * T * E + 12 * T * K
        spread = abs(med[p + 'eager'] / med[p + 'eager_again'] - 1)
        out[p + 'same_route_spread'] = round(spread, 4)
        out[p + 'fused_over_eager'] = round(med[p + 'fused'] / med[p + 'eager'], 4)
        out[p + 'fused_beats_eager_by_more_than_the_spread'] = med[p + 'fused'] < med[p + 'eager'] * (1 - spread)
        out[p + 'fused_algorithmic_bytes'] = nbytes
        out[p + 'fused_tbps'] = round(nbytes / (med[p + 'fused'] * 1e-6) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'router_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_router needs a GPU'
    torch.cuda.set_device(0)
    out = dict(tool='bench_router', device=torch.cuda.get_device_name(0), num_topk=K, rounds=args.rounds,
               iters=args.iters, warmup=args.warmup, **bench(args))
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
