"""swiglu_backward_cast_to_mx against the route a caller has without it, one JSON line (also written to `--out`): at
N x I (default 65536 x 2048, h bf16 [N, 2 I], dact bf16 [N, I]), for each format (fp8, fp6, fp4) and with and without
the transposed pair, in one process on the same inputs,
  (a) fused            swiglu_backward_cast_to_mx(h, dact, fmt[, with_transposed=True])
  (u) unfused          the eager bf16 formula -- s = sigmoid(g), dgate = da * u * s * (1 + g * (1 - s)),
                       dup = da * g * s, cat -- then per_token_cast_to_fpX or
                       cast_to_mxfpX_transposed(..., with_rowwise=True); timed twice a round (`_again`): the ratio of
                       its two medians is the same-route spread of the run
  (f) forward          swiglu_cast_to_mx(h, fmt[, with_transposed=True]), the forward kernel beside it

Device events after `--warmup` calls; `--rounds` rounds alternating the routes, `--iters` calls a round; medians with
the min-max of the rounds.  Before any timing every form is checked against rule 2 on the whole shape: its pairs are,
bit for bit, the library's casts of the dh it returns.

Acceptance (`faster_than_unfused_beyond_the_spread`): 1 - (a) / (u) exceeds the same-route spread, per form.  The
algorithmic bytes of (a) -- 6 N I read, and 2 (b N I / 8 + N I / 32) written per pair of b-bit codes -- over its
median are its TB/s; the forward's are 4 N I read and b N I / 8 + N I / 32 written per pair."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BITS = {'fp8': 8, 'fp6': 6, 'fp4': 4}


def timed(fn, iters: int) -> float:
    """Microseconds per call of fn over `iters` back-to-back calls (device events)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def same(a, b) -> bool:
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def rowwise_cast(fmt):
    import deepep_amd
    if fmt == 'fp8':
        return lambda x: deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32)
    return getattr(deepep_amd, f'per_token_cast_to_{fmt}')


def bench(N, I, args):
    import deepep_amd
    gen = torch.Generator(device='cuda').manual_seed(N + I)
    h = (torch.randn((N, 2 * I), device='cuda', generator=gen) * 4).to(torch.bfloat16)
    dact = (torch.randn((N, I), device='cuda', generator=gen) * 4).to(torch.bfloat16)

    def eager_dh():
        g, u = h[:, :I], h[:, I:]
        s = torch.sigmoid(g)
        return torch.cat([dact * u * s * (1 + g * (1 - s)), dact * g * s], dim=1)

    variants, checks = {}, {}
    for fmt in BITS:
        for t in (False, True):
            name = fmt + ('_t' if t else '')
            cast_t = getattr(deepep_amd, f'cast_to_mx{fmt}_transposed')
            cast = (lambda x, cast_t=cast_t: cast_t(x, with_rowwise=True)) if t else rowwise_cast(fmt)
            unfused = lambda cast=cast: cast(eager_dh())
            mine = {'fused': lambda fmt=fmt, t=t: deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, with_transposed=t),
                    'unfused': unfused, 'unfused_again': unfused,
                    'forward': lambda fmt=fmt, t=t: deepep_amd.swiglu_cast_to_mx(h, fmt, with_transposed=t)}
            *got, dh = deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, with_transposed=t, return_dh=True)  # rule 2
            want = cast(dh)
            flat = lambda r: [x for pair in r for x in pair] if t else list(r)
            torch.cuda.synchronize()
            checks[name] = all(same(a, b) for a, b in zip(flat(got), flat(want)))
            assert checks[name], name
            del got, want, dh
            variants.update({f'{name}_{k}': v for k, v in mine.items()})

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():                # alternating: one round of each, then the next round
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    out = dict(rows=N, inter=I, pairs_equal_the_casts_of_dh=checks)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    ni = N * I
    for fmt, bits in BITS.items():
        for t in (False, True):
            p = fmt + ('_t_' if t else '_')
            pair = ni * bits // 8 + ni // 32
            nbytes, fwd_bytes = 6 * ni + (2 if t else 1) * 2 * pair, 4 * ni + (2 if t else 1) * pair
            spread = abs(med[p + 'unfused'] / med[p + 'unfused_again'] - 1)
            out[p + 'same_route_spread'] = round(spread, 4)
            out[p + 'fused_over_unfused'] = round(med[p + 'fused'] / med[p + 'unfused'], 4)
            out[p + 'faster_than_unfused_beyond_the_spread'] = 1 - med[p + 'fused'] / med[p + 'unfused'] > spread
            out[p + 'fused_algorithmic_bytes'] = nbytes
            out[p + 'fused_tbps'] = round(nbytes / (med[p + 'fused'] * 1e-6) / 1e12, 3)
            out[p + 'forward_tbps'] = round(fwd_bytes / (med[p + 'forward'] * 1e-6) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='65536x2048')
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swiglu_backward_cast_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_swiglu_backward_cast needs a GPU'
    torch.cuda.set_device(0)
    N, I = (int(v) for v in args.shape.split('x'))
    out = dict(tool='bench_swiglu_backward_cast', device=torch.cuda.get_device_name(0), rounds=args.rounds,
               iters=args.iters, warmup=args.warmup, **bench(N, I, args))
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
