"""The requantisation along the tokens against the route it replaces, one JSON line (also written to `--out`): for each
shape (default 65536 x 7168, the expanded rows of 8192 tokens x top-8, and 8192 x 7168) and each of the five forms
(an FP8 pair with fp32, packed UE8M0 or per-32 exponent-byte factors; an MXFP4 pair; an MXFP6 pair), in one process on
the same pair,
  (a) fused               requant_mxfpX_transposed(q, sf)
  (c) back_then_cast      cast_to_mxfpX_transposed(per_token_cast_back*(q, sf)): the route it replaces, two launches and
                          a bf16 [N, H] buffer, timed twice a round (`_again`): the ratio of its two medians is the
                          same-route spread of the run
  (t) cast_only           cast_to_mxfpX_transposed(y) on bf16 rows that already exist, for context

Device events after `--warmup` calls; `--rounds` rounds alternating the routes, `--iters` calls a round; medians with
the min-max of the rounds.  Before any timing every form's (a) is checked bitwise against (c) on the whole shape.

The gate, inside this run, per form and shape: (a) must lie below (c) by more than the same-route spread.  The ratio of
the routes' algorithmic bytes is reported, not gated: with b bytes a code, (a) moves 2 b N H + N H / 16 (+ the fp32 or
packed factors' N H / 32 or N H / 128 in place of one N H / 32) and (c) 4 N H more (the bf16 rows written and read
back): 0.34 for MXFP8, 0.21 for FP4, 0.28 for FP6.  So are (a) / (t) and the algorithmic TB/s of (a).  The tool prints
the line, then exits 1 if a gate fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# form: (public function, cast back, transposed cast, the row-wise cast and its keywords, bits a code, factor bytes per
# element of the matrix)
FORMS = {
    'fp32': ('requant_mxfp8_transposed', 'per_token_cast_back', 'cast_to_mxfp8_transposed', 'per_token_cast_to_fp8',
             dict(), 8, 4 / 128),
    'ue8m0': ('requant_mxfp8_transposed', 'per_token_cast_back', 'cast_to_mxfp8_transposed', 'per_token_cast_to_fp8',
              dict(round_scale=True, use_ue8m0=True), 8, 1 / 128),
    'mx': ('requant_mxfp8_transposed', 'per_token_cast_back', 'cast_to_mxfp8_transposed', 'per_token_cast_to_fp8',
           dict(round_scale=True, use_ue8m0=True, group_size=32), 8, 1 / 32),
    'fp4': ('requant_mxfp4_transposed', 'per_token_cast_back_fp4', 'cast_to_mxfp4_transposed', 'per_token_cast_to_fp4',
            dict(), 4, 1 / 32),
    'fp6': ('requant_mxfp6_transposed', 'per_token_cast_back_fp6', 'cast_to_mxfp6_transposed', 'per_token_cast_to_fp6',
            dict(), 6, 1 / 32),
}


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


def bench_shape(N, H, args):
    import deepep_amd
    g = torch.Generator(device='cuda').manual_seed(N + H)
    x = torch.randn((N, H), device='cuda', generator=g)
    x = (x * torch.exp2(torch.randint(-6, 6, (N, 1), device='cuda', generator=g).float())).to(torch.bfloat16)

    variants, checks = {}, {}
    for name, (public, back, cast_t, cast, kw, _, _) in FORMS.items():
        requant, back, cast_t = getattr(deepep_amd, public), getattr(deepep_amd, back), getattr(deepep_amd, cast_t)
        q, sf = getattr(deepep_amd, cast)(x, **kw)
        y = back(q, sf)                                     # (t)'s rows: what (c) writes and reads back
        mine = {
            'fused': lambda requant=requant, q=q, sf=sf: requant(q, sf),
            'back_then_cast': lambda back=back, cast_t=cast_t, q=q, sf=sf: cast_t(back(q, sf)),
            'cast_only': lambda cast_t=cast_t, y=y: cast_t(y),
            'back_then_cast_again': lambda back=back, cast_t=cast_t, q=q, sf=sf: cast_t(back(q, sf)),
        }
        got, want = mine['fused'](), mine['back_then_cast']()              # before any timing, on the whole shape
        torch.cuda.synchronize()
        checks[name] = dict(fused_equals_back_then_cast=same(got[0], want[0]) and same(got[1], want[1]))
        assert all(checks[name].values()), (name, checks[name])
        del got, want
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
    out = dict(rows=N, hidden=H, checks=checks)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    nh = N * H
    gates = {}
    for name, (_, _, _, _, _, bits, sf_bytes) in FORMS.items():
        p = name + '_'
        bytes_a = 2 * nh * bits // 8 + nh * sf_bytes + nh // 32
        route = med[p + 'back_then_cast']
        spread = abs(route / med[p + 'back_then_cast_again'] - 1)
        ratio = med[p + 'fused'] / route
        out[p + 'same_route_spread'] = round(spread, 4)
        out[p + 'fused_over_back_then_cast'] = round(ratio, 4)
        out[p + 'bytes_ratio'] = round(bytes_a / (bytes_a + 4 * nh), 4)
        out[p + 'fused_over_cast_only'] = round(med[p + 'fused'] / med[p + 'cast_only'], 4)
        out[p + 'fused_tbps'] = round(bytes_a / (med[p + 'fused'] * 1e-6) / 1e12, 3)
        gates[p + 'fused'] = bool(ratio < 1 - spread)
    out['gates'] = gates
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='65536x7168,8192x7168')
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'requant_transposed_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_requant_transposed needs a GPU'
    torch.cuda.set_device(0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    out = dict(tool='bench_requant_transposed', device=torch.cuda.get_device_name(0), rounds=args.rounds,
               iters=args.iters, warmup=args.warmup, shapes=[bench_shape(N, H, args) for N, H in shapes])
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    sys.exit(0 if all(all(s['gates'].values()) for s in out['shapes']) else 1)


if __name__ == '__main__':
    main()
