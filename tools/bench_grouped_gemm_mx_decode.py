"""Time grouped_gemm_mx_decode on the alignment-16 layout against the only route there was before it: grouped_gemm_mx
over the same tokens laid out at alignment 128.  Device events around each call, a warm-up, the two routes (and a
second series of the new one: the same-route spread) alternated inside one process, medians with min-max, and the
weight bytes (codes + exponent bytes) per second of each route; one JSON document on stdout (and in --out).

  python tools/bench_grouped_gemm_mx_decode.py [--experts 32] [--rounds 15] [--out profiles/grouped_gemm_mx_decode.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepep_amd  # noqa: E402

CAST = {'fp8': lambda t: deepep_amd.per_token_cast_to_fp8(t, True, True, group_size=32),
        'fp4': deepep_amd.per_token_cast_to_fp4}


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def laid_out(pair, E, tokens, align):
    """The pair's E * tokens rows as an expanded layout at `align` (zero codes and bytes between), and its expert_ends."""
    seg = (tokens + align - 1) // align * align
    out = tuple(torch.zeros((E * seg, t.shape[1]), dtype=torch.uint8, device='cuda').view(t.dtype) for t in pair)
    for o, t in zip(out, pair):
        o.view(torch.uint8).view(E, seg, -1)[:, :tokens] = t.view(torch.uint8).view(E, tokens, -1)
    ends = torch.arange(E, dtype=torch.int32, device='cuda') * seg + tokens
    return out, ends


def routes(fmt, E, tokens, K, O):
    cast = CAST[fmt]
    rows = cast(torch.randn((E * tokens, K), device='cuda').to(torch.bfloat16))
    b = cast((torch.randn((E * O, K), device='cuda') * K ** -0.5).to(torch.bfloat16))
    b3 = tuple(t.view(E, O, -1) for t in b)
    a16, ends16 = laid_out(rows, E, tokens, 16)
    a128, ends128 = laid_out(rows, E, tokens, 128)
    weight_bytes = sum(t.numel() * t.element_size() for t in b)
    return (lambda: deepep_amd.grouped_gemm_mx_decode(a16, b3, ends16, expert_alignment=16),
            lambda: deepep_amd.grouped_gemm_mx(a128, b3, ends128, expert_alignment=128), weight_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--experts', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    E = args.experts
    result = {'experts': E, 'rounds': args.rounds, 'cases': []}
    for K, O in ((7168, 4096), (2048, 7168)):
        for fmt in CAST:
            for tokens in (8, 16, 32, 64):
                decode, aligned128, weight_bytes = routes(fmt, E, tokens, K, O)
                series = (('grouped_gemm_mx_decode', decode), ('grouped_gemm_mx@128', aligned128),
                          ('grouped_gemm_mx_decode again', decode))
                times = {name: [] for name, _ in series}
                for r in range(args.warmup + args.rounds):
                    for name, fn in series:
                        t = timed(fn)
                        if r >= args.warmup:
                            times[name].append(t)
                case = {'shape': f'{K}->{O}', 'format': fmt, 'tokens_per_expert': tokens, 'weight_bytes': weight_bytes}
                for name, ts in times.items():
                    med = statistics.median(ts)
                    case[name] = {'median_us': round(med, 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1),
                                  'weight_gb_per_s': round(weight_bytes / med / 1e3, 1)}
                case['same_route_spread_us'] = round(abs(case['grouped_gemm_mx_decode']['median_us'] -
                                                         case['grouped_gemm_mx_decode again']['median_us']), 1)
                case['aligned128_over_decode'] = round(case['grouped_gemm_mx@128']['median_us'] /
                                                       case['grouped_gemm_mx_decode']['median_us'], 3)
                result['cases'].append(case)
                print(json.dumps(case), file=sys.stderr)
                del decode, aligned128
                torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
