"""Time grouped_gemm_mx / grouped_gemm_mx_wgrad against what a caller did before them: the cast back of both operands
followed by one torch.matmul per expert (bf16, hipBLASLt).  Device events around each call, a warm-up, the routes
alternated inside one process, medians with min-max; one JSON document on stdout (and in --out).

  python tools/bench_grouped_gemm_mx.py [--experts 8] [--rows 1024] [--rounds 15] [--out profiles/grouped_gemm_mx.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepep_amd  # noqa: E402

CAST = {'fp8': (lambda t: deepep_amd.per_token_cast_to_fp8(t, True, True, group_size=32), deepep_amd.per_token_cast_back),
        'fp4': (deepep_amd.per_token_cast_to_fp4, deepep_amd.per_token_cast_back_fp4),
        'fp6': (deepep_amd.per_token_cast_to_fp6, deepep_amd.per_token_cast_back_fp6)}


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def routes_fprop(fmt, E, rows, K, O):
    cast, back = CAST[fmt]
    N = E * rows
    a = cast(torch.randn((N, K), device='cuda').to(torch.bfloat16))
    b = cast((torch.randn((E * O, K), device='cuda') * K ** -0.5).to(torch.bfloat16))
    b3 = tuple(t.view(E, O, -1) for t in b)
    ends = torch.arange(1, E + 1, dtype=torch.int32, device='cuda') * rows

    def ours():
        return deepep_amd.grouped_gemm_mx(a, b3, ends)

    def before():
        x, w = back(*a), back(*b).view(E, O, K)
        return [torch.matmul(x[e * rows:(e + 1) * rows], w[e].t()) for e in range(E)]
    return ours, before


def routes_wgrad(fmt, E, rows, O, H):
    cast, back = CAST[fmt]
    N = E * rows
    dy = cast(torch.randn((O, N), device='cuda').to(torch.bfloat16))
    x = cast(torch.randn((H, N), device='cuda').to(torch.bfloat16))
    ends = torch.arange(1, E + 1, dtype=torch.int32, device='cuda') * rows

    def ours():
        return deepep_amd.grouped_gemm_mx_wgrad(dy, x, ends)

    def before():
        d, v = back(*dy), back(*x)
        return [torch.matmul(d[:, e * rows:(e + 1) * rows], v[:, e * rows:(e + 1) * rows].t()) for e in range(E)]
    return ours, before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--experts', type=int, default=8)
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    E, rows = args.experts, args.rows
    shapes = [('fprop 7168->2048', routes_fprop, 7168, 2048), ('fprop 2048->7168', routes_fprop, 2048, 7168),
              ('wgrad 2048x7168', routes_wgrad, 2048, 7168)]
    result = {'experts': E, 'rows_per_expert': rows, 'rounds': args.rounds, 'cases': []}
    for label, make, d0, d1 in shapes:
        flops = 2.0 * E * rows * d0 * d1
        for fmt in CAST:
            ours, before = make(fmt, E, rows, d0, d1)
            times = {'grouped_gemm_mx': [], 'cast_back+matmul': []}
            for r in range(args.warmup + args.rounds):
                for name, fn in (('grouped_gemm_mx', ours), ('cast_back+matmul', before)):
                    t = timed(fn)
                    if r >= args.warmup:
                        times[name].append(t)
            case = {'shape': label, 'format': fmt}
            for name, ts in times.items():
                med = statistics.median(ts)
                case[name] = {'median_us': round(med, 1), 'min_us': round(min(ts), 1), 'max_us': round(max(ts), 1),
                              'tflops': round(flops / med / 1e6, 1)}
            case['before_over_ours'] = round(case['cast_back+matmul']['median_us'] / case['grouped_gemm_mx']['median_us'], 3)
            result['cases'].append(case)
            print(json.dumps(case), file=sys.stderr)
            del ours, before
            torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
