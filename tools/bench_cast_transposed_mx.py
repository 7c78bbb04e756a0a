"""The transposed MXFP4 and MXFP6 casts against the route they replace, one JSON line (also written to `--out`): for
each shape (default 65536 x 7168, the expanded rows of 8192 tokens x top-8, and 8192 x 7168) and each format X in
fp4, fp6, in one process on the same input,
  (a) transposed          cast_to_mxfpX_transposed(x)
  (b) both                cast_to_mxfpX_transposed(x, with_rowwise=True)
  (c) transpose_then_cast per_token_cast_to_fpX(x.t().contiguous()): the parent's route to (a)'s bytes, timed twice a
                          round (`_again`): the ratio of its two medians is the same-route spread of the run
  (d) rowwise             per_token_cast_to_fpX(x)
  (e) = (c) + (d)         the parent's route to (b)'s bytes (the sum of the two medians)
and, in the same rounds, the MXFP8 sibling cast_to_mxfp8_transposed(x) and (x, with_rowwise=True).

Device events after `--warmup` calls; `--rounds` rounds alternating the forms, `--iters` calls a round; medians with
the min-max of the rounds.  Before any timing every form is checked bitwise: (a) and (b) against (c) and (d) on the
whole shape, and against tests/mxt46_ref (the CPU reference) on the first `--check-rows` tokens (a block's bytes depend
on its own 32 rows only, so a prefix of the rows has the prefix of the reference).

The gates, all inside this run: (a) / (c) and (b) / (e) must lie below the ratio of the routes' algorithmic bytes by
more than the same-route spread.  With b = bits / 8 bytes a code, (a) moves (2 + b) N H + N H / 32 bytes and (c) 4 N H
more (the transpose's read and write of a bf16 matrix: 6 N H of bf16 traffic against 2 N H); (b) moves
(2 + 2b) N H + N H / 16 and (e) is (c) plus (d) = (a)'s bytes: 0.39 / 0.34 for FP4, 0.41 / 0.37 for FP6.  The tool
prints the line, then exits 1 if a gate fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def check_format(fmt, x, variants, check_rows):
    """Every form of one format against the other route (whole shape) and the CPU reference (a prefix)."""
    N = x.shape[0]
    q_t, sf_t = variants['transposed']()
    (q, sf), (q_t2, sf_t2) = variants['both']()
    q_t_route, sf_t_route = variants['transpose_then_cast']()
    q_route, sf_route = variants['rowwise']()
    torch.cuda.synchronize()
    checks = dict(
        transposed_equals_transpose_then_cast=same(q_t, q_t_route) and same(sf_t, sf_t_route),
        both_equals_transpose_then_cast=same(q_t2, q_t_route) and same(sf_t2, sf_t_route),
        both_equals_rowwise=same(q, q_route) and same(sf, sf_route))
    n = min(N, check_rows)
    ref_t, ref_row = fmt.transposed_pair(x[:n].cpu()), fmt.rowwise_pair(x[:n].cpu())
    checks['transposed_equals_cpu_reference'] = all(
        same(a[:, :fmt.row_bytes(n)].cpu(), ref_t[0]) and same(b[:, :n // 32].cpu(), ref_t[1])
        for a, b in ((q_t, sf_t), (q_t2, sf_t2)))
    checks['rowwise_equals_cpu_reference'] = same(q[:n].cpu(), ref_row[0]) and same(sf[:n].cpu(), ref_row[1])
    assert all(checks.values()), (fmt.name, checks)
    return dict(checked_rows_on_cpu=n, **checks)


def bench_shape(N, H, args):
    import deepep_amd
    from tests.mxt46_ref import FORMATS
    g = torch.Generator(device='cuda').manual_seed(N + H)
    x = torch.randn((N, H), device='cuda', generator=g)
    x = (x * torch.exp2(torch.randint(-6, 6, (N, 1), device='cuda', generator=g).float())).to(torch.bfloat16)

    variants, checks = {}, {}
    for fmt in FORMATS:
        cast_t, cast = getattr(deepep_amd, fmt.public), getattr(deepep_amd, fmt.rowwise_cast)
        mine = {
            'transposed': lambda cast_t=cast_t: cast_t(x),
            'transpose_then_cast': lambda cast=cast: cast(x.t().contiguous()),
            'both': lambda cast_t=cast_t: cast_t(x, with_rowwise=True),
            'rowwise': lambda cast=cast: cast(x),
            'transpose_then_cast_again': lambda cast=cast: cast(x.t().contiguous()),
        }
        checks[fmt.name] = check_format(fmt, x, mine, args.check_rows)     # before any timing
        variants.update({f'{fmt.name}_{k}': v for k, v in mine.items()})
    variants['fp8_transposed'] = lambda: deepep_amd.cast_to_mxfp8_transposed(x)
    variants['fp8_both'] = lambda: deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True)

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
    for fmt in FORMATS:
        p = fmt.name + '_'
        code = nh * fmt.bits // 8
        bytes_a = 2 * nh + code + nh // 32
        bytes_b = 2 * nh + 2 * code + nh // 16
        route_a = med[p + 'transpose_then_cast']
        route_b = route_a + med[p + 'rowwise']
        spread = abs(route_a / med[p + 'transpose_then_cast_again'] - 1)
        ratio_a, ratio_b = med[p + 'transposed'] / route_a, med[p + 'both'] / route_b
        bytes_ratio_a = bytes_a / (bytes_a + 4 * nh)
        bytes_ratio_b = bytes_b / (bytes_a + 4 * nh + bytes_a)
        out[p + 'transpose_then_cast_plus_rowwise_us_median'] = round(route_b, 2)
        out[p + 'same_route_spread'] = round(spread, 4)
        out[p + 'transposed_over_transpose_then_cast'] = round(ratio_a, 4)
        out[p + 'both_over_transpose_then_cast_plus_rowwise'] = round(ratio_b, 4)
        out[p + 'bytes_ratio_transposed'] = round(bytes_ratio_a, 4)
        out[p + 'bytes_ratio_both'] = round(bytes_ratio_b, 4)
        out[p + 'transposed_tbps'] = round(bytes_a / (med[p + 'transposed'] * 1e-6) / 1e12, 3)
        out[p + 'both_tbps'] = round(bytes_b / (med[p + 'both'] * 1e-6) / 1e12, 3)
        out[p + 'rowwise_tbps'] = round(bytes_a / (med[p + 'rowwise'] * 1e-6) / 1e12, 3)
        out[p + 'transposed_over_fp8_transposed'] = round(med[p + 'transposed'] / med['fp8_transposed'], 4)
        out[p + 'both_over_fp8_both'] = round(med[p + 'both'] / med['fp8_both'], 4)
        gates[p + 'transposed'] = bool(ratio_a < bytes_ratio_a - spread)
        gates[p + 'both'] = bool(ratio_b < bytes_ratio_b - spread)
    out['fp8_transposed_tbps'] = round((3 * nh + nh // 32) / (med['fp8_transposed'] * 1e-6) / 1e12, 3)
    out['fp8_both_tbps'] = round((4 * nh + nh // 16) / (med['fp8_both'] * 1e-6) / 1e12, 3)
    out['gates'] = gates
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='65536x7168,8192x7168')
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--check-rows', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx46_transposed_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cast_transposed_mx needs a GPU'
    torch.cuda.set_device(0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    out = dict(tool='bench_cast_transposed_mx', device=torch.cuda.get_device_name(0), rounds=args.rounds,
               iters=args.iters, warmup=args.warmup, shapes=[bench_shape(N, H, args) for N, H in shapes])
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    sys.exit(0 if all(all(s['gates'].values()) for s in out['shapes']) else 1)


if __name__ == '__main__':
    main()
