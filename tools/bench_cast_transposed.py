"""The transposed MXFP8 cast against the route it replaces, one JSON line: for each shape (default 65536 x 7168, the
expanded rows of 8192 tokens x top-8, and 8192 x 7168), in one process on the same input,
  (a) transposed          cast_to_mxfp8_transposed(x)
  (b) both                cast_to_mxfp8_transposed(x, with_rowwise=True)
  (c) transpose_then_cast per_token_cast_to_fp8(x.t().contiguous(), ..., group_size=32): the parent's route to (a)'s
                          bytes, timed twice a round (`_again`): the ratio of its two medians is the same-route spread
  (d) rowwise             per_token_cast_to_fp8(x, ..., group_size=32): the byte-rate yardstick
  (e) = (c) + (d)         the parent's route to (b)'s bytes (the sum of the two medians)

Device events after `--warmup` calls; `--rounds` rounds alternating the forms, `--iters` calls a round; medians with
the min-max of the rounds.  Before any timing every form is checked bitwise: (a) and (b) against (c) and (d) on the
whole shape, and against tests/mxt_ref (the CPU reference) on the first `--check-rows` tokens (a block's bytes depend
on its own 32 rows only, so a prefix of the rows has the prefix of the reference).  The rates are algorithmic bytes
(3 N H + N H / 32 for (a), 4 N H + N H / 16 for (b), 3 N H + N H / 32 for (d)) over the median."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def bench_shape(N, H, args):
    import deepep_amd
    from tests.mxt_ref import mxt_pair, rowwise_pair
    kw = dict(round_scale=True, use_ue8m0=True, group_size=32)
    g = torch.Generator(device='cuda').manual_seed(N + H)
    x = torch.randn((N, H), device='cuda', generator=g)
    x = (x * torch.exp2(torch.randint(-6, 6, (N, 1), device='cuda', generator=g).float())).to(torch.bfloat16)

    variants = {
        'transposed': lambda: deepep_amd.cast_to_mxfp8_transposed(x),
        'transpose_then_cast': lambda: deepep_amd.per_token_cast_to_fp8(x.t().contiguous(), **kw),
        'both': lambda: deepep_amd.cast_to_mxfp8_transposed(x, with_rowwise=True),
        'rowwise': lambda: deepep_amd.per_token_cast_to_fp8(x, **kw),
        'transpose_then_cast_again': lambda: deepep_amd.per_token_cast_to_fp8(x.t().contiguous(), **kw),
    }
    # the checks, before any timing
    q_t, sf_t = variants['transposed']()
    (q, sf), (q_t2, sf_t2) = variants['both']()
    q_t_route, sf_t_route = variants['transpose_then_cast']()
    q_route, sf_route = variants['rowwise']()
    torch.cuda.synchronize()
    checks = dict(
        transposed_equals_transpose_then_cast=same(q_t, q_t_route) and same(sf_t, sf_t_route),
        both_equals_transpose_then_cast=same(q_t2, q_t_route) and same(sf_t2, sf_t_route),
        both_equals_rowwise=same(q, q_route) and same(sf, sf_route))
    n = min(N, args.check_rows)
    ref_t, ref_row = mxt_pair(x[:n].cpu()), rowwise_pair(x[:n].cpu())
    checks['transposed_equals_cpu_reference'] = all(
        same(a[:, :n].cpu(), ref_t[0]) and same(b[:, :n // 32].cpu(), ref_t[1])
        for a, b in ((q_t, sf_t), (q_t2, sf_t2)))
    checks['rowwise_equals_cpu_reference'] = same(q[:n].cpu(), ref_row[0]) and same(sf[:n].cpu(), ref_row[1])
    assert all(checks.values()), checks
    del q_t, sf_t, q, sf, q_t2, sf_t2, q_t_route, sf_t_route, q_route, sf_route

    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():                # alternating: one round of each, then the next round
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    out = dict(rows=N, hidden=H, checked_rows_on_cpu=n, **checks)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    route_a = med['transpose_then_cast']
    route_b = route_a + med['rowwise']
    out['transpose_then_cast_plus_rowwise_us_median'] = round(route_b, 2)
    out['same_route_spread'] = round(abs(route_a / med['transpose_then_cast_again'] - 1), 4)
    out['transposed_over_transpose_then_cast'] = round(med['transposed'] / route_a, 4)
    out['both_over_transpose_then_cast_plus_rowwise'] = round(med['both'] / route_b, 4)
    nh = N * H
    for name, moved in (('transposed', 3 * nh + nh // 32), ('both', 4 * nh + nh // 16), ('rowwise', 3 * nh + nh // 32)):
        out[f'{name}_tbps'] = round(moved / (med[name] * 1e-6) / 1e12, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='65536x7168,8192x7168')
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--check-rows', type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cast_transposed needs a GPU'
    torch.cuda.set_device(0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    out = dict(tool='bench_cast_transposed', device=torch.cuda.get_device_name(0), rounds=args.rounds,
               iters=args.iters, warmup=args.warmup, shapes=[bench_shape(N, H, args) for N, H in shapes])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
