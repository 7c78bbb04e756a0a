"""MXFP6 against MXFP8 and MXFP4 at EP = 1, one JSON line: per_token_cast_to_fp6 (and the cast kernel with either width
of its row stores), per_token_cast_back_fp6 and the cached dispatch(..., cast_to_fp6=True, do_expand=True), each beside
its MXFP8 and MXFP4 siblings in the same process on the same inputs.

Device events after `--warmup` calls; `--rounds` rounds alternating the forms, `--iters` calls a round; medians with
the min-max of the rounds.  Every MXFP8 form is timed twice a round (`*_fp8` and `*_fp8_again`): the ratio of its two
medians is the same-route spread of the run.  Before any timing the FP6 cast (both store widths), the cast back and the
cached dispatch are checked bitwise against tests/fp6_ref (the cast and the cast back row block by row block on the
CPU; the dispatch against the tuple dispatch of the reference pair)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.distributed as dist

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tokens', type=int, default=8192)
    ap.add_argument('--hidden', type=int, default=7168)
    ap.add_argument('--topk', type=int, default=8)
    ap.add_argument('--experts', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fp6 needs a GPU'
    torch.cuda.set_device(0)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29649')
    dist.init_process_group('gloo', rank=0, world_size=1)
    import deepep_amd
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    from tests.fp6_ref import fp6_back_ref, fp6_pair
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    torch.manual_seed(0)
    scores = torch.rand((T, E), device='cuda')
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    idx = idx.to(torch.int64)
    x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    buf = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    kern = HipKernels()
    fresh = dict(topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    mx = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True, fp8_group_size=32)

    def cast6(store_bytes):
        """per_token_cast_to_fp6 with the width of the row stores chosen (the same two allocations)."""
        q = torch.empty((T, 3 * H // 4), dtype=torch.uint8, device='cuda')
        sf = torch.empty((T, H // 32), dtype=torch.uint8, device='cuda')
        kern.cast_fp6(x, q, sf, store_bytes=store_bytes)
        return q, sf

    # the checks, before any timing
    q6, sf6 = deepep_amd.per_token_cast_to_fp6(x)
    forms = {8: cast6(8), 16: cast6(16)}
    back6 = deepep_amd.per_token_cast_back_fp6(q6, sf6)
    torch.cuda.synchronize()
    x_cpu, q6_cpu, sf6_cpu, back6_cpu = x.cpu(), q6.cpu(), sf6.cpu(), back6.cpu()
    cast_same = back_same = True
    q_ref = torch.empty_like(q6_cpu)
    sf_ref = torch.empty_like(sf6_cpu)
    for r in range(0, T, 1024):
        q_ref[r:r + 1024], sf_ref[r:r + 1024] = fp6_pair(x_cpu[r:r + 1024])
        cast_same &= torch.equal(q_ref[r:r + 1024], q6_cpu[r:r + 1024]) and \
            torch.equal(sf_ref[r:r + 1024], sf6_cpu[r:r + 1024])
        back_same &= torch.equal(fp6_back_ref(q_ref[r:r + 1024], sf_ref[r:r + 1024]).view(torch.int16),
                                 back6_cpu[r:r + 1024].view(torch.int16))
    forms_same = all(torch.equal(q.cpu(), q_ref) and torch.equal(sf.cpu(), sf_ref) for q, sf in forms.values())
    assert cast_same, 'per_token_cast_to_fp6 differs from tests/fp6_ref.fp6_pair'
    assert forms_same, 'a store form of the FP6 cast differs from tests/fp6_ref.fp6_pair'
    assert back_same, 'per_token_cast_back_fp6 differs from tests/fp6_ref.fp6_back_ref'
    ref = buf.dispatch((q_ref.cuda(), sf_ref.cuda()), **fresh)
    handle = ref[3]
    cached = dict(handle=handle, topk_weights=w, do_expand=True)
    got = buf.dispatch(x, cast_to_fp6=True, **cached)
    torch.cuda.synchronize()
    dispatch_same = (torch.equal(ref[0][0], got[0][0]) and torch.equal(ref[0][1], got[0][1]) and
                     torch.equal(ref[2], got[2]))
    assert dispatch_same, 'dispatch(x, cast_to_fp6=True) differs from the tuple dispatch of the reference pair'
    del ref, got, back6, forms
    q8, sf8 = deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32)
    q4, sf4 = deepep_amd.per_token_cast_to_fp4(x)

    variants = {
        'cast_fp8': lambda: deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32),
        'cast_fp4': lambda: deepep_amd.per_token_cast_to_fp4(x),
        'cast_fp6': lambda: deepep_amd.per_token_cast_to_fp6(x),
        'cast_fp6_stores8': lambda: cast6(8),
        'cast_fp6_stores16': lambda: cast6(16),
        'cast_fp8_again': lambda: deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32),
        'cast_back_fp8': lambda: deepep_amd.per_token_cast_back(q8, sf8),
        'cast_back_fp4': lambda: deepep_amd.per_token_cast_back_fp4(q4, sf4),
        'cast_back_fp6': lambda: deepep_amd.per_token_cast_back_fp6(q6, sf6),
        'cast_back_fp8_again': lambda: deepep_amd.per_token_cast_back(q8, sf8),
        'dispatch_fp8': lambda: buf.dispatch(x, **mx, **cached),
        'dispatch_fp4': lambda: buf.dispatch(x, cast_to_fp4=True, **cached),
        'dispatch_fp6': lambda: buf.dispatch(x, cast_to_fp6=True, **cached),
        'dispatch_fp8_again': lambda: buf.dispatch(x, **mx, **cached),
    }
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():                # alternating: one round of each, then the next round
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    out = dict(tool='bench_fp6', device=torch.cuda.get_device_name(0), tokens=T, hidden=H, topk=K, experts=E,
               expanded_rows=int(handle.num_expanded_tokens), rounds=args.rounds, iters=args.iters,
               warmup=args.warmup, cast_bitwise_equal_to_reference=cast_same,
               cast_store_forms_bitwise_equal_to_reference=forms_same,
               cast_back_bitwise_equal_to_reference=back_same, dispatch_bitwise_equal_to_tuple_dispatch=dispatch_same)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    for kind in ('cast', 'cast_back', 'dispatch'):
        out[f'{kind}_fp6_over_fp8'] = round(med[f'{kind}_fp6'] / med[f'{kind}_fp8'], 4)
        out[f'{kind}_fp6_over_fp8_again'] = round(med[f'{kind}_fp6'] / med[f'{kind}_fp8_again'], 4)
        out[f'{kind}_fp6_over_fp4'] = round(med[f'{kind}_fp6'] / med[f'{kind}_fp4'], 4)
        out[f'{kind}_fp8_same_route_spread'] = round(abs(med[f'{kind}_fp8'] / med[f'{kind}_fp8_again'] - 1), 4)
    out['cast_fp6_stores16_over_stores8'] = round(med['cast_fp6_stores16'] / med['cast_fp6_stores8'], 4)
    # the bytes each codec kernel must move: bf16 rows on one side, codes and exponent bytes on the other
    for name, row in (('fp8', H), ('fp6', 3 * H // 4), ('fp4', H // 2)):
        moved = T * H * 2 + T * row + T * H // 32
        out[f'cast_{name}_gbps'] = round(moved / (med[f'cast_{name}'] * 1e-6) / 1e9, 1)
        out[f'cast_back_{name}_gbps'] = round(moved / (med[f'cast_back_{name}'] * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
