"""MXFP4 against MXFP8 at EP = 1, one JSON line: per_token_cast_to_fp4, per_token_cast_back_fp4 and the cached
dispatch(..., cast_to_fp4=True, do_expand=True), each beside its MXFP8 sibling in the same process on the same inputs.

Device events after `--warmup` calls; `--rounds` rounds alternating the forms, `--iters` calls a round; medians with
the min-max of the rounds.  Every MXFP8 form is timed twice a round (`*_fp8` and `*_fp8_again`): the ratio of its two
medians is the same-route spread of the run.  Before any timing the FP4 cast, the cast back and the cached dispatch
are checked bitwise against tests/fp4_ref (the cast and the cast back row block by row block on the CPU; the dispatch
against the tuple dispatch of the reference pair)."""
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
    assert torch.cuda.is_available(), 'bench_fp4 needs a GPU'
    torch.cuda.set_device(0)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29647')
    dist.init_process_group('gloo', rank=0, world_size=1)
    import deepep_amd
    from deepep_amd import ElasticBuffer
    from tests.fp4_ref import fp4_back_ref, fp4_pair
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    torch.manual_seed(0)
    scores = torch.rand((T, E), device='cuda')
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    idx = idx.to(torch.int64)
    x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    buf = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    fresh = dict(topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    mx = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True, fp8_group_size=32)

    # the checks, before any timing
    q4, sf4 = deepep_amd.per_token_cast_to_fp4(x)
    back4 = deepep_amd.per_token_cast_back_fp4(q4, sf4)
    torch.cuda.synchronize()
    x_cpu, q4_cpu, sf4_cpu, back4_cpu = x.cpu(), q4.cpu(), sf4.cpu(), back4.cpu()
    cast_same = back_same = True
    q_ref = torch.empty_like(q4_cpu)
    sf_ref = torch.empty_like(sf4_cpu)
    for r in range(0, T, 1024):
        q_ref[r:r + 1024], sf_ref[r:r + 1024] = fp4_pair(x_cpu[r:r + 1024])
        cast_same &= torch.equal(q_ref[r:r + 1024], q4_cpu[r:r + 1024]) and \
            torch.equal(sf_ref[r:r + 1024], sf4_cpu[r:r + 1024])
        back_same &= torch.equal(fp4_back_ref(q_ref[r:r + 1024], sf_ref[r:r + 1024]).view(torch.int16),
                                 back4_cpu[r:r + 1024].view(torch.int16))
    assert cast_same, 'per_token_cast_to_fp4 differs from tests/fp4_ref.fp4_pair'
    assert back_same, 'per_token_cast_back_fp4 differs from tests/fp4_ref.fp4_back_ref'
    ref = buf.dispatch((q_ref.cuda(), sf_ref.cuda()), **fresh)
    handle = ref[3]
    cached = dict(handle=handle, topk_weights=w, do_expand=True)
    got = buf.dispatch(x, cast_to_fp4=True, **cached)
    torch.cuda.synchronize()
    dispatch_same = (torch.equal(ref[0][0], got[0][0]) and torch.equal(ref[0][1], got[0][1]) and
                     torch.equal(ref[2], got[2]))
    assert dispatch_same, 'dispatch(x, cast_to_fp4=True) differs from the tuple dispatch of the reference pair'
    del ref, got, back4
    q8, sf8 = deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32)

    variants = {
        'cast_fp8': lambda: deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32),
        'cast_fp4': lambda: deepep_amd.per_token_cast_to_fp4(x),
        'cast_fp8_again': lambda: deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32),
        'cast_back_fp8': lambda: deepep_amd.per_token_cast_back(q8, sf8),
        'cast_back_fp4': lambda: deepep_amd.per_token_cast_back_fp4(q4, sf4),
        'cast_back_fp8_again': lambda: deepep_amd.per_token_cast_back(q8, sf8),
        'dispatch_fp8': lambda: buf.dispatch(x, **mx, **cached),
        'dispatch_fp4': lambda: buf.dispatch(x, cast_to_fp4=True, **cached),
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
    out = dict(tool='bench_fp4', device=torch.cuda.get_device_name(0), tokens=T, hidden=H, topk=K, experts=E,
               expanded_rows=int(handle.num_expanded_tokens), rounds=args.rounds, iters=args.iters,
               warmup=args.warmup, cast_bitwise_equal_to_reference=cast_same,
               cast_back_bitwise_equal_to_reference=back_same, dispatch_bitwise_equal_to_tuple_dispatch=dispatch_same)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 2)
        out[f'{name}_us_min'] = round(min(v), 2)
        out[f'{name}_us_max'] = round(max(v), 2)
    for kind in ('cast', 'cast_back', 'dispatch'):
        out[f'{kind}_fp4_over_fp8'] = round(med[f'{kind}_fp4'] / med[f'{kind}_fp8'], 4)
        out[f'{kind}_fp4_over_fp8_again'] = round(med[f'{kind}_fp4'] / med[f'{kind}_fp8_again'], 4)
        out[f'{kind}_fp8_same_route_spread'] = round(abs(med[f'{kind}_fp8'] / med[f'{kind}_fp8_again'] - 1), 4)
    # the bytes each codec kernel must move: bf16 rows on one side, codes and exponent bytes on the other
    out['cast_fp4_gbps'] = round((T * H * 2 + T * H // 2 + T * H // 32) / (med['cast_fp4'] * 1e-6) / 1e9, 1)
    out['cast_fp8_gbps'] = round((T * H * 2 + T * H + T * H // 32) / (med['cast_fp8'] * 1e-6) / 1e9, 1)
    out['cast_back_fp4_gbps'] = round((T * H * 2 + T * H // 2 + T * H // 32) / (med['cast_back_fp4'] * 1e-6) / 1e9, 1)
    out['cast_back_fp8_gbps'] = round((T * H * 2 + T * H + T * H // 32) / (med['cast_back_fp8'] * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
