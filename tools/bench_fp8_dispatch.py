"""FP8 dispatch with the torch cast vs the HIP cast kernel in front (BASELINE config 4's shape at EP = 1),
one JSON line.

  A  workloads.per_token_cast_to_fp8(x) on the GPU (eager torch kernels), then dispatch((q, sf), do_expand=True)
  B  deepep_amd.per_token_cast_to_fp8(x) (one HIP kernel, deepep_cast_fp8), then the same dispatch
  C  dispatch(x, cast_to_fp8=True, do_expand=True): the cast inside the dispatch's own copy kernel
  D  dispatch(x, cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True, do_expand=True): C with power-of-two
     scale factors packed as UE8M0 exponent bytes, int32 [rows, H / 512] (a quarter of C's scale-factor bytes, the
     same row traffic); compared with C of the same run, against C's same-route spread

All in one process on the same inputs, alternating round by round after a warm-up, each round timed with
device events around `--iters` calls; fresh dispatches (one host sync each, as bench.py's) and cached-handle
dispatches (kernels only).  C is timed twice per round (`*_C` and `*_C_again`): the difference of the two
medians is the session's same-route spread.  Reported per variant: median and minimum of the rounds' per-call
times, B / A and C / B of the medians; the stand-alone cast kernel (deepep_cast_fp8) alone: time and GB/s over
the bytes it must move, T * H * 3 + T * H / 128 * 4; and the cast back of the [T, H] pair,
deepep_amd.per_token_cast_back (deepep_cast_back_fp8, timed twice per round) against
workloads.per_token_cast_back on the GPU (eager torch kernels), over the same bytes; the packed cast
(deepep_cast_fp8_ue8m0) beside the round_scale cast, and the packed cast back (deepep_cast_back_fp8_ue8m0, on D's
pair) beside the fp32 one.  Before timing, D's output is checked bitwise against the tuple dispatch of the round_scale
pair with its factors packed by torch, and the packed cast back against the fp32 cast back of that pair.  B's and
C's outputs are checked bitwise against the dispatch of the pair the same torch code gives on the CPU (the
cast's contract) and the cast back against the torch code on the CPU; how many of A's own bytes (eager GPU
kernels) differ from the CPU's is reported."""
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
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fp8_dispatch needs a GPU'
    torch.cuda.set_device(0)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29643')
    dist.init_process_group('gloo', rank=0, world_size=1)
    from deepep_amd import ElasticBuffer, per_token_cast_back as hip_cast_back, per_token_cast_to_fp8 as hip_cast
    from workloads import per_token_cast_back, per_token_cast_to_fp8
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    torch.manual_seed(0)
    scores = torch.rand((T, E), device='cuda')
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    idx = idx.to(torch.int64)
    x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    buf = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    fresh = dict(topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)

    # B against the contract: the dispatch of the pair the torch restatement gives on the CPU, bitwise
    q_cpu, sf_cpu = per_token_cast_to_fp8(x.cpu())
    q_cpu, sf_cpu = q_cpu.cuda(), sf_cpu.cuda()
    ref = buf.dispatch((q_cpu, sf_cpu), **fresh)
    got = buf.dispatch(hip_cast(x), **fresh)
    got_c = buf.dispatch(x, cast_to_fp8=True, **fresh)
    torch.cuda.synchronize()

    def same_as_ref(r):
        return (torch.equal(ref[0][0].view(torch.uint8), r[0][0].view(torch.uint8)) and torch.equal(ref[0][1], r[0][1])
                and torch.equal(ref[2], r[2]) and torch.equal(ref[3].recv_src_metadata, r[3].recv_src_metadata))

    same, same_c = same_as_ref(got), same_as_ref(got_c)
    assert same, 'the dispatch of the HIP-cast pair differs from the dispatch of the CPU-cast pair'
    assert same_c, 'dispatch(x, cast_to_fp8=True) differs from the dispatch of the CPU-cast pair'
    back_same = torch.equal(hip_cast_back(q_cpu, sf_cpu).view(torch.int16).cpu(),
                            per_token_cast_back(q_cpu.cpu(), sf_cpu.cpu()).view(torch.int16))
    assert back_same, 'per_token_cast_back differs from the torch code on the CPU'
    # A's own cast (the same torch code run by eager GPU kernels) need not give the CPU's bits: how far it is
    q_gpu, sf_gpu = per_token_cast_to_fp8(x)
    a_q_diff = (q_gpu.view(torch.uint8) != q_cpu.view(torch.uint8)).float().mean().item()
    a_sf_diff = (sf_gpu.view(torch.int32) != sf_cpu.view(torch.int32)).float().mean().item()
    # D against the tuple dispatch of (round_scale q, its factors' exponent bytes packed four to an int32 by torch)
    q_rs, sf_rs = hip_cast(x, round_scale=True)
    sf_packed = ((sf_rs.view(torch.int32) >> 23) & 0xff).to(torch.uint8).view(torch.int32)
    ue8m0 = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True)
    ref_d = buf.dispatch((q_rs, sf_packed), **fresh)
    got_d = buf.dispatch(x, **ue8m0, **fresh)
    same_d = (torch.equal(ref_d[0][0].view(torch.uint8), got_d[0][0].view(torch.uint8)) and
              got_d[0][1].dtype == torch.int32 and torch.equal(ref_d[0][1], got_d[0][1]) and
              torch.equal(ref_d[2], got_d[2]) and torch.equal(ref_d[3].recv_src_metadata, got_d[3].recv_src_metadata))
    assert same_d, 'dispatch(x, ..., fp8_use_ue8m0=True) differs from the dispatch of the packed round_scale pair'
    back_packed_same = torch.equal(hip_cast_back(q_rs, sf_packed).view(torch.int16),
                                   hip_cast_back(q_rs, sf_rs).view(torch.int16))
    assert back_packed_same, 'the packed cast back differs from the fp32 cast back'
    del ref, got_c, q_gpu, sf_gpu, ref_d, got_d
    handle = got[3]
    cached = dict(handle=handle, topk_weights=w, do_expand=True)
    q = torch.empty((T, H), dtype=torch.float8_e4m3fn, device='cuda')
    sf = torch.empty((T, H // 128), dtype=torch.float32, device='cuda')
    sf32 = torch.empty((T, H // 512), dtype=torch.int32, device='cuda')
    variants = {
        'fresh_A': lambda: buf.dispatch(per_token_cast_to_fp8(x), **fresh),
        'fresh_B': lambda: buf.dispatch(hip_cast(x), **fresh),
        'cached_A': lambda: buf.dispatch(per_token_cast_to_fp8(x), **cached),
        'cached_B': lambda: buf.dispatch(hip_cast(x), **cached),
        'fresh_C': lambda: buf.dispatch(x, cast_to_fp8=True, **fresh),
        'cached_C': lambda: buf.dispatch(x, cast_to_fp8=True, **cached),
        'fresh_C_again': lambda: buf.dispatch(x, cast_to_fp8=True, **fresh),
        'cached_C_again': lambda: buf.dispatch(x, cast_to_fp8=True, **cached),
        'fresh_D': lambda: buf.dispatch(x, **ue8m0, **fresh),
        'cached_D': lambda: buf.dispatch(x, **ue8m0, **cached),
        'torch_cast': lambda: per_token_cast_to_fp8(x),
        'cast_kernel': lambda: buf.kernels.cast_fp8(x, q, sf),
        'torch_cast_back': lambda: per_token_cast_back(q_cpu, sf_cpu),
        'cast_back_kernel': lambda: hip_cast_back(q_cpu, sf_cpu),
        'cast_back_kernel_again': lambda: hip_cast_back(q_cpu, sf_cpu),
        'cast_kernel_round_scale': lambda: buf.kernels.cast_fp8(x, q, sf, True),
        'cast_kernel_ue8m0': lambda: buf.kernels.cast_fp8(x, q, sf32, True, ue8m0=True),
        'cast_back_kernel_round_scale': lambda: hip_cast_back(q_rs, sf_rs),
        'cast_back_kernel_ue8m0': lambda: hip_cast_back(q_rs, sf_packed),
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
    cast_bytes = T * H * 3 + T * H // 128 * 4
    out = dict(tool='bench_fp8_dispatch', device=torch.cuda.get_device_name(0), tokens=T, hidden=H, topk=K, experts=E,
               expanded_rows=int(handle.num_expanded_tokens), rounds=args.rounds, iters=args.iters, B_bitwise_equal_to_cpu_cast=same,
               C_bitwise_equal_to_cpu_cast=same_c, cast_back_bitwise_equal_to_cpu=back_same,
               A_gpu_cast_q_bytes_differing=a_q_diff, A_gpu_cast_sf_differing=a_sf_diff,
               D_bitwise_equal_to_packed_pair_dispatch=same_d, packed_cast_back_bitwise_equal_to_fp32=back_packed_same)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 1)
        out[f'{name}_us_min'] = round(min(v), 1)
    out['fresh_B_over_A'] = round(med['fresh_B'] / med['fresh_A'], 4)
    out['cached_B_over_A'] = round(med['cached_B'] / med['cached_A'], 4)
    for kind in ('fresh', 'cached'):
        out[f'{kind}_C_over_B'] = round(med[f'{kind}_C'] / med[f'{kind}_B'], 4)
        out[f'{kind}_C_minus_B_us'] = round(med[f'{kind}_C'] - med[f'{kind}_B'], 1)
        out[f'{kind}_C_same_route_spread_us'] = round(abs(med[f'{kind}_C'] - med[f'{kind}_C_again']), 1)
        out[f'{kind}_D_over_C'] = round(med[f'{kind}_D'] / med[f'{kind}_C'], 4)
        out[f'{kind}_D_minus_C_us'] = round(med[f'{kind}_D'] - med[f'{kind}_C'], 1)
    out['cast_kernel_ue8m0_minus_round_scale_us'] = round(med['cast_kernel_ue8m0'] - med['cast_kernel_round_scale'], 1)
    out['cast_back_kernel_ue8m0_minus_round_scale_us'] = round(med['cast_back_kernel_ue8m0'] -
                                                              med['cast_back_kernel_round_scale'], 1)
    out['cast_back_kernel_gbps'] = round(cast_bytes / (med['cast_back_kernel'] * 1e-6) / 1e9, 1)
    out['torch_cast_back_gbps_same_bytes'] = round(cast_bytes / (med['torch_cast_back'] * 1e-6) / 1e9, 1)
    out['cast_back_same_route_spread_us'] = round(abs(med['cast_back_kernel'] - med['cast_back_kernel_again']), 1)
    out['cast_back_kernel_over_torch'] = round(med['cast_back_kernel'] / med['torch_cast_back'], 4)
    out['cast_kernel_bytes'] = cast_bytes
    out['cast_kernel_gbps'] = round(cast_bytes / (med['cast_kernel'] * 1e-6) / 1e9, 1)
    out['torch_cast_gbps_same_bytes'] = round(cast_bytes / (med['torch_cast'] * 1e-6) / 1e9, 1)
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
