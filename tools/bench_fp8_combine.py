"""The combine over FP8 expert rows against the cast back in front of the bf16 combine (BASELINE config 2's shape at
EP = 1: T = 8192, H = 7168, K = 8, 65,536 expanded rows), one JSON line.

  A   combine(y, handle, topk_weights=w) over bf16 rows y that already exist (the cast-back rows, made once)
  B   y = deepep_amd.per_token_cast_back(q, sf); combine(y, ...) -- what a caller holding the pair does without this
  C   combine((q, sf), handle, topk_weights=w): fp32 scale factors, the cast back in the combine kernel's registers
  C'  combine((q, sf_packed), ...): the same with packed UE8M0 factors (`Cp` in the output)

All in one process on the same inputs, alternating round by round after a warm-up, each round timed with device
events around `--iters` calls.  Every route is timed twice per round (`X` and `X_again`): the difference of the two
medians is that route's own spread in this session.  Reported: median and minimum per route, C - B against the larger
of the two spreads, C / A, and C's and C''s fraction of 8 TB/s over their own algorithmic bytes per token,
K * H + K * H / 128 * 4 (packed: K * H / 128) + H * 2 + K * 8.  Before timing, C's and C''s outputs are compared
bitwise with the bf16 route over the cast-back rows of the same pair.

--sweep: the launch shapes of the FP8 source -- vectors per lane {1, 2} x rows in flight {2, 4, 8} x waves per
workgroup {4, 8}, driven through deepep_set_launch_config and units_per_block at the kernel level -- for the FUSED
reduce of this shape and for phase A (LOCAL into packed send rows with the weight tail) at the shape one rank of
EP = 8 sees with these inputs (the tokens of 8 ranks routed to the experts of rank 0), each beside the automatic
shape and the bf16 kernel over the cast-back rows."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8e12


def timed(fn, iters: int) -> float:
    """Microseconds per call of fn over `iters` back-to-back calls (device events)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def same_bits(a, b) -> bool:
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def phase_a_shape(T, K, E, ranks, H, device):
    """Rank 0's phase A at EP = `ranks`: (slot table [units, K], expanded rows) for ranks * T tokens routed by
    random top-K scores, units = the tokens with an expert on rank 0, slots in expert order."""
    g = torch.Generator(device=device).manual_seed(1)
    scores = torch.rand((ranks * T, E), device=device, generator=g)
    idx = torch.topk(scores, K, dim=-1, sorted=False)[1]
    local = idx < E // ranks
    units = local.any(dim=1).nonzero().view(-1)
    idx_u, local_u = idx[units], local[units]
    flat = local_u.view(-1).nonzero().view(-1)                   # (unit, lane) pairs on rank 0
    order = torch.argsort(idx_u.view(-1)[flat], stable=True)     # expert-major slots
    table = torch.full((units.numel() * K,), -1, dtype=torch.int32, device=device)
    table[flat[order]] = torch.arange(flat.numel(), dtype=torch.int32, device=device)
    return table.view(-1, K), int(flat.numel())


def sweep(kern, args):
    from deepep_amd import per_token_cast_back, per_token_cast_to_fp8
    from deepep_amd.handle import packed_row_layout
    from deepep_amd.kernels import MODE_FUSED, MODE_LOCAL
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    dev = torch.device('cuda')
    out = {}
    # FUSED: every token's K expanded rows, expert-major slots
    g = torch.Generator(device=dev).manual_seed(2)
    fused_table = torch.randperm(T * K, device=dev, generator=g).to(torch.int32).view(T, K)
    local_table, local_rows = phase_a_shape(T, K, E, 8, H, dev)
    for label, mode, table, rows in (('fused', MODE_FUSED, fused_table, T * K),
                                     ('phase_a_ep8', MODE_LOCAL, local_table, local_rows)):
        y = torch.randn((rows, H), device=dev).to(torch.bfloat16)
        q, sf = per_token_cast_to_fp8(y)
        y = per_token_cast_back(q, sf)
        w = torch.rand((rows,), device=dev)
        units = table.shape[0]
        if mode == MODE_LOCAL:
            row_bytes, w_off, w_pad = packed_row_layout(H, K, True)
            buf_rows = torch.empty((units, row_bytes // 2), dtype=torch.bfloat16, device=dev)
            dst = buf_rows[:, :H]
            ow = buf_rows.view(torch.float32)[:, w_off // 4:w_off // 4 + K]
        else:
            dst = torch.empty((units, H), dtype=torch.bfloat16, device=dev)
            ow = torch.empty((units, K), dtype=torch.float32, device=dev)
            w_pad = 0

        def call(src, upb=0, **kw):
            kern.combine_reduce(mode, src, dst, units, table=table, wtable=table, wsrc=w, out_weights=ow,
                                weights_pad=w_pad, units_per_block=upb, **kw)

        def measure(fn):
            for _ in range(3):
                fn()
            return round(statistics.median(timed(fn, args.sweep_iters) for _ in range(args.sweep_rounds)), 1)

        res = dict(units=units, rows=rows, bf16_auto_us=measure(lambda: call(y)),
                   fp8_auto_us=measure(lambda: call(q, src_sf=sf)))
        try:
            for vpt in (1, 2):
                for rif in (2, 4, 8):
                    assert kern.lib.deepep_set_launch_config(vpt, rif) == 0
                    for waves in (4, 8):
                        res[f'fp8_vpt{vpt}_rows{rif}_waves{waves}_us'] = measure(lambda: call(q, waves, src_sf=sf))
        finally:
            assert kern.lib.deepep_set_launch_config(0, 0) == 0
        res['bf16_auto_again_us'] = measure(lambda: call(y))
        res['fp8_auto_again_us'] = measure(lambda: call(q, src_sf=sf))
        out[label] = res
        del y, q, sf, dst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tokens', type=int, default=8192)
    ap.add_argument('--hidden', type=int, default=7168)
    ap.add_argument('--topk', type=int, default=8)
    ap.add_argument('--experts', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--sweep-rounds', type=int, default=5)
    ap.add_argument('--sweep-iters', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fp8_combine needs a GPU'
    torch.cuda.set_device(0)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29644')
    dist.init_process_group('gloo', rank=0, world_size=1)
    from deepep_amd import ElasticBuffer, per_token_cast_back, per_token_cast_to_fp8
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    torch.manual_seed(0)
    scores = torch.rand((T, E), device='cuda')
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    idx = idx.to(torch.int64)
    x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    buf = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    rows = recv_x.shape[0]
    del recv_x, x
    # the expert rows: every expanded row its own values, held as an FP8 pair in both scale-factor forms
    src = torch.randn((rows, H), device='cuda').to(torch.bfloat16)
    q, sf = per_token_cast_to_fp8(src)
    q_rs, sf_packed = per_token_cast_to_fp8(src, round_scale=True, use_ue8m0=True)
    del src
    y, y_rs = per_token_cast_back(q, sf), per_token_cast_back(q_rs, sf_packed)

    def combine(xin):
        return buf.combine(xin, handle, topk_weights=recv_w)

    ref, ref_rs = combine(y), combine(y_rs)
    got, got_p = combine((q, sf)), combine((q_rs, sf_packed))
    torch.cuda.synchronize()
    same_c = same_bits(got[0], ref[0]) and torch.equal(got[1], ref[1])
    same_cp = same_bits(got_p[0], ref_rs[0]) and torch.equal(got_p[1], ref_rs[1])
    assert same_c, 'combine((q, sf)) differs from the combine of the cast-back rows'
    assert same_cp, 'combine((q, packed sf)) differs from the combine of the cast-back rows'
    assert bool(torch.isfinite(ref[0].float()).all())
    del ref, ref_rs, got, got_p, y_rs
    routes = {'A': lambda: combine(y), 'B': lambda: combine(per_token_cast_back(q, sf)),
              'C': lambda: combine((q, sf)), 'Cp': lambda: combine((q_rs, sf_packed))}
    variants = {}
    for name, fn in routes.items():
        variants[name] = fn
    for name, fn in routes.items():
        variants[name + '_again'] = fn
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():                # alternating: one round of each, then the next round
            times[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in times.items()}
    out = dict(tool='bench_fp8_combine', device=torch.cuda.get_device_name(0), tokens=T, hidden=H, topk=K, experts=E,
               expanded_rows=rows, rounds=args.rounds, iters=args.iters, C_bitwise_equal_to_cast_back_route=same_c,
               Cp_bitwise_equal_to_cast_back_route=same_cp)
    for name, v in times.items():
        out[f'{name}_us_median'] = round(med[name], 1)
        out[f'{name}_us_min'] = round(min(v), 1)
    spread = {name: abs(med[name] - med[name + '_again']) for name in routes}
    for name in routes:
        out[f'{name}_same_route_spread_us'] = round(spread[name], 1)
    out['C_minus_B_us'] = round(med['C'] - med['B'], 1)
    out['C_below_B_by_more_than_both_spreads'] = bool(med['B'] - med['C'] > max(spread['B'], spread['C']))
    out['C_over_B'] = round(med['C'] / med['B'], 4)
    out['C_over_A'] = round(med['C'] / med['A'], 4)
    out['Cp_over_A'] = round(med['Cp'] / med['A'], 4)
    out['Cp_minus_C_us'] = round(med['Cp'] - med['C'], 1)
    bytes_a = T * (K * H * 2 + H * 2 + K * 8)
    bytes_c = T * (K * H + K * H // 128 * 4 + H * 2 + K * 8)
    bytes_cp = T * (K * H + K * H // 128 + H * 2 + K * 8)
    out['algorithmic_bytes_per_token'] = dict(A=bytes_a // T, C=bytes_c // T, Cp=bytes_cp // T)
    out['byte_ratio_C_over_A'] = round(bytes_c / bytes_a, 4)
    for name, nbytes in (('A', bytes_a), ('C', bytes_c), ('Cp', bytes_cp)):
        out[f'{name}_fraction_of_8TBps'] = round(nbytes / (med[name] * 1e-6) / PEAK_BYTES_PER_S, 4)
    if args.sweep:
        del y
        out['sweep'] = sweep(buf.kernels, args)
    print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
