"""What combine(use_logfmt=True) adds on one GPU: the LogFMT-10 codec kernels, the LogFMT epilogue against the bf16
epilogue, and the whole EP = 4 / EP = 8 combine step with and without the flag -- one JSON line.

  codec      deepep_cast_logfmt, deepep_cast_back_logfmt and deepep_logfmt_pack_rows (top-8 weight tails) over
             --tokens x --hidden rows: microseconds and bytes moved per second (read + written, from the shapes)
  epilogue   phase B of one rank at EP = 8 with these inputs (the tokens of one rank, each reducing one row per rank
             that holds one of its experts): combine_reduce(MODE_EPILOGUE) over LogFMT wire rows against the same call
             over bf16 packed rows; the outputs are compared bitwise with the bf16 call over the cast-back rows first
             (--sweep: its launch shapes, vectors per lane {1, 2} x rows in flight {2, 4, 8}, through
             deepep_set_launch_config, beside the automatic shape)
  step       the whole combine of EP = 4 and EP = 8, ranks simulated by threads on the one GPU (tests/sim.py), bench.py's
             inputs, one chunk: the host time of --step-iters calls of every rank, device synchronised at both ends,
             per call, with and without use_logfmt

Ranks that share a GPU exchange through device copies, so `step` shows the added pack pass and the decode, not the
saving on the links: that is 0.646 of the bytes per row (handle.logfmt_row_layout against packed_row_layout) until a
node with 8 GPUs runs it.

Every route is timed twice per round (`X` and `X_again`), the rounds alternate between the routes in one process after
a warm-up, and the difference of a route's two medians is its spread in this session."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

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


def alternate(routes: dict, rounds: int, iters: int, warmup: int) -> dict:
    """{route: median us, route + '_again': median us, route + '_spread': |difference|}"""
    variants = dict(routes)
    variants.update({name + '_again': fn for name, fn in routes.items()})
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, iters))
    out = {name + '_us': round(statistics.median(v), 1) for name, v in times.items()}
    for name in routes:
        out[name + '_spread_us'] = round(abs(out[name + '_us'] - out[name + '_again_us']), 1)
    return out


def codec(kern, args) -> dict:
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    T, H, K = args.tokens, args.hidden, args.topk
    x = (torch.randn((T, H), device='cuda') * 0.1).to(torch.bfloat16)
    planes = torch.empty((T, H * 5 // 4), dtype=torch.uint8, device='cuda')
    meta = torch.empty((T, H // 128), dtype=torch.int32, device='cuda')
    back = torch.empty((T, H), dtype=torch.bfloat16, device='cuda')
    rb, w_off, _ = packed_row_layout(H, K, True)
    lb, lw_off, _ = logfmt_row_layout(H, K, True)
    packed = torch.zeros((T, rb // 2), dtype=torch.bfloat16, device='cuda')
    packed[:, :H] = x
    wire = torch.empty((T, lb), dtype=torch.uint8, device='cuda')
    routes = {'cast': lambda: kern.cast_logfmt(x, planes, meta),
              'cast_back': lambda: kern.cast_back_logfmt(planes, meta, back),
              'pack': lambda: kern.logfmt_pack_rows(packed, T, H, wire, src_tail_offset=w_off, dst_tail_offset=lw_off,
                                                    tail_bytes=lb - lw_off)}
    out = alternate(routes, args.rounds, args.iters, args.warmup)
    coded = H * 5 // 4 + H // 32
    nbytes = {'cast': T * (H * 2 + coded), 'cast_back': T * (coded + H * 2), 'pack': T * (H * 2 + coded + 2 * (lb - lw_off))}
    for name, n in nbytes.items():
        out[name + '_bytes'] = n
        out[name + '_TB_per_s'] = round(n / (out[name + '_us'] * 1e-6) / 1e12, 3)
    return out


def epilogue(kern, args) -> dict:
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    from deepep_amd.kernels import MODE_EPILOGUE
    T, H, K, E, R = args.tokens, args.hidden, args.topk, args.experts, 8
    g = torch.Generator(device='cuda').manual_seed(1)
    idx = torch.topk(torch.rand((T, E), device='cuda', generator=g), K, dim=-1, sorted=False)[1]
    on_rank = torch.zeros((T, R), dtype=torch.bool, device='cuda')
    on_rank.scatter_(1, idx // (E // R), True)
    flat = on_rank.t().reshape(-1)                               # rows in rank order, as the all-to-all delivers them
    rows = int(flat.sum())
    table = torch.full((R * T,), -1, dtype=torch.int32, device='cuda')
    table[flat] = torch.arange(rows, dtype=torch.int32, device='cuda')
    table = table.view(R, T).t().contiguous()                    # [T, R]: the rank layout of phase B
    rb, w_off, _ = packed_row_layout(H, K, True)
    lb, lw_off, _ = logfmt_row_layout(H, K, True)
    src = torch.zeros((rows, rb // 2), dtype=torch.bfloat16, device='cuda')
    src[:, :H] = (torch.randn((rows, H), device='cuda') * 0.1).to(torch.bfloat16)
    wire = torch.zeros((rows, lb), dtype=torch.uint8, device='cuda')
    kern.logfmt_pack_rows(src, rows, H, wire, src_tail_offset=w_off, dst_tail_offset=lw_off, tail_bytes=lb - lw_off)
    coded = H * 5 // 4
    planes, meta = wire[:, :coded], wire.view(torch.int32)[:, coded // 4:coded // 4 + H // 128]
    back = torch.zeros((rows, rb // 2), dtype=torch.bfloat16, device='cuda')
    tmp = torch.empty((rows, H), dtype=torch.bfloat16, device='cuda')
    kern.cast_back_logfmt(planes, meta, tmp)
    back[:, :H] = tmp
    del tmp
    bias = torch.randn((T, H), device='cuda').to(torch.bfloat16)
    out_a = torch.empty((T, H), dtype=torch.bfloat16, device='cuda')
    out_b = torch.empty((T, H), dtype=torch.bfloat16, device='cuda')

    def bf16(rows_, out):
        kern.combine_reduce(MODE_EPILOGUE, rows_[:, :H], out, T, table=table, bias0=bias)

    def logfmt(out):
        kern.combine_reduce(MODE_EPILOGUE, planes, out, T, table=table, bias0=bias, src_logfmt_meta=meta)

    bf16(back, out_a)
    logfmt(out_b)
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), 'the LogFMT epilogue differs from the bf16 one'
    res = alternate({'bf16_epilogue': lambda: bf16(src, out_a), 'logfmt_epilogue': lambda: logfmt(out_b)},
                    args.rounds, args.iters, args.warmup)
    res.update(tokens=T, source_rows=rows, bitwise_equal_to_the_bf16_epilogue_over_cast_back_rows=True,
               bf16_bytes=rows * H * 2 + 2 * T * H * 2, logfmt_bytes=rows * (coded + H // 32) + 2 * T * H * 2)
    res['logfmt_over_bf16'] = round(res['logfmt_epilogue_us'] / res['bf16_epilogue_us'], 4)
    if args.sweep:
        # the LogFMT epilogue's launch shapes through the diagnostics knob, beside the automatic one (twice)
        def measure():
            for _ in range(args.warmup):
                logfmt(out_b)
            return round(statistics.median(timed(lambda: logfmt(out_b), args.iters) for _ in range(5)), 1)
        sweep = {'auto_us': measure()}
        try:
            for vpt in (1, 2):
                for rif in (2, 4, 8):
                    assert kern.lib.deepep_set_launch_config(vpt, rif) == 0
                    sweep[f'vpt{vpt}_rows{rif}_us'] = measure()
        finally:
            assert kern.lib.deepep_set_launch_config(0, 0) == 0
        sweep['auto_again_us'] = measure()
        res['sweep'] = sweep
    return res


def step(world: int, args) -> dict:
    from deepep_amd import ElasticBuffer
    from tests.sim import FakeGroup, ThreadComm
    T, H, K, E = args.tokens, args.hidden, args.topk, args.experts
    comm = ThreadComm(world)
    lock = threading.Lock()
    order = ['bf16', 'logfmt', 'bf16_again', 'logfmt_again']
    times = {name: [] for name in order}
    errors = []

    def rank_fn(rank):
        try:
            torch.cuda.set_device(0)
            with lock:                                   # bench.py's inputs: torch.manual_seed(0 + rank)
                torch.manual_seed(rank)
                scores = torch.rand((T, E), device='cuda')
                x = torch.randn((T, H), device='cuda').to(torch.bfloat16)
            w, idx = torch.topk(scores, K, dim=-1, sorted=False)
            buf = ElasticBuffer(FakeGroup(rank, world, comm), num_max_tokens_per_rank=T, hidden=H, num_topk=K)
            comm.install(buf, rank)
            ex_x, _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx.to(torch.int64), topk_weights=w, num_experts=E,
                                                    do_expand=True)
            y = (torch.randn(ex_x.shape, device='cuda') * 0.1).to(torch.bfloat16)
            del ex_x, x

            def call(flag):
                buf.combine(y, handle, topk_weights=ex_w, apply_topk_weights=True, use_logfmt=flag)

            for flag in (False, True):
                for _ in range(args.warmup):
                    call(flag)
            for _ in range(args.step_rounds):
                for name in order:
                    torch.cuda.synchronize()
                    comm.bar.wait()
                    t0 = time.perf_counter()
                    for _ in range(args.step_iters):
                        call(name.startswith('logfmt'))
                    torch.cuda.synchronize()
                    comm.bar.wait()
                    if rank == 0:
                        times[name].append((time.perf_counter() - t0) * 1e6 / args.step_iters)
        except Exception:
            import traceback
            errors.append(traceback.format_exc())
            comm.bar.abort()

    threads = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise RuntimeError(errors[0])
    out = {name + '_us': round(statistics.median(v), 1) for name, v in times.items()}
    for name in ('bf16', 'logfmt'):
        out[name + '_spread_us'] = round(abs(out[name + '_us'] - out[name + '_again_us']), 1)
    out['logfmt_over_bf16'] = round(out['logfmt_us'] / out['bf16_us'], 4)
    out['what'] = f'host time per combine call of all {world} thread ranks on one GPU, device synchronised at both ends'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tokens', type=int, default=8192)
    ap.add_argument('--hidden', type=int, default=7168)
    ap.add_argument('--topk', type=int, default=8)
    ap.add_argument('--experts', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step-rounds', type=int, default=5)
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--worlds', type=int, nargs='*', default=[4, 8])
    ap.add_argument('--sweep', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_logfmt_combine needs a GPU'
    torch.cuda.set_device(0)
    os.environ['DEEPEP_COMBINE_CHUNKS'] = '1'
    os.environ['DEEPEP_TRANSPORT'] = 'rccl'
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    from deepep_amd.kernels import HipKernels
    kern = HipKernels()
    out = dict(tool='bench_logfmt_combine', device=torch.cuda.get_device_name(0), tokens=args.tokens,
               hidden=args.hidden, topk=args.topk, experts=args.experts, rounds=args.rounds, iters=args.iters,
               wire_row_bytes=logfmt_row_layout(args.hidden, args.topk, True)[0],
               bf16_row_bytes=packed_row_layout(args.hidden, args.topk, True)[0])
    out['wire_over_bf16_row_bytes'] = round(out['wire_row_bytes'] / out['bf16_row_bytes'], 4)
    out['codec'] = codec(kern, args)
    torch.cuda.empty_cache()
    out['epilogue_ep8_phase_b'] = epilogue(kern, args)
    torch.cuda.empty_cache()
    for world in args.worlds:
        out[f'step_ep{world}'] = step(world, args)
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
