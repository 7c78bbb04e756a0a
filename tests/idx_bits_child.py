"""One process that runs buffer cases under the EP_NUM_TOPK_IDX_BITS it was started with -- TEST
INFRASTRUCTURE ONLY (not collected by pytest; run as `python -m tests.idx_bits_child --case NAME`).

deep_ep.topk_idx_t is fixed when deepep_amd is imported, so the 32-bit mode needs a fresh process:
tests/test_idx_bits_cpu.py and tests/test_idx_bits_gpu.py start this module with
EP_NUM_TOPK_IDX_BITS=32 (`run_child` below), one child at a time, and read the one JSON line it
prints: {"topk_idx_t": "torch.int32", "failures": [...], "seconds": {case: s}}.  A run in which the
variable did not take effect reports torch.int64 and is rejected by the parent.

--case takes one name or several separated by commas (one start-up for all of them):
  ep1                 EP = 1 at T=129, H=520, K=3, E=9, num_max_tokens_per_rank = T + 7: both dispatch
                      layouts fresh, cached and without a CPU sync, every combine flavour, all bitwise
                      against the 64-bit oracle (any device);
  golden_ep1/4/8      tests/test_combine_gpu.py::_buffer_case over the golden fixtures F1 / F4 / F2,
                      thread ranks on the one GPU (tests/sim.py); golden_ep4_chunks3: F4 with
                      DEEPEP_COMBINE_CHUNKS=3;
  graph               cached expanded dispatch + combine captured into a HIP graph and replayed;
  reject              routing of the other width is refused (any device).
--device cpu runs a case on the CPU with the oracle stand-in (tests/oracle_kernels.py).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CASES = {'golden_ep1': ('f1_ep1_t128_h1024_k2.npz', 1, 0), 'golden_ep4': ('f4_ep4_t96_h256_k2.npz', 4, 0),
                'golden_ep8': ('f2_ep8_t64_h256_k8.npz', 8, 0), 'golden_ep4_chunks3': ('f4_ep4_t96_h256_k2.npz', 4, 3)}


def run_child(cases, bits='32', device=None, timeout=240):
    """Start one child for `cases` (a name or a list of names) with EP_NUM_TOPK_IDX_BITS=`bits` (None: unset)
    and return its report.  The child is a fresh process (never an exec over this one), is not retried, and
    must exit 0 with exactly one JSON line on stdout."""
    env = {k: v for k, v in os.environ.items() if k != 'EP_NUM_TOPK_IDX_BITS'}
    if bits is not None:
        env['EP_NUM_TOPK_IDX_BITS'] = bits
    cmd = [sys.executable, '-m', 'tests.idx_bits_child', '--case', cases if isinstance(cases, str) else ','.join(cases)]
    if device is not None:
        cmd += ['--device', device]
    if device == 'cpu':
        env.update(HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')      # the child opens no GPU
    proc = subprocess.run(cmd, cwd=ROOT, env=env, timeout=timeout, capture_output=True, text=True)
    assert proc.returncode == 0, f'child exited with {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}'
    lines = [line for line in proc.stdout.splitlines() if line.startswith('{')]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def _group():
    """A one-rank gloo group (what the EP = 1 tests of the suite use)."""
    import torch.distributed as dist
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    return dist.group.WORLD


def _buffer(device, **kw):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(_group(), **kw)
    if device == 'cpu':
        from tests.oracle_kernels import OracleKernels
        buf._kernels = OracleKernels()
    return buf


def _u16(t) -> np.ndarray:
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bf16(a: np.ndarray, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16).to(device)


def case_ep1(device):
    """T=129: two 128-row receive blocks, the second partial; H=520: a ragged row tail; K=3: T * K is
    odd, so routing read at the wrong width straddles rows; ~30 % of the entries -1 and one token
    routed nowhere; num_max_tokens_per_rank = T + 7.  Everything is bitwise against the oracle fed
    with the int64 routing."""
    import torch
    import oracle
    from deepep_amd import topk_idx_t
    from tests.test_buffer_cpu import _weighted_single
    T, H, K, E = 129, 520, 3, 9
    T_max = T + 7
    rng = np.random.default_rng(3200)
    idx = np.array([rng.permutation(E)[:K] for _ in range(T)], dtype=np.int64)
    idx[rng.random((T, K)) < 0.3] = -1
    idx[5] = -1                                               # a token routed nowhere
    w = (rng.random((T, K)).astype(np.float32) * (idx >= 0)).astype(np.float32)
    x_u16 = oracle.f32_to_bf16(rng.standard_normal((T, H)).astype(np.float32))
    biases = [oracle.f32_to_bf16(rng.standard_normal((T, H)).astype(np.float32)) for _ in range(2)]
    x = _bf16(x_u16, device)
    g_idx = torch.from_numpy(idx).to(topk_idx_t).to(device)
    g_w = torch.from_numpy(w).to(device)
    fails = []

    def sync():
        if device != 'cpu':
            torch.cuda.synchronize()

    def check(ok, what):
        if not ok:
            fails.append(what)

    # ---- the 64-bit oracle's dispatch: received rows in source order, the expanded layout
    disp = oracle.simulate_dispatch([idx], E, T_max)[0]
    meta_ref = disp['src_metadata']
    tok = meta_ref[:, 0] % T_max                               # EP = 1: the source token of every received row
    n = meta_ref.shape[0]
    assert n < T
    n_exp = disp['num_expanded']
    exp_tok, exp_k = disp['expanded_src'][:, 0] % T_max, disp['expanded_src'][:, 1]

    def check_recv(tag, out, cached_w=True):
        rx, ri, rw, h = out[:4]
        rows = rx.shape[0]
        check(ri.dtype == topk_idx_t and h.topk_idx.dtype == topk_idx_t,
              f'{tag}: recv_topk_idx {ri.dtype} / handle.topk_idx {h.topk_idx.dtype} != {topk_idx_t}')
        check(np.array_equal(ri.cpu().numpy()[:n], idx[tok]), f'{tag}: recv_topk_idx != oracle')
        check(bool((ri[n:] == -1).all()), f'{tag}: recv_topk_idx past the received rows')
        check(np.array_equal(_u16(rx)[:n], x_u16[tok]) and rows == ri.shape[0], f'{tag}: recv_x != oracle')
        if cached_w:
            check(np.array_equal(rw.cpu().numpy()[:n], w[tok]), f'{tag}: recv_topk_weights != oracle')
        m = h.recv_src_metadata.cpu().numpy()
        check(np.array_equal(m[:n, :2], meta_ref[:, :2]) and bool((m[:n, 2:] == -1).all()) and bool((m[n:] == -1).all()),
              f'{tag}: recv_src_metadata != oracle')
        return rows

    def check_expanded(tag, out):
        ex, ei, ew, h = out[:4]
        check(ei is None and h.topk_idx.dtype == topk_idx_t, f'{tag}: recv_topk_idx / handle.topk_idx')
        check(np.array_equal(_u16(ex)[:n_exp], x_u16[exp_tok]), f'{tag}: expanded recv_x != oracle')
        check(np.array_equal(ew.cpu().numpy()[:n_exp], w[exp_tok, exp_k]), f'{tag}: expanded weights != oracle')
        m = h.recv_src_metadata.cpu().numpy()
        check(np.array_equal(m[:n], meta_ref) and bool((m[n:] == -1).all()), f'{tag}: expanded recv_src_metadata != oracle')

    def expanded_combines(tag, buf, amr, h, ex_w, rows):
        """Every expanded combine flavour over handle `h` (the oracle recipe of
        tests/test_fuzz_gpu.py::test_random_shapes_ep1): bias 0 and 2, plain and gating-weighted."""
        y = oracle.f32_to_bf16(rng.standard_normal((rows, H)).astype(np.float32))
        y3 = np.zeros((T, K, H), np.uint16)
        y3[exp_tok, exp_k] = y[:n_exp]
        ew = np.zeros((rows,), np.float32)
        ew[:n_exp] = w[exp_tok, exp_k]
        for nb in (0, 2):
            b = [biases[0] if nb else None, biases[1] if nb else None]
            g_bias = (_bf16(b[0], device), _bf16(b[1], device)) if nb else None
            for weighted in (False, True):
                out, out_w, _ = buf.combine(_bf16(y, device), h, topk_weights=ex_w if (weighted or amr) else None,
                                            bias=g_bias, apply_topk_weights=weighted)
                sync()
                if amr:
                    part, _ = oracle.phase_a(y, meta_ref, K, True, ew, weighted=weighted)
                    recv = np.zeros((1, T_max, H), np.uint16)
                    recv[0, tok] = part
                    exp, _ = oracle.phase_b(recv, None, idx, E, 1, True, True, b[0], b[1])
                elif weighted:
                    cb = tuple(torch.from_numpy(v.view(np.int16)).view(torch.bfloat16) for v in b) if nb else None
                    exp = _u16(_weighted_single(y3, torch.from_numpy(idx), torch.from_numpy(w), cb))
                else:
                    exp = oracle.combine_ep([y], [meta_ref], [idx], E, T_max, expanded=True,
                                            allow_multiple_reduction=False, bias_per_rank=[tuple(b)])[0][0][:T]
                check(np.array_equal(_u16(out), exp), f'{tag}: expanded combine amr={amr} b{nb} weighted={weighted}')
                check(out_w is None or np.array_equal(out_w.cpu().numpy(), w),
                      f'{tag}: expanded combined_topk_weights amr={amr} b{nb} weighted={weighted}')
                check(out_w is not None or not (weighted or amr), f'{tag}: no combined_topk_weights')

    def plain_combines(tag, buf, h, recv_w, rows):
        """The non-expanded combine (the caller pre-reduced its local experts): bias 0 and 2; its weight
        pass-through reads the routing on the device (the EP = 1 weight table)."""
        x_red = oracle.f32_to_bf16(rng.standard_normal((rows, H)).astype(np.float32))
        recv = np.zeros((1, T_max, H), np.uint16)
        recv[0, tok] = x_red[:n]
        for nb in (0, 2):
            b = [biases[0] if nb else None, biases[1] if nb else None]
            g_bias = (_bf16(b[0], device), _bf16(b[1], device)) if nb else None
            out, out_w, _ = buf.combine(_bf16(x_red, device), h, topk_weights=recv_w, bias=g_bias)
            sync()
            exp, _ = oracle.phase_b(recv, None, idx, E, 1, True, True, b[0], b[1])
            check(np.array_equal(_u16(out), exp), f'{tag}: non-expanded combine b{nb}')
            check(np.array_equal(out_w.cpu().numpy(), w), f'{tag}: non-expanded combined_topk_weights b{nb}')

    for amr in (True, False):
        buf = _buffer(device, num_max_tokens_per_rank=T_max, hidden=H, num_topk=K, allow_multiple_reduction=amr)
        check(buf.kernels.name == ('oracle' if device == 'cpu' else 'hip'), f'kernel provider {buf.kernels.name}')
        args = dict(topk_idx=g_idx, topk_weights=g_w, num_experts=E, num_max_tokens_per_rank=T_max)
        # ---- fresh and cached dispatch, both layouts
        fresh = buf.dispatch(x, **args)
        rows = check_recv(f'amr={amr} fresh', fresh)
        check(rows == n, f'amr={amr}: {rows} received rows, oracle {n}')
        # the handle holds the int64 routing the kernels read since its dispatch; later calls reuse it
        r64 = fresh[3].routing_idx64()
        check(r64.dtype == torch.int64 and r64.is_contiguous() and np.array_equal(r64.cpu().numpy(), idx) and
              (r64 is fresh[3].topk_idx) == (topk_idx_t == torch.int64), f'amr={amr}: the handle\'s int64 routing')
        seen, pack = [], buf.kernels.dispatch_pack
        buf.kernels.dispatch_pack = lambda *a, **k: (seen.append(a[2]), pack(*a, **k))[1]    # a[2]: topk_idx
        cached = buf.dispatch(x, topk_weights=g_w, handle=fresh[3])
        del buf.kernels.dispatch_pack
        check(len(seen) == 1 and seen[0] is r64 and fresh[3].routing_idx64() is r64,
              f'amr={amr}: a cached dispatch converted the routing again')
        check_recv(f'amr={amr} cached', cached)
        check(cached[3] is fresh[3] and torch.equal(cached[0], fresh[0]) and torch.equal(cached[1], fresh[1]) and
              torch.equal(cached[2], fresh[2]), f'amr={amr}: cached dispatch differs from the fresh one')
        ex = buf.dispatch(x, do_expand=True, **args)
        check_expanded(f'amr={amr} fresh', ex)
        check(ex[3].num_expanded_tokens == n_exp and ex[0].shape[0] == n_exp, f'amr={amr}: expanded rows')
        ex_c = buf.dispatch(x, topk_weights=g_w, do_expand=True, handle=ex[3])
        check_expanded(f'amr={amr} cached', ex_c)
        check(torch.equal(ex_c[0], ex[0]) and torch.equal(ex_c[2], ex[2]),
              f'amr={amr}: cached expanded dispatch differs from the fresh one')
        # ---- combine: expanded (plain / gating-weighted), non-expanded (the device-side routing read)
        expanded_combines(f'amr={amr}', buf, amr, ex[3], ex[2], n_exp)
        if amr:
            plain_combines(f'amr={amr}', buf, fresh[3], fresh[2], n)
            # ---- dispatch without a CPU sync (worst-case shapes), then combine
            free = buf.dispatch(x, do_cpu_sync=False, **args)
            rows = check_recv('no-CPU-sync', free)
            check(rows == T_max, f'no-CPU-sync: {rows} rows, worst case {T_max}')
            plain_combines('no-CPU-sync', buf, free[3], free[2], rows)
            free_c = buf.dispatch(x, topk_weights=g_w, handle=free[3])
            check(torch.equal(free_c[0], free[0]) and torch.equal(free_c[1], free[1]) and
                  free_c[1].dtype == topk_idx_t, 'no-CPU-sync: cached dispatch differs from the fresh one')
            ex_free = buf.dispatch(x, do_expand=True, do_cpu_sync=False, **args)
            check_expanded('no-CPU-sync', ex_free)
            expanded_combines('no-CPU-sync', buf, amr, ex_free[3], ex_free[2], ex_free[0].shape[0])
    return fails


def case_golden(name, device):
    """tests/test_combine_gpu.py::_buffer_case (the 64-bit suite's body) over a golden fixture."""
    assert device != 'cpu', 'the golden thread-rank cases run on the GPU (CPU: tests/test_idx_bits_cpu.py)'
    import threading
    import torch
    from tests.sim import ThreadComm
    from tests.test_combine_gpu import _buffer_case
    fixture, world, chunks = GOLDEN_CASES[name]
    saved = os.environ.get('DEEPEP_COMBINE_CHUNKS')
    if chunks:
        os.environ['DEEPEP_COMBINE_CHUNKS'] = str(chunks)       # read at every combine
    try:
        if world == 1:
            _group()
        torch.cuda.init()                                   # CUDA initialised here, not lazily by racing threads
        torch.cuda.get_device_properties(0)                 # (as tests/sim.py::run_threads)
        comm = ThreadComm(world) if world > 1 else None
        results = {}
        threads = [threading.Thread(target=_buffer_case, args=(r, world, fixture, comm, results)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
    finally:
        if chunks:
            os.environ.pop('DEEPEP_COMBINE_CHUNKS') if saved is None else os.environ.update(DEEPEP_COMBINE_CHUNKS=saved)
    fails = [f'rank {r}: {f}' for r, fs in sorted(results.items()) for f in fs]
    if len(results) != world:
        fails.append(f'{world - len(results)} of {world} ranks did not finish')
    return fails


def case_graph(device):
    """The recipe of tests/test_combine_gpu.py::test_hip_graph_cached_dispatch_and_combine at T=130,
    H=512, K=4, E=16: the handle holds the int64 routing, so the capture records no conversion that
    would break it, and the replay equals the eager call bitwise."""
    assert device != 'cpu', 'HIP graphs need the GPU'
    import torch
    import oracle
    from deepep_amd import topk_idx_t
    T, H, K, E = 130, 512, 4, 16
    _group()
    g = torch.Generator(device='cuda').manual_seed(5)
    scores = torch.rand((T, E), device='cuda', generator=g)
    w, idx = torch.topk(scores, K, dim=-1, sorted=False)
    idx = idx.to(topk_idx_t)
    idx[torch.rand(idx.shape, device='cuda', generator=g) < 0.1] = -1
    w = w.masked_fill(idx < 0, 0)
    buf = _buffer(device, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    x = torch.randn((T, H), device='cuda', generator=g).to(torch.bfloat16)
    _, _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    fails = []
    if handle.topk_idx.dtype != topk_idx_t:
        fails.append(f'handle.topk_idx is {handle.topk_idx.dtype}')

    def layer():
        ex_x, _, ex_w2, _, _ = buf.dispatch(x, topk_weights=w, do_expand=True, handle=handle)
        return buf.combine(ex_x, handle, topk_weights=ex_w2, apply_topk_weights=True)[:2]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            layer()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_w = layer()
    x.copy_(torch.randn(x.shape, device='cuda', generator=g).to(torch.bfloat16))
    graph.replay()
    ref, ref_w = layer()
    torch.cuda.synchronize()
    if not (torch.equal(out, ref) and torch.equal(out_w, ref_w)):
        fails.append('graph replay differs from the eager call')
    if not torch.equal(out_w, w):
        fails.append('combined_topk_weights != topk_weights')
    # the weighted sum of a token's own expanded copies: x scaled by the sum of its valid weights
    exact = x.double() * (w.double() * (idx >= 0)).sum(dim=1, keepdim=True)
    d = oracle.calc_diff(oracle.bf16_to_f32(_u16(out)), exact.cpu().numpy())
    if not d < 1e-5:
        fails.append(f'calc_diff {d} >= 1e-5')
    return fails


def case_reject(device):
    """Routing of the other width than deep_ep.topk_idx_t is refused by the dispatch's host assertion."""
    import torch
    from deepep_amd import topk_idx_t
    other = torch.int64 if topk_idx_t == torch.int32 else torch.int32
    T, H, K, E = 8, 64, 2, 4
    buf = _buffer(device, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    x = torch.zeros((T, H), dtype=torch.bfloat16, device=device)
    idx = (torch.arange(T * K, device=device).view(T, K) % E)
    fails = []
    try:
        buf.dispatch(x, topk_idx=idx.to(other), num_experts=E)
        fails.append(f'{other} routing was accepted with deep_ep.topk_idx_t = {topk_idx_t}')
    except RuntimeError as e:
        if 'deep_ep.topk_idx_t' not in str(e):
            fails.append(f'unexpected error: {e}')
    recv_idx = buf.dispatch(x, topk_idx=idx.to(topk_idx_t), num_experts=E)[1]
    if recv_idx.dtype != topk_idx_t or not torch.equal(recv_idx, idx.to(topk_idx_t)):
        fails.append('the routing of the right width was not dispatched')
    return fails


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', required=True)
    ap.add_argument('--device', default=None, choices=['cpu', 'cuda'])
    a = ap.parse_args()
    import torch
    import deepep_amd
    device = a.device or ('cuda' if torch.cuda.is_available() else 'cpu')
    failures, seconds = [], {}
    for name in a.case.split(','):
        t0 = time.perf_counter()
        try:
            if name in GOLDEN_CASES:
                fs = case_golden(name, device)
            else:
                fs = {'ep1': case_ep1, 'graph': case_graph, 'reject': case_reject}[name](device)
            if device != 'cpu':
                torch.cuda.synchronize()
        except Exception:
            # an exception may be a device fault: nothing more is started on the GPU in this process
            failures.append(f'{name}: {traceback.format_exc()}')
            break
        seconds[name] = round(time.perf_counter() - t0, 2)
        failures += [f'{name}: {f}' for f in fs]
    print(json.dumps({'topk_idx_t': str(deepep_amd.topk_idx_t), 'device': device, 'failures': failures,
                      'seconds': seconds}), flush=True)


if __name__ == '__main__':
    main()
