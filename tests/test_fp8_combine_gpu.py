"""FP8 expert rows into the combine, on the GPU: combine((x_fp8, x_scales), handle, ...) and
HipKernels.combine_reduce(..., src_sf=...) return, bit for bit (signed zeros count), what the same build's bf16 route
returns over per_token_cast_back of the same pair -- at the kernel level in every mode, shape class and scale-factor
form, through the public combine at EP = 1, over 4 thread ranks and over xGMI windows in two processes.  The bf16
route is itself pinned to the torch code by tests/test_cast_back_gpu.py and to the oracle by the golden tests.  Every
expected result is asserted free of NaN and Inf: the inputs hold finite bytes only."""
import os
import sys
import threading
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from tests.fp8_combine_ref import (binade_rows, bits, byte_sweep_pair, col_major, combine_differences,
                                   pair_combine_cases, pair_forms, routed_inputs, same_bits)
from tests.fp8_oracle_kernels import Spy
from tests.test_cast_keyword_gpu import _free_port, _group1
from tests.ue8m0_ref import pack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MODE_LOCAL, MODE_EPILOGUE, MODE_FUSED = 0, 1, 2
POISON = 0x7b7b                                        # bf16 bits no result below produces by accident
UNITS, SRC_ROWS = 33, 301                              # 33 units: more than one workgroup at every shape


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


def _back(q, sf):
    import deepep_amd
    return deepep_amd.per_token_cast_back(q, sf)


_PAIRS = {}


def _pairs(H: int):
    """The three forms of SRC_ROWS cast rows of H columns, and their cast-back rows (computed once per H)."""
    if H not in _PAIRS:
        forms = pair_forms(binade_rows(SRC_ROWS, H, H), 'cuda')
        _PAIRS[H] = {name: (pair, _back(*pair)) for name, pair in forms.items()}
        torch.cuda.synchronize()
    return _PAIRS[H]


def _table(width: int, seed: int, rows: int = SRC_ROWS) -> torch.Tensor:
    """[UNITS, width] slots: random rows, a fifth masked, unit 5 without a valid slot, unit 7 with one."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, rows, (UNITS, width), generator=g, dtype=torch.int32)
    t[torch.rand((UNITS, width), generator=g) < 0.2] = -1
    t[5] = -1
    t[7] = -1
    t[7, width - 1] = 11
    return t.cuda()


def _poisoned(rows: int, H: int) -> torch.Tensor:
    return torch.full((rows, H), POISON, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _reduce_both(kern, mode, pair, y, table, H, weighted=False, biases=0, weights=False, pad=0, seed=0, flag=False):
    """The pair call and the same call on the cast-back rows y, outputs pre-filled with poison (three rows more than
    there are units: rows that must not be written are seen).  Returns what differs."""
    g = torch.Generator().manual_seed(seed)
    q, sf = pair
    row_w = torch.rand((q.shape[0],), generator=g).cuda() if weighted or weights else None
    bias = [torch.randn((UNITS, H), generator=g).to(torch.bfloat16).cuda() for _ in range(biases)] + [None, None]
    outs = []
    for src, kw in ((q, dict(src_sf=sf)), (y, dict())):
        out = _poisoned(UNITS + 3, H)
        ow = torch.full((UNITS + 3, max(pad, table.shape[1])), -7.0, device='cuda') if weights else None
        err = torch.zeros((8,), dtype=torch.int32, device='cuda') if flag else None
        kern.combine_reduce(mode, src, out, UNITS, table=table, row_weights=row_w if weighted else None,
                            bias0=bias[0], bias1=bias[1], wtable=table if weights else None,
                            wsrc=row_w if weights else None,
                            out_weights=ow[:, :table.shape[1]] if weights else None, weights_pad=pad,
                            error_flag=err, **kw)
        outs.append((out, ow, err))
    torch.cuda.synchronize()
    (a, aw, ae), (b, bw, be) = outs
    assert bool(torch.isfinite(b[:UNITS].float()).all()), 'wrongly chosen input: the bf16 route gives NaN / Inf'
    assert bool((bits(b[UNITS:]) == POISON).all())
    bad = []
    if not same_bits(a, b):
        bad.append('rows')
    if weights and not same_bits(aw, bw):
        bad.append('weights')
    if flag and not torch.equal(ae.cpu(), be.cpu()):
        bad.append('error record')
    return bad


# ----------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize('width', [1, 2, 3, 8, 9])     # the row copy; the -0 start; past one load group (2 / 4 / 8)
@pytest.mark.parametrize('H', [128, 512, 1152, 7168])  # one group; the packed minimum; chunks + one group; config 2
def test_reduce_equals_cast_back_route(kern, H, width):
    table = _table(width, H + width)
    fails = []
    for form, (pair, y) in _pairs(H).items():
        for mode, biases in ((MODE_FUSED, 0), (MODE_FUSED, 2), (MODE_EPILOGUE, 0), (MODE_EPILOGUE, 1),
                             (MODE_EPILOGUE, 2), (MODE_LOCAL, 0)):
            for weighted in (False, True):
                bad = _reduce_both(kern, mode, pair, y, table, H, weighted=weighted, biases=biases, seed=width)
                if bad:
                    fails.append((form, mode, biases, weighted, bad))
    assert sorted(_pairs(H)) == (['col_major', 'fp32', 'ue8m0'] if H % 512 == 0 else ['col_major', 'fp32'])
    assert not fails, fails


@pytest.mark.parametrize('mode', [MODE_LOCAL, MODE_FUSED])
def test_weight_pass_through_and_error_record(kern, mode):
    """The pass-through with and without the padded tail line, weighted by the same array and not, and a slot past
    the source rows: skipped and flagged the same way by both routes (the scale factors are only ever addressed
    through the validated slot)."""
    H, width = 1152, 8
    table = _table(width, 3)
    table[9, 2] = SRC_ROWS                                     # one row past the end
    table[10, 0] = 2 ** 31 - 1
    fails = []
    for form, (pair, y) in _pairs(H).items():
        for weighted in (False, True):
            for pad in (0, 32):
                bad = _reduce_both(kern, mode, pair, y, table, H, weighted=weighted, weights=True, pad=pad, flag=True)
                if bad:
                    fails.append((form, weighted, pad, bad))
    assert not fails, fails


def test_every_finite_byte_in_every_column_position(kern):
    """byte_sweep_pair: the 254 finite bytes (both zeros, the subnormals) in every column position, factors
    2^-20 .. 2^20, as fp32 and packed factors; the row copy (width 1) stores each dequantised value as it is, -0.0
    included, widths 2 and 3 sum them from -0 and +0."""
    H = 1024
    q, sf = byte_sweep_pair(H)
    q = q.cuda()
    forms = {'fp32': sf.cuda(), 'col_major': col_major(sf.cuda()), 'ue8m0': pack_ref(sf).cuda()}
    ys = {name: _back(q, f) for name, f in forms.items()}
    torch.cuda.synchronize()
    assert same_bits(ys['fp32'], ys['ue8m0']) and int((bits(ys['fp32']) == -32768).sum()) == H     # byte 0x80: -0.0
    u = torch.arange(UNITS, dtype=torch.int32)
    fails = []
    for width in (1, 2, 3):
        for base in range(0, 254, UNITS):                      # 8 tables: every row is some unit's first slot
            cols = [(base + u + 85 * j) % 254 for j in range(width)]
            table = torch.stack(cols, dim=1).to(torch.int32).cuda()
            for name, f in forms.items():
                for mode in (MODE_FUSED, MODE_LOCAL):
                    bad = _reduce_both(kern, mode, (q, f), ys[name], table, H)
                    if bad:
                        fails.append((width, base, name, mode, bad))
    assert not fails, fails


def test_strided_rows_no_units_and_the_launch_knob(kern):
    H, width = 512, 3
    table = _table(width, 17)
    (q, sf), y = _pairs(H)['fp32']
    wide = torch.zeros((SRC_ROWS, H + 64), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    wide.view(torch.uint8)[:, :H] = q.view(torch.uint8)
    view = wide[:, :H]
    assert view.stride(0) == H + 64 and not view.is_contiguous()
    assert not _reduce_both(kern, MODE_FUSED, (view, sf), y, table, H)
    # no units: nothing is launched, whatever the other arguments hold
    out = _poisoned(4, H)
    kern.combine_reduce(MODE_FUSED, q, out, 0, table=table, src_sf=sf)
    torch.cuda.synchronize()
    assert bool((bits(out) == POISON).all())
    # every launch shape the diagnostics knob can select gives the same bits
    fails = []
    try:
        for vpt in (1, 2):
            for rows in (2, 4, 8):
                assert kern.lib.deepep_set_launch_config(vpt, rows) == 0
                for mode in (MODE_FUSED, MODE_LOCAL, MODE_EPILOGUE):
                    for upb in (4, 8):
                        out = _poisoned(UNITS, H)
                        want = _poisoned(UNITS, H)
                        kern.combine_reduce(mode, q, out, UNITS, table=table, units_per_block=upb, src_sf=sf)
                        kern.combine_reduce(mode, y, want, UNITS, table=table, units_per_block=upb)
                        if not same_bits(out, want):
                            fails.append((vpt, rows, mode, upb))
    finally:
        assert kern.lib.deepep_set_launch_config(0, 0) == 0
    torch.cuda.synchronize()
    assert not fails, fails


def test_wrapper_rejections_launch_nothing(kern):
    H = 512
    table = _table(3, 1)
    (q, sf), _ = _pairs(H)['fp32']
    packed = _pairs(H)['ue8m0'][0][1]
    out = _poisoned(UNITS, H)
    off = torch.zeros((SRC_ROWS, H + 8), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    bad = [dict(src=q.view(torch.uint8)), dict(src=q.cpu()), dict(src=q.t()), dict(src=q[:, :192]),
           dict(src=off[:, :H]),                                            # rows 8 bytes off a 16-byte multiple
           dict(src_sf=sf.double()), dict(src_sf=sf[:, :-1]), dict(src_sf=sf[:-1]), dict(src_sf=sf.cpu()),
           dict(src_sf=packed[:, :0]), dict(src_sf=torch.zeros((SRC_ROWS, H // 128), dtype=torch.int32, device='cuda')),
           dict(src=q[:, :384], src_sf=torch.zeros((SRC_ROWS, 1), dtype=torch.int32, device='cuda')),
           dict(out=out.float())]
    for kw in bad:
        args = dict(dict(src=q, src_sf=sf, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.combine_reduce(MODE_FUSED, args['src'], args['out'], UNITS, table=table, src_sf=args['src_sf'])
    torch.cuda.synchronize()
    assert bool((bits(out) == POISON).all())                   # nothing was launched
    kern.combine_reduce(MODE_FUSED, q, out, UNITS, table=table, src_sf=packed)
    torch.cuda.synchronize()
    assert not bool((bits(out) == POISON).all())


# ----------------------------------------------------------------------------- public, EP = 1
T1, K1, E1 = 129, 3, 8


def _buffer(group, T, H, K, kernels=None, **kw):
    """kernels: the provider the spy forwards to (default: HipKernels())."""
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, **kw)
    buf._kernels = Spy(HipKernels() if kernels is None else kernels)
    return buf


@pytest.mark.parametrize('H', [512, 2560])             # the packed minimum; two full chunks and a half
def test_pair_combine_equals_cast_back_route_one_rank(H):
    buf = _buffer(_group1(), T1, H, K1)
    single = _buffer(_group1(), T1, H, K1, allow_multiple_reduction=False)
    fails = pair_combine_cases(buf, routed_inputs(H, T1, H, K1, E1, 'cuda'), routed_inputs(H + 1, 0, H, K1, E1, 'cuda'),
                               E1, _back, single=single)
    assert not fails, fails
    assert 'cast_back_fp8' not in buf.kernels.names() + single.kernels.names()


def test_independent_expert_rows_one_rank():
    """Expert rows that are not copies of the dispatched tokens, so the order of the sum shows."""
    H = 2560
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = routed_inputs(5, T1, H, K1, E1, 'cuda')
    recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True)
    for name, pair in pair_forms(binade_rows(recv_x.shape[0], H, 6), 'cuda').items():
        for kw in (dict(), dict(apply_topk_weights=True)):
            bad = combine_differences(buf, pair, handle, _back, topk_weights=recv_w, **kw)
            assert not bad, (name, kw, bad)


def test_pair_combine_execution_modes():
    """No host synchronisation, a HIP graph replayed twice over rewritten pairs, a CU budget and the async mode."""
    H = 512
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = routed_inputs(7, T1, H, K1, E1, 'cuda')
    (q, sf), _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                                                 cast_to_fp8=True)
    assert not combine_differences(buf, (q, sf), handle, _back, topk_weights=recv_w)      # (the plan is built)
    want = buf.combine(_back(q, sf), handle, topk_weights=recv_w)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = buf.combine((q, sf), handle, topk_weights=recv_w)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert not combine_differences(buf, (q, sf), handle, _back, topk_weights=recv_w, num_sms=16)
    assert not combine_differences(buf, (q, sf), handle, _back, wait=True, topk_weights=recv_w,
                                   async_with_compute_stream=True)
    assert not combine_differences(buf, (q, sf), handle, _back, wait=True, topk_weights=recv_w, num_sms=16,
                                   async_with_compute_stream=True)
    # one capture, replayed twice with the pair rewritten in between
    pairs = [pair_forms(binade_rows(q.shape[0], H, 70 + i), 'cuda')['fp32'] for i in range(2)]
    qs, sfs = q.clone(), sf.clone()

    def call():
        return buf.combine((qs, sfs), handle, topk_weights=recv_w)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for i in (0, 1):
        qs.view(torch.uint8).copy_(pairs[i][0].view(torch.uint8))
        sfs.copy_(pairs[i][1])
        graph.replay()
        torch.cuda.synchronize()
        want = buf.combine(_back(*pairs[i]), handle, topk_weights=recv_w)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want[0].float()).all())
        assert same_bits(out[0], want[0]) and same_bits(out[1], want[1]), f'replay {i}'
    assert not same_bits(pairs[0][0].view(torch.uint8), pairs[1][0].view(torch.uint8))
    del graph


def test_public_rejections_launch_nothing():
    H = 512
    buf = _buffer(_group1(), T1, H, K1)
    x, idx, w = routed_inputs(9, T1, H, K1, E1, 'cuda')
    (q, sf), _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E1, do_expand=True,
                                                 cast_to_fp8=True)
    n = q.shape[0]
    wide = torch.zeros((n, H + 64), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    before = len(buf.kernels.calls)
    for what, pair in (('first member not float8', (q.view(torch.uint8), sf)),
                       ('rows not contiguous', (wide[:, :H], sf)),
                       ('1-D rows', (q[0], sf)),
                       ('H % 128 != 0', (q[:, :192].contiguous(), sf[:, :2].contiguous())),
                       ('float64 factors', (q, sf.double())),
                       ('factor shape', (q, sf[:, :-1])),
                       ('factors on the host', (q, sf.cpu())),
                       ('int32 factors, H % 512 != 0', (q[:, :384].contiguous(),
                                                        torch.zeros((n, 1), dtype=torch.int32, device='cuda')))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.combine(pair, handle, topk_weights=recv_w)
        assert len(buf.kernels.calls) == before, what
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- EP = 4, thread ranks
T4, H4, K4, E4 = 33, 512, 4, 8


def _rank_thread(rank, comm, bypass, leaving, results, kernels=None):
    """kernels: rank -> the provider that rank's spies forward to (default: HipKernels())."""
    from tests.sim import FakeGroup
    bufs = inputs = empty = None
    try:
        torch.cuda.set_device(0)
        bufs = []
        for amr in (True, False):
            buf = _buffer(FakeGroup(rank, comm.n, comm), T4, H4, K4, allow_multiple_reduction=amr,
                          kernels=None if kernels is None else kernels(rank))
            comm.install(buf, rank)
            buf.local_bypass = bypass
            bufs.append(buf)
        inputs = routed_inputs(40 + rank, T4, H4, K4, E4, 'cuda')
        empty = routed_inputs(50 + rank, 0 if rank == 1 else T4, H4, K4, E4, 'cuda')
        # every form and mode, the padded plans of do_cpu_sync=False handles and a rank without tokens among them
        fails = pair_combine_cases(bufs[0], inputs, empty, E4, _back, single=bufs[1])
        torch.cuda.synchronize()
        names = bufs[0].kernels.names() + bufs[1].kernels.names()
        if 'cast_back_fp8' in names or 'combine_reduce' not in names:
            fails.append(f'unexpected wrapper calls {sorted(set(names))}')
        results[rank] = fails
    except Exception:
        results[rank] = [traceback.format_exc()]
        comm.bar.abort()
    finally:
        with leaving:                                          # the ranks leave one at a time, the device idle
            torch.cuda.synchronize()
            bufs = inputs = empty = None


@pytest.mark.parametrize('bypass', [True, False])
def test_pair_combine_equals_cast_back_route_four_thread_ranks(bypass):
    from tests.sim import ThreadComm, run_threads
    comm = ThreadComm(4)
    results = run_threads(4, _rank_thread, (comm, bypass, threading.Lock()), timeout=120)
    assert sorted(results) == [0, 1, 2, 3], results
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad


# ----------------------------------------------------------------------------- EP = 2 over xGMI windows
def _xgmi_worker(rank, world, port, amr, queue):
    sys.path.insert(0, ROOT)
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        os.environ['DEEPEP_TRANSPORT'] = 'xgmi'
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        inputs = routed_inputs(60 + rank, T4, H4, K4, E4, 'cuda')
        empty = routed_inputs(65 + rank, 0 if rank == 1 else T4, H4, K4, E4, 'cuda')
        buf = _buffer(dist.group.WORLD, T4, H4, K4, allow_multiple_reduction=amr, explicitly_destroy=True,
                      num_gpu_timeout_secs=20)
        fails = pair_combine_cases(buf, inputs, empty, E4, _back) if amr else \
            pair_combine_cases_single(buf, inputs, empty)
        torch.cuda.synchronize()
        buf._sym.check()
        names = buf.kernels.names()
        buf.destroy()
        if 'combine_reduce_scatter' not in names or 'cast_back_fp8' in names:
            fails.append(f'unexpected wrapper calls {sorted(set(names))}')
        queue.put((rank, fails))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        queue.put((rank, [traceback.format_exc()]))


def pair_combine_cases_single(buf, inputs, empty):
    """The single-reduction cases of pair_combine_cases on a buffer built with allow_multiple_reduction=False."""
    fails = []
    for label, (x, idx, w), kw, more in (
            ('single reduction', inputs, dict(), dict()),
            ('single reduction, apply_topk_weights', inputs, dict(), dict(apply_topk_weights=True)),
            ('single reduction, no CPU sync', inputs,
             dict(do_cpu_sync=False, expert_alignment=16, do_zero_padding=True), dict()),
            ('single reduction, no tokens on one rank', empty, dict(), dict())):
        pair, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E4, do_expand=True,
                                                  cast_to_fp8=True, **kw)
        if more:
            more = dict(more, topk_weights=recv_w)
        bad = combine_differences(buf, pair, handle, _back, **more)
        if bad:
            fails.append(f'{label}: {bad}')
    return fails


@pytest.mark.parametrize('multiple_reduction', [True, False])
def test_pair_combine_equals_cast_back_route_over_xgmi_windows(multiple_reduction):
    world = 2
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_xgmi_worker, args=(r, world, port, multiple_reduction, queue)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, failures = queue.get(timeout=150)
            results[rank] = failures
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    if len(results) != world or any(results.values()):
        tails = {r: [f[-1500:] for f in fl] for r, fl in results.items()}
        pytest.fail(f'{len(results)}/{world} ranks reported; failures: {tails}', pytrace=False)
