"""combine(use_logfmt=True) over the xGMI windows on the GPU (combine_item_scatter_logfmt, csrc/combine.hip).

  kernel   deepep_combine_reduce_scatter_logfmt in one process, its windows two slices of one local allocation: the
           wire rows are bit for bit the composition of two older kernels -- cast_logfmt of the row the bf16 scatter
           stores for the same arguments, and that scatter's weight tail -- and no byte outside the coded bytes and
           the tail of a written row is touched
  end to end   processes sharing the GPU over HIP-IPC windows (the pattern of tests/test_xgmi_gpu.py): the xGMI
           combine with the flag is bit for bit the RCCL one (which tests/test_logfmt_gpu.py and test_logfmt_cpu.py
           pin to the codec and the float64 stand-in), alternating with plain calls on the one window, with an FP8
           pair, and captured into a HIP graph
  quality  the reference's own check (tests/legacy/test_low_latency.py:178-181) at EP = 4 over the windows
"""
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fp8_combine_ref import same_bits
from tests.test_logfmt_gpu import SRC_ROWS, UNITS, _cast_input, _epilogue_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD = 0xa5
GAP = 48                                  # bytes between two window rows (16-byte aligned rows, never written)
EXTRA = 5                                 # window rows no unit is stored into


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


_SOURCES = {}


def _source(H: int):
    """SRC_ROWS bf16 rows, randn * 0.25; rows 0-4 are _cast_input's: in their first group zeros, a constant, an Inf, a
    NaN and bf16 denormals beside one normal value."""
    if H not in _SOURCES:
        g = torch.Generator().manual_seed(H + 2)
        x = (torch.randn((SRC_ROWS, H), generator=g) * 0.25).to(torch.bfloat16)
        x[:5] = _cast_input(H)[0][:5]
        _SOURCES[H] = (x.cuda(), torch.rand((SRC_ROWS,), generator=g).cuda())
    return _SOURCES[H]


def _table(width: int, seed: int) -> torch.Tensor:
    """_epilogue_table (units 0-4: 0, 1, 2, 3 and min(8, width) valid slots); a table of width 1 also sends the
    five special source rows through units 5-9, unreduced."""
    t = _epilogue_table(width, seed)
    if width == 1:
        t[5:10, 0] = torch.arange(5, dtype=torch.int32, device='cuda')
    return t


class Windows:
    """Two windows, the halves of one allocation filled with the guard byte, of rows `pitch` bytes apart; the units'
    rows are a random choice of both windows' rows."""

    def __init__(self, row_bytes: int, seed: int, units: int = UNITS):
        self.row_bytes, self.pitch = row_bytes, row_bytes + GAP
        self.per_window = (units + EXTRA + 1) // 2
        self.bytes = self.per_window * self.pitch
        self.mem = torch.full((2 * self.bytes,), GUARD, dtype=torch.uint8, device='cuda')
        assert self.mem.data_ptr() % 16 == 0
        self.bases = torch.tensor([self.mem.data_ptr(), self.mem.data_ptr() + self.bytes], dtype=torch.int64,
                                  device='cuda')
        self.rows = torch.randperm(2 * self.per_window, generator=torch.Generator().manual_seed(seed))[:units]
        self.out_rows = (self.mem.data_ptr() + self.rows * self.pitch).to(torch.int64).cuda()

    @property
    def windows(self):
        return self.bases, self.bytes

    def image(self) -> torch.Tensor:
        """[2 * per_window, pitch] bytes on the host."""
        return self.mem.cpu().view(2 * self.per_window, self.pitch)


def _scatter_both(kern, H, table, weighted, num_weights, seed, *, edit=None, flag=0):
    """The bf16 scatter and the LogFMT scatter with the same arguments, each into its own windows (the same rows of
    them).  edit(out_rows) changes both address lists alike.  -> (bf16 windows, LogFMT windows, error records)."""
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    src, row_w = _source(H)
    K = max(num_weights, 1)
    pk = packed_row_layout(H, K, True, num_weights == 1)
    lf = logfmt_row_layout(H, K, True, num_weights == 1)
    res = []
    for (row_bytes, w_off, w_pad), kw in ((pk, {}), (lf, dict(dst_logfmt=True))):
        win = Windows(row_bytes, seed)
        if edit is not None:
            edit(win)
        err = torch.zeros((8,), dtype=torch.int32, device='cuda')
        err[0] = flag
        kern.combine_reduce_scatter(src, UNITS, win.out_rows, table=table, row_weights=row_w if weighted else None,
                                    wtable=table if num_weights else None, wsrc=row_w if num_weights else None,
                                    num_weights=num_weights, weights_offset=w_off, weights_pad=w_pad,
                                    error_flag=err, windows=win.windows, **kw)
        res.append((win, w_off, err))
    torch.cuda.synchronize()
    return res


def _compare(kern, H, res, num_weights, stored):
    """What differs between the LogFMT windows and cast_logfmt of the bf16 windows' rows; `stored`: the units that
    are stored at all (bool [UNITS])."""
    (bw, b_off, _), (lw, l_off, _) = res
    bimg, limg = bw.image(), lw.image()
    rows = bw.rows[stored]
    x = bimg[rows, :2 * H].contiguous().view(torch.bfloat16).cuda()
    n = x.shape[0]
    planes = torch.empty((n, H * 5 // 4), dtype=torch.uint8, device='cuda')
    meta = torch.empty((n, H // 128), dtype=torch.int32, device='cuda')
    kern.cast_logfmt(x, planes, meta)
    torch.cuda.synchronize()
    coded = H * 5 // 4
    bad = []
    if not torch.equal(limg[rows, :coded], planes.cpu()):
        bad.append('planes')
    if not torch.equal(limg[rows, coded:coded + H // 32], meta.cpu().view(torch.uint8).view(n, H // 32)):
        bad.append('meta')
    written = torch.zeros_like(limg, dtype=torch.bool)
    written[rows, :coded + H // 32] = True
    if num_weights:
        if not torch.equal(limg[rows, l_off:l_off + 128], bimg[rows, b_off:b_off + 128]):
            bad.append('weight tail')
        written[rows, l_off:l_off + 128] = True
    if not bool((limg[~written] == GUARD).all()):
        bad.append('a byte outside the coded bytes and the tail')
    # the bf16 scatter's own guard, so that a fault of the harness is not blamed on the new kernel
    bw_written = torch.zeros_like(bimg, dtype=torch.bool)
    bw_written[rows, :2 * H] = True
    if num_weights:
        bw_written[rows, b_off:b_off + 128] = True
    assert bool((bimg[~bw_written] == GUARD).all())
    return bad


@pytest.mark.parametrize('width', [1, 3, 8])
@pytest.mark.parametrize('H', [128, 384, 2176, 7168])
def test_wire_rows_are_cast_logfmt_of_the_bf16_scatters_rows(kern, H, width):
    table = _table(width, H + width)
    all_units = torch.ones((UNITS,), dtype=torch.bool)
    fails = []
    for weighted in (False, True):
        for num_weights in (0, 1, width):
            res = _scatter_both(kern, H, table, weighted, num_weights, seed=H + width + num_weights)
            bad = _compare(kern, H, res, num_weights, all_units)
            if not torch.equal(res[0][2].cpu(), res[1][2].cpu()):
                bad.append(f'error records {res[0][2].tolist()} / {res[1][2].tolist()}')
            if bad:
                fails.append((weighted, num_weights, bad))
    assert not fails, fails
    if width == 1:                         # the special rows did travel: a NaN group and an exact (constant) group
        win = res[1][0]
        img = win.image()
        metas = img[win.rows[5:10], H * 5 // 4:H * 5 // 4 + 4].contiguous().view(torch.int32).view(-1)
        assert int(metas[0]) == 0 and (int(metas[1]) & 0xffff) == (int(metas[1]) >> 16) & 0xffff
        assert (int(metas[2]) & 0xffff) == 0x7f80 and (int(metas[3]) & 0x7fff) > 0x7f80


def test_padding_rejected_and_outside_rows_store_nothing(kern):
    H, width = 384, 3
    table = _table(width, 17)
    canary = torch.full((1 << 16,), GUARD, dtype=torch.uint8, device='cuda')
    outside = canary.data_ptr() + 4096

    def edit(win):
        win.out_rows[6] = 1                                   # a padding position: silent
        win.out_rows[11] = 0                                  # a unit the plan rejected: bit 1
        win.out_rows[20] = outside                            # not in any window: bit 4 and the record

    res = _scatter_both(kern, H, table, True, width, seed=3, edit=edit)
    stored = torch.ones((UNITS,), dtype=torch.bool)
    stored[[6, 11, 20]] = False
    assert not _compare(kern, H, res, width, stored)          # the rows of units 6, 11, 20 included: all guard bytes
    assert bool((canary == GUARD).all())
    (_, _, be), (lw, l_off, le) = res
    be, le = be.tolist(), le.tolist()
    assert le[0] == be[0] == 1 | 4 and le[1:6] == be[1:6] and le[1] == 1 and le[2] == 20
    assert (le[5] & 0xffffffff) << 32 | (le[4] & 0xffffffff) == outside
    assert le[6] == (lw.bytes - (l_off + 128)) >> 4           # the extent a wire row is checked with
    # a window one byte short of the last row's tail: that row is outside it
    from deepep_amd.handle import logfmt_row_layout
    row_bytes, w_off, w_pad = logfmt_row_layout(H, width)
    win = Windows(row_bytes, 5)
    last = int(win.rows.argmax())
    src, row_w = _source(H)
    err = torch.zeros((8,), dtype=torch.int32, device='cuda')
    short = int(win.rows.max()) * win.pitch + win.row_bytes - 1
    kern.combine_reduce_scatter(src, UNITS, win.out_rows, table=table, wtable=table, wsrc=row_w, num_weights=width,
                                weights_offset=w_off, weights_pad=w_pad, error_flag=err,
                                windows=(win.bases[:1], short), dst_logfmt=True)
    torch.cuda.synchronize()
    img = win.image()
    assert int(err[0]) == 4 and int(err[2]) == last and bool((img[win.rows[last]] == GUARD).all())
    assert bool((img[win.rows[(last + 1) % UNITS], :H] != GUARD).any())


def test_a_timed_out_barrier_stores_nothing(kern):
    for H, width in ((128, 1), (2176, 8)):
        res = _scatter_both(kern, H, _table(width, 2), False, width, seed=9, flag=2)
        for win, _, err in res:
            assert bool((win.mem == GUARD).all()) and int(err[0]) == 2


def test_every_instantiated_shape(kern):
    width = 8
    all_units = torch.ones((UNITS,), dtype=torch.bool)
    fails = []
    try:
        for vpt in (1, 2):
            for rows in (2, 4):
                assert kern.lib.deepep_set_launch_config(vpt, rows) == 0
                for H in (128, 2176):
                    for weighted in (False, True):
                        res = _scatter_both(kern, H, _table(width, 6), weighted, width, seed=vpt + rows)
                        bad = _compare(kern, H, res, width, all_units)
                        if bad:
                            fails.append((vpt, rows, H, weighted, bad))
    finally:
        assert kern.lib.deepep_set_launch_config(0, 0) == 0
    assert not fails, fails


def test_wrapper_refusals_launch_nothing(kern):
    from deepep_amd.handle import logfmt_row_layout
    H = 384
    row_bytes, w_off, w_pad = logfmt_row_layout(H, 3)
    win = Windows(row_bytes, 1)
    table = _table(3, 1)
    src, row_w = _source(H)
    sf = torch.ones((SRC_ROWS, H // 128), device='cuda')
    for s, kw in ((torch.zeros((SRC_ROWS, 192), dtype=torch.bfloat16, device='cuda'), {}),
                  (src.to(torch.float8_e4m3fn), dict(src_sf=sf)), (src, dict(src_sf=sf)), (src.cpu(), {}),
                  (src.float(), {})):
        with pytest.raises(RuntimeError):
            kern.combine_reduce_scatter(s, UNITS, win.out_rows, table=table, wtable=table, wsrc=row_w, num_weights=3,
                                        weights_offset=w_off, weights_pad=w_pad, windows=win.windows,
                                        dst_logfmt=True, **kw)
    with pytest.raises(RuntimeError):                          # a weight tail on top of the meta dwords
        kern.combine_reduce_scatter(src, UNITS, win.out_rows, table=table, wtable=table, wsrc=row_w, num_weights=3,
                                    weights_offset=H * 5 // 4, weights_pad=w_pad, windows=win.windows,
                                    dst_logfmt=True)
    torch.cuda.synchronize()
    assert bool((win.mem == GUARD).all())


# ----------------------------------------------------------------------------- end to end, HIP-IPC windows
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _spawn(target, world, args, timeout=150):
    """Collect / join / kill (tests/test_xgmi_gpu.py): a lost rank ends the test instead of hanging it."""
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, queue) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, payload = queue.get(timeout=timeout)
            results[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return results


def _init(rank, world, port, chunks=0):
    sys.path.insert(0, ROOT)
    if chunks:
        os.environ['DEEPEP_COMBINE_CHUNKS'] = str(chunks)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    return dist


def _buffers(dist, T, H, K, amr, timeout=20):
    from deepep_amd import ElasticBuffer
    from deepep_amd.kernels import HipKernels
    from tests.fp8_oracle_kernels import Spy
    bufs = {}
    for transport in ('xgmi', 'rccl'):
        os.environ['DEEPEP_TRANSPORT'] = transport
        bufs[transport] = ElasticBuffer(dist.group.WORLD, num_max_tokens_per_rank=T, hidden=H, num_topk=K,
                                        allow_multiple_reduction=amr, explicitly_destroy=True,
                                        num_gpu_timeout_secs=timeout)
    bufs['xgmi']._kernels = Spy(HipKernels())
    return bufs


def _worker(rank, world, port, queue, T, H, K, empty_rank, chunks):
    try:
        dist = _init(rank, world, port, chunks)
        import deepep_amd
        dev = torch.device('cuda', 0)
        E = 8 * world
        rng = np.random.default_rng(300 + world + K + rank)
        Tr = 0 if rank == empty_rank else T                   # empty_rank sends no tokens
        idx = np.array([rng.permutation(E)[:K] for _ in range(Tr)], dtype=np.int64).reshape(Tr, K)
        idx[rng.random((Tr, K)) < 0.15] = -1
        if Tr:
            idx[0] = -1                                       # a token routed nowhere
        w = rng.random((Tr, K)).astype(np.float32) * (idx >= 0)
        idx_t, w_t = torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev)
        g = torch.Generator(device=dev).manual_seed(40 + rank)
        x = torch.zeros((Tr, H), dtype=torch.bfloat16, device=dev)
        b0 = torch.randn((Tr, H), device=dev, generator=g).to(torch.bfloat16)
        b1 = torch.randn((Tr, H), device=dev, generator=g).to(torch.bfloat16)
        failures = []
        for amr in (True, False):
            bufs = _buffers(dist, T, H, K, amr)
            xb, rb = bufs['xgmi'], bufs['rccl']
            _, _, ex_w, handle, _ = xb.dispatch(x, topk_idx=idx_t, topk_weights=w_t, num_experts=E, do_expand=True)
            y = (torch.randn((handle.num_expanded_tokens, H), device=dev, generator=g) * 0.25).to(torch.bfloat16)
            cases = [dict(topk_weights=ex_w), dict(topk_weights=ex_w, bias=(b0, b1)), dict(bias=b0)] if amr else \
                [dict(topk_weights=ex_w, apply_topk_weights=True, bias=b0), dict()]
            sym = None
            for ci, kw in enumerate(cases):
                tag = f'amr={amr} case {ci}'
                want = rb.combine(y, handle, use_logfmt=True, **kw)[:2]
                plain = rb.combine(y, handle, **kw)[:2]
                torch.cuda.synchronize()
                n0 = len(xb.kernels.calls)
                for it in range(3):                           # the pitch of the one window's rows switches each call
                    got = xb.combine(y, handle, use_logfmt=True, **kw)[:2]
                    got_plain = xb.combine(y, handle, **kw)[:2]
                    torch.cuda.synchronize()
                    sym = xb._sym if sym is None else sym
                    if xb._sym is not sym:
                        failures.append(f'{tag} round {it}: the window was re-allocated')
                    if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
                        failures.append(f'{tag} round {it}: xgmi use_logfmt != rccl use_logfmt')
                    if not (same_bits(got_plain[0], plain[0]) and same_bits(got_plain[1], plain[1])):
                        failures.append(f'{tag} round {it}: the plain xgmi combine after a LogFMT one')
                    if Tr and same_bits(got[0], got_plain[0]):
                        failures.append(f'{tag} round {it}: the flag changed nothing')
                    if not same_bits(got[1], got_plain[1]):
                        failures.append(f'{tag} round {it}: the flag changed the passed-through weights')
                calls = xb.kernels.calls[n0:]
                names = [c[0] for c in calls]
                if not any(c[0] == 'combine_reduce_scatter' and dict(c[2]).get('dst_logfmt') for c in calls) or \
                        not any(c[0] == 'combine_reduce' and 'src_logfmt_meta' in dict(c[2]) for c in calls):
                    failures.append(f'{tag}: the flag made the calls {names}')
                if 'logfmt_pack_rows' in names or 'cast_logfmt' in names:
                    failures.append(f'{tag}: a staging encode in {names}')
            # an FP8 pair (fp32 factors): phase A reduces into staging rows, the LogFMT scatter copies them
            pair = deepep_amd.per_token_cast_to_fp8(y)
            kw = cases[0]
            want = rb.combine(pair, handle, use_logfmt=True, **kw)[:2]
            got = xb.combine(pair, handle, use_logfmt=True, **kw)[:2]
            torch.cuda.synchronize()
            if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
                failures.append(f'amr={amr}: FP8 pair, xgmi use_logfmt != rccl use_logfmt')
            # a HIP graph after the eager calls (the plan is cached): replayed twice, an eager call in between
            kw = cases[1] if amr else cases[0]
            want = rb.combine(y, handle, use_logfmt=True, **kw)[:2]
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                g_out, g_w, _ = xb.combine(y, handle, use_logfmt=True, **kw)
            for it in range(2):
                g_out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                if not (same_bits(g_out, want[0]) and same_bits(g_w, want[1])):
                    failures.append(f'amr={amr}: graph replay {it}')
                if it == 0:
                    out = xb.combine(y, handle, use_logfmt=True, **kw)[0]
                    torch.cuda.synchronize()
                    if not same_bits(out, want[0]):
                        failures.append(f'amr={amr}: eager call between the replays')
            del graph
            if xb._sym is not sym:
                failures.append(f'amr={amr}: the window was re-allocated')
            xb._sym.check()
            for b in bufs.values():
                b.destroy()
        queue.put((rank, failures))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        queue.put((rank, [traceback.format_exc()]))


@pytest.mark.parametrize('world,T,H,K,empty_rank,chunks', [
    (2, 96, 384, 3, -1, 0), (4, 64, 2176, 8, -1, 3),
    (4, 80, 256, 2, -1, 0),                                   # R > K: the top-k window layout
    (3, 40, 512, 4, 1, 2),                                    # a rank that sends nothing
    (8, 48, 512, 8, -1, 2)])
def test_xgmi_use_logfmt_is_the_rccl_use_logfmt(world, T, H, K, empty_rank, chunks):
    results = _spawn(_worker, world, (T, H, K, empty_rank, chunks))
    if len(results) != world or any(results.values()):
        tails = {r: [f[-1500:] for f in fl] for r, fl in results.items()}
        pytest.fail(f'{len(results)}/{world} ranks reported; failures: {tails}', pytrace=False)


# ----------------------------------------------------------------------------- quality
def _quality_worker(rank, world, port, queue, T, H, K, E):
    try:
        dist = _init(rank, world, port)
        from deepep_amd import topk_idx_t
        from tests import logfmt_ref as lf
        bufs = _buffers(dist, T, H, K, False)
        diffs, failures = [], []
        for scale in (0.1, 0.25):
            g = torch.Generator().manual_seed(11 + rank)      # the inputs of tests/test_logfmt_gpu.py's quality test
            x = (torch.randn((T, H), generator=g) * scale).to(torch.bfloat16).cuda()
            w, idx = torch.topk(torch.rand((T, E), generator=g), K, dim=-1)
            idx, w = idx.to(topk_idx_t).cuda(), w.cuda()
            recv_x, _, recv_w, handle, _ = bufs['xgmi'].dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E,
                                                                 do_expand=True)
            exact = x.double() * w.double().sum(dim=1, keepdim=True)
            outs = {t: b.combine(recv_x, handle, topk_weights=recv_w, apply_topk_weights=True, use_logfmt=True)[0]
                    for t, b in bufs.items()}                 # identity experts: the expanded rows as they came
            torch.cuda.synchronize()
            diffs.append(lf.calc_diff(exact.cpu(), outs['xgmi'].cpu()))
            if not same_bits(outs['xgmi'], outs['rccl']):
                failures.append(f'randn * {scale}: xgmi != rccl')
            if bool(torch.isnan(outs['xgmi'].float()).any()):
                failures.append(f'randn * {scale}: NaN in combined_x')
        bufs['xgmi']._sym.check()
        for b in bufs.values():
            b.destroy()
        queue.put((rank, (diffs, failures)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        queue.put((rank, ([], [traceback.format_exc()])))


def test_quality_over_the_windows_is_within_the_references_bound():
    """The reference's own check (tests/legacy/test_low_latency.py:178-181) at EP = 4 over the windows: weighted
    single reduction, identity experts, rows randn * 0.1 and randn * 0.25: calc_diff(x * sum(w), combined_x) < 1e-5,
    the reference's bound."""
    results = _spawn(_quality_worker, 4, (128, 7168, 8, 32))
    assert sorted(results) == [0, 1, 2, 3], results
    print(f'calc_diff per rank (randn * 0.1, randn * 0.25) over the windows = { {r: v[0] for r, v in results.items()} }')
    for rank, (diffs, failures) in results.items():
        assert not failures, (rank, failures)
        assert len(diffs) == 2 and all(d < 1e-5 for d in diffs), (rank, diffs)
