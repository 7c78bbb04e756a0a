"""LogFMT-10 on the GPU (deepep_amd/csrc/logfmt_codec.h, logfmt.hip, combine_item_logfmt): the codec kernels against
the float64 stand-in of tests/logfmt_ref.py, logfmt_pack_rows against the cast kernel, the LogFMT epilogue against the
bf16 epilogue over the same build's cast-back rows, and ElasticBuffer.combine(..., use_logfmt=True) over 2 and 4 thread
ranks against the same call made through a provider that replaces the two fused steps by the codec kernels and the
bf16 epilogue -- eagerly with no host synchronisation, and captured into a HIP graph and replayed.

The 1e-3 caps on the share of elements that may differ from the float64 stand-in (by one code, by one bf16 ulp) are
conditions, not measurements: the fp32 and the float64 stand-ins disagree in 2-6e-5 of the codes and 3-4e-5 of the
decoded values on the CPU, and a wrong rounding term moves tens of percent."""
import threading
import traceback

import pytest
import torch

from tests import logfmt_ref as lf
from tests.fp8_combine_ref import bits, routed_inputs, same_bits
from tests.fp8_oracle_kernels import Spy
from tests.test_cast_keyword_gpu import _group1

pytestmark = pytest.mark.gpu

MODE_EPILOGUE = 1
POISON = 0x7b7b
HIDDEN = [128, 384, 2176, 7168]           # one group; three; 17 groups = 272 vectors (two passes and a part); config 2
ROWS = [1, 5, 129]                        # less than a workgroup of four rows; one more; 33 workgroups, the last short


@pytest.fixture(scope='module')
def kern():
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    return HipKernels()


def _cast(kern, x):
    T, H = x.shape
    planes = torch.full((T + 1, H * 5 // 4), 0xa5, dtype=torch.uint8, device='cuda')
    meta = torch.full((T + 1, H // 128), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    kern.cast_logfmt(x, planes[:T], meta[:T])
    torch.cuda.synchronize()
    assert bool((planes[T] == 0xa5).all()) and bool((meta[T] == 0x5a5a5a5a).all())
    return planes[:T], meta[:T]


def _back(kern, planes, meta):
    out = torch.empty((planes.shape[0], meta.shape[1] * 128), dtype=torch.bfloat16, device='cuda')
    kern.cast_back_logfmt(planes, meta, out)
    return out


_INPUTS = {}


def _cast_input(H: int):
    """129 rows: randn * {0.1, 0.25, 10} by group, and in the first group of rows 0-4 zeros, a constant, an Inf, a NaN
    and bf16 denormals beside one normal value; with the float64 stand-in's codes, signs and meta (computed once)."""
    if H not in _INPUTS:
        g = torch.Generator().manual_seed(H)
        n, G = 129, H // 128
        scale = torch.tensor([0.1, 0.25, 10.0])[torch.randint(0, 3, (n, G, 1), generator=g)]
        x = (torch.randn((n, G, 128), generator=g) * scale).reshape(n, H).to(torch.bfloat16)
        x[0, :128] = 0
        x[1, :128] = -1.75
        x[2, 3] = float('inf')
        x[3, 9] = float('nan')
        x[4, :128] = lf.bits_bf16(torch.full((128,), 0x8040))
        x[4, 77] = 0.5
        _INPUTS[H] = (x, lf.encode_ref(x, torch.float64))
    return _INPUTS[H]


# ----------------------------------------------------------------------------- cast
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('H', HIDDEN)
def test_cast_against_the_float64_stand_in(kern, H, rows):
    x, (code, sign, meta) = _cast_input(H)
    wide = torch.zeros((rows, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x[:rows].cuda()
    for xin in (x[:rows].cuda(), wide[:, :H]):                 # contiguous and strided rows
        planes, m = _cast(kern, xin)
        assert torch.equal(m.cpu(), meta[:rows]), 'meta'
        c, s = lf.unpack_planes(planes.cpu())
        assert torch.equal(s, sign[:rows])
        diff = (c - code[:rows]).abs()
        print(f'H={H} rows={rows}: codes off by one in {float((diff != 0).float().mean()):.2e} of the elements')
        assert int(diff.max()) <= 1
        assert float((diff != 0).float().mean()) <= 1e-3
    import deepep_amd
    p2, m2 = deepep_amd.per_token_cast_to_logfmt(wide[:, :H])
    torch.cuda.synchronize()
    assert torch.equal(p2, planes) and torch.equal(m2, m)


# ----------------------------------------------------------------------------- cast back
def _sweep(H: int):
    """1024 rows in which every column position sees every code 0..511 with both signs; the metas cycle through a
    narrow group, a wide one (amin = 0), one with amax >= 1, a degenerate and a non-finite one."""
    r, c = torch.arange(1024).view(-1, 1), torch.arange(H).view(1, -1)
    combo = (r + c) % 1024
    kinds = torch.tensor([[0x4040, 0x4030], [0x3e80, 0], [0x4120, 0x3a00], [0x3f00, 0x3f00], [0x7f80, 0x3f80]])
    kind = (r // 64 + torch.arange(H // 128).view(1, -1)) % 5
    amax, amin = kinds[kind, 0], kinds[kind, 1]
    amax = amax + torch.where(kind == 3, 0, 1) * (r % 8)       # (a degenerate group stays degenerate)
    amin = torch.where(kind == 3, amax, amin)
    meta = (amax | amin << 16).to(torch.int32)
    return lf.pack_planes((combo & 511).to(torch.int32), (combo >> 9).to(torch.int32)), meta


@pytest.mark.parametrize('H', [128, 384])
def test_cast_back_every_code_and_sign_in_every_column(kern, H):
    import deepep_amd
    planes, meta = _sweep(H)
    want = bits(lf.cast_back_ref(planes, meta, torch.float64)).to(torch.int32) & 0xffff
    got16 = deepep_amd.per_token_cast_back_logfmt(planes.cuda(), meta.cuda())
    torch.cuda.synchronize()
    got = bits(got16).to(torch.int32) & 0xffff
    nan = (want & 0x7fff) > 0x7f80
    assert int(nan.sum()) > 0 and bool(((got & 0x7fff) > 0x7f80)[nan].all()) and not bool(((got & 0x7fff) > 0x7f80)[~nan].any())
    ok = ~nan
    assert bool(((got >> 15) == (want >> 15))[ok].all()), 'sign'
    diff = ((got & 0x7fff) - (want & 0x7fff)).abs()[ok]
    print(f'H={H}: decoded values off by one ulp in {float((diff != 0).float().mean()):.2e} of the elements')
    assert int(diff.max()) <= 1
    assert float((diff != 0).float().mean()) <= 1e-3
    # degenerate groups: a nonzero code is amax exactly, code 0 is zero
    code, _ = lf.unpack_planes(planes)
    degenerate = ((meta & 0xffff) == ((meta >> 16) & 0xffff)).repeat_interleave(128, dim=1)
    amax = (meta & 0xffff).repeat_interleave(128, dim=1)
    assert bool(((got & 0x7fff) == torch.where(code == 0, 0, amax))[degenerate].all())


def test_cast_back_of_cast_reads_strided_rows(kern):
    H = 384
    x, _ = _cast_input(H)
    planes, meta = _cast(kern, x.cuda())
    wide = torch.zeros((129, 512 + H // 32), dtype=torch.uint8, device='cuda')      # rows 524 bytes apart: refused
    with pytest.raises(RuntimeError):
        kern.cast_back_logfmt(wide[:, :H * 5 // 4], meta, torch.empty((129, H), dtype=torch.bfloat16, device='cuda'))
    wire = torch.zeros((129, 640), dtype=torch.uint8, device='cuda')
    wire[:, :480] = planes
    wire[:, 480:492] = meta.view(torch.uint8).view(129, 12)
    out = _back(kern, wire[:, :480], wire.view(torch.int32)[:, 120:123])
    torch.cuda.synchronize()
    assert same_bits(out, _back(kern, planes, meta))


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize('single, K', [(False, 3), (False, 8), (True, 8), (None, 8)])      # None: no weight tail
@pytest.mark.parametrize('H', HIDDEN)
def test_pack_rows_is_the_cast_kernel_with_the_tail_copied(kern, H, single, K):
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    with_w = single is not None
    rb, w_off, _ = packed_row_layout(H, K, with_w, bool(single))
    lb, lw_off, _ = logfmt_row_layout(H, K, with_w, bool(single))
    x, _ = _cast_input(H)
    n, extra = 129, 4                                        # the kernel runs over the first n rows of n + extra
    g = torch.Generator().manual_seed(H + K)
    src = torch.randint(0, 256, (n + extra, rb), generator=g, dtype=torch.uint8).cuda()
    src[:n, :H * 2] = x.cuda().view(torch.uint8).view(n, H * 2)
    dst = torch.full((n + extra, lb), 0xa5, dtype=torch.uint8, device='cuda')
    kern.logfmt_pack_rows(src.view(torch.bfloat16), n, H, dst, src_tail_offset=w_off, dst_tail_offset=lw_off,
                          tail_bytes=lb - lw_off)
    planes, meta = _cast(kern, x.cuda())
    torch.cuda.synchronize()
    coded = H * 5 // 4
    assert torch.equal(dst[:n, :coded], planes)
    assert torch.equal(dst[:n, coded:coded + H // 32], meta.view(torch.uint8).view(n, H // 32))
    assert bool((dst[:n, coded + H // 32:lw_off] == 0xa5).all())             # the padding is not written
    if with_w:
        assert lb - lw_off == rb - w_off == 128 and torch.equal(dst[:n, lw_off:], src[:n, w_off:])
    assert bool((dst[n:] == 0xa5).all())


# ----------------------------------------------------------------------------- the epilogue
UNITS, SRC_ROWS = 33, 301


def _epilogue_table(width: int, seed: int) -> torch.Tensor:
    """[UNITS, width] slots: random rows, a fifth masked; units 0-4 with 0, 1, 2, 3 and min(8, width) valid slots."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, SRC_ROWS, (UNITS, width), generator=g, dtype=torch.int32)
    t[torch.rand((UNITS, width), generator=g) < 0.2] = -1
    for u, n in enumerate((0, 1, 2, 3, 8)):
        t[u] = -1
        t[u, width - min(n, width):] = torch.randint(0, SRC_ROWS, (min(n, width),), generator=g, dtype=torch.int32)
    return t.cuda()


_SOURCES = {}


def _source(kern, H: int):
    if H not in _SOURCES:
        g = torch.Generator().manual_seed(H + 1)
        x = (torch.randn((SRC_ROWS, H), generator=g) * 0.25).to(torch.bfloat16).cuda()
        x[7, :128] = 0
        x[8, :128] = 0.375
        planes, meta = _cast(kern, x)
        _SOURCES[H] = (planes, meta, _back(kern, planes, meta))
        torch.cuda.synchronize()
    return _SOURCES[H]


def _epilogue_both(kern, H, table, weighted, biases, weights, seed=0):
    planes, meta, y = _source(kern, H)
    g = torch.Generator().manual_seed(seed)
    row_w = torch.rand((SRC_ROWS,), generator=g).cuda()
    bias = [torch.randn((UNITS, H), generator=g).to(torch.bfloat16).cuda() for _ in range(biases)] + [None, None]
    outs = []
    for src, kw in ((planes, dict(src_logfmt_meta=meta)), (y, dict())):
        out = torch.full((UNITS + 3, H), POISON, dtype=torch.int16, device='cuda').view(torch.bfloat16)
        ow = torch.full((UNITS + 3, 32), -7.0, device='cuda') if weights else None
        err = torch.zeros((8,), dtype=torch.int32, device='cuda')
        kern.combine_reduce(MODE_EPILOGUE, src, out, UNITS, table=table, row_weights=row_w if weighted else None,
                            bias0=bias[0], bias1=bias[1], wtable=table if weights else None,
                            wsrc=row_w if weights else None, out_weights=ow[:, :table.shape[1]] if weights else None,
                            weights_pad=32 if weights else 0, error_flag=err, **kw)
        outs.append((out, ow, err))
    torch.cuda.synchronize()
    (a, aw, ae), (b, bw, be) = outs
    assert bool(torch.isfinite(b[:UNITS].float()).all()) and bool((bits(b[UNITS:]) == POISON).all())
    bad = [] if same_bits(a, b) else ['rows']
    if weights and not same_bits(aw, bw):
        bad.append('weights')
    if not torch.equal(ae.cpu(), be.cpu()):
        bad.append('error record')
    return bad


@pytest.mark.parametrize('width', [1, 2, 3, 8, 9])
@pytest.mark.parametrize('H', HIDDEN)
def test_logfmt_epilogue_is_the_bf16_epilogue_over_cast_back_rows(kern, H, width):
    table = _epilogue_table(width, H + width)
    fails = [(weighted, biases, weights, bad)
             for weighted in (False, True) for biases in (0, 1, 2) for weights in (False, True)
             for bad in [_epilogue_both(kern, H, table, weighted, biases, weights, seed=width)] if bad]
    assert not fails, fails


def test_a_slot_past_the_source_rows_and_every_launch_shape(kern):
    H, width = 2176, 8
    table = _epilogue_table(width, 5)
    table[9, 2] = SRC_ROWS                                     # one row past the end: skipped and flagged by both
    table[10, 0] = 2 ** 31 - 1
    assert not _epilogue_both(kern, H, table, True, 1, True)
    planes, meta, _ = _source(kern, H)
    err = torch.zeros((8,), dtype=torch.int32, device='cuda')
    out = torch.empty((UNITS, H), dtype=torch.bfloat16, device='cuda')
    kern.combine_reduce(MODE_EPILOGUE, planes, out, UNITS, table=table, src_logfmt_meta=meta, error_flag=err)
    torch.cuda.synchronize()
    assert int(err[0]) & 1
    fails = []
    try:
        for vpt in (1, 2):
            for rows in (2, 4, 8):
                assert kern.lib.deepep_set_launch_config(vpt, rows) == 0
                for h in (128, H):
                    for weighted in (False, True):
                        bad = _epilogue_both(kern, h, _epilogue_table(width, 6), weighted, 2, True)
                        if bad:
                            fails.append((vpt, rows, h, weighted, bad))
    finally:
        assert kern.lib.deepep_set_launch_config(0, 0) == 0
    assert not fails, fails


def test_wrapper_rejections_launch_nothing(kern):
    H = 384
    planes, meta, y = _source(kern, H)
    table = _epilogue_table(3, 1)
    out = torch.full((UNITS, H), POISON, dtype=torch.int16, device='cuda').view(torch.bfloat16)
    for kw in (dict(src=planes[:, :H]), dict(src=planes.view(torch.int8)), dict(src=planes.cpu()),
               dict(meta=meta.float()), dict(meta=meta[:, :-1]), dict(meta=meta[:-1]), dict(meta=meta.cpu()),
               dict(mode=2), dict(mode=0), dict(out=out.float())):
        a = dict(dict(src=planes, meta=meta, mode=MODE_EPILOGUE, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.combine_reduce(a['mode'], a['src'], a['out'], UNITS, table=table, src_logfmt_meta=a['meta'])
    with pytest.raises(RuntimeError):
        kern.combine_reduce(MODE_EPILOGUE, planes, out, UNITS, table=table, src_logfmt_meta=meta, src_sf=meta)
    torch.cuda.synchronize()
    assert bool((bits(out) == POISON).all())


# ----------------------------------------------------------------------------- end to end, thread ranks
class Composition:
    """HipKernels whose two fused LogFMT steps are replaced by the codec kernels: logfmt_pack_rows by cast_logfmt and
    copies, the LogFMT epilogue by cast_back_logfmt and the bf16 epilogue.  TEST ONLY."""
    name = 'hip'

    def __init__(self):
        from deepep_amd.kernels import HipKernels
        self._hip = HipKernels()

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def logfmt_pack_rows(self, src, num_rows, hidden, dst, src_tail_offset=0, dst_tail_offset=0, tail_bytes=0,
                         stream=None):
        if num_rows == 0:
            return
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            x = src.view(torch.bfloat16)[:num_rows, :hidden]
            planes = torch.empty((num_rows, hidden * 5 // 4), dtype=torch.uint8, device=src.device)
            meta = torch.empty((num_rows, hidden // 128), dtype=torch.int32, device=src.device)
            self._hip.cast_logfmt(x, planes, meta, stream=stream)
            coded = hidden * 5 // 4
            dst[:num_rows, :coded] = planes
            dst[:num_rows, coded:coded + hidden // 32] = meta.view(torch.uint8).view(num_rows, hidden // 32)
            if tail_bytes:
                dst[:num_rows, dst_tail_offset:dst_tail_offset + tail_bytes] = \
                    src.view(torch.uint8).view(src.shape[0], -1)[:num_rows, src_tail_offset:src_tail_offset + tail_bytes]

    def combine_reduce(self, mode, src, out, num_units, *args, src_logfmt_meta=None, stream=None, **kw):
        if src_logfmt_meta is None:
            return self._hip.combine_reduce(mode, src, out, num_units, *args, stream=stream, **kw)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            rows = torch.empty((src.shape[0], out.shape[1]), dtype=torch.bfloat16, device=src.device)
            if src.shape[0]:
                self._hip.cast_back_logfmt(src, src_logfmt_meta, rows, stream=stream)
            return self._hip.combine_reduce(mode, rows, out, num_units, *args, stream=stream, **kw)


class MailComm:
    """A row all-to-all among thread ranks through persistent mailboxes, with no cross-stream events, so that a
    combine that uses it can be captured into a HIP graph: every call copies this rank's send rows into its
    mailboxes and then its receive rows out of the peers'.  Eagerly the ranks meet at a host barrier between the two;
    a captured call has no barrier, so the graphs are replayed twice, one rank at a time: the first round fills every
    mailbox, the second reads them all complete (and rewrites them with the same bytes)."""

    def __init__(self, n: int):
        self.n, self.bar = n, threading.Barrier(n, timeout=120)
        self.boxes = {}

    class _Work:
        def __init__(self):
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream())

        def wait(self):
            torch.cuda.current_stream().wait_event(self.event)
            return True

    def a2a(self, rank, out, inp, out_splits=None, in_splits=None):
        capturing = torch.cuda.is_current_stream_capturing()
        in_splits = in_splits if in_splits is not None else [inp.shape[0] // self.n] * self.n
        pos = 0
        for s in range(self.n):
            cnt = in_splits[s]
            key = (rank, s, inp.shape[1] * inp.element_size())
            if not capturing:
                self.boxes[key] = torch.empty((cnt, inp.shape[1]), dtype=inp.dtype, device=inp.device)
            assert self.boxes[key].shape[0] == cnt
            self.boxes[key].copy_(inp[pos:pos + cnt])
            pos += cnt
        if not capturing:
            torch.cuda.synchronize()
            self.bar.wait()
        pos = 0
        for s in range(self.n):
            box = self.boxes[(s, rank, out.shape[1] * out.element_size())]
            assert out_splits is None or box.shape[0] == out_splits[s]
            out[pos:pos + box.shape[0]].copy_(box)
            pos += box.shape[0]
        assert pos == out.shape[0]
        work = self._Work()
        if not capturing:
            torch.cuda.synchronize()
            self.bar.wait()
        return work

    def install(self, buf, rank):
        buf._a2a = lambda out, inp, os_=None, is_=None: self.a2a(rank, out, inp, os_, is_).wait()
        buf._a2a_async = lambda out, inp, os_, is_: self.a2a(rank, out, inp, os_, is_)


def _ep_buffer(rank, comm, T, H, K, kernels, amr):
    from deepep_amd import ElasticBuffer
    from tests.sim import FakeGroup
    buf = ElasticBuffer(FakeGroup(rank, comm.n, comm), num_max_tokens_per_rank=T, hidden=H, num_topk=K,
                        allow_multiple_reduction=amr)
    buf._kernels = Spy(kernels)
    comm.install(buf, rank)
    return buf


def _cases(amr, recv_w, b0, b1):
    if amr:
        return [dict(topk_weights=recv_w), dict(topk_weights=recv_w, bias=(b0, b1)), dict(bias=b0)]
    return [dict(topk_weights=recv_w, apply_topk_weights=True, bias=b0), dict()]


def _ep_rank(rank, comm, mail, capture_lock, T, H, K, E, results):
    from deepep_amd.kernels import HipKernels
    fails = []
    try:
        torch.cuda.set_device(0)
        x, idx, w = routed_inputs(100 * comm.n + rank, T, H, K, E, 'cuda')        # a fifth of the slots masked
        g = torch.Generator().manual_seed(7 + rank)
        b0, b1 = ((torch.randn((T, H), generator=g)).to(torch.bfloat16).cuda() for _ in range(2))
        for amr in (True, False):
            fused = _ep_buffer(rank, comm, T, H, K, HipKernels(), amr)
            composed = _ep_buffer(rank, comm, T, H, K, Composition(), amr)
            recv_x, _, recv_w, handle, _ = fused.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
            _, _, _, handle_c, _ = composed.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
            y = (torch.randn(recv_x.shape, generator=g) * 0.25).to(torch.bfloat16).cuda()
            for i, kw in enumerate(_cases(amr, recv_w, b0, b1)):
                want = composed.combine(y, handle_c, use_logfmt=True, **kw)
                fused.combine(y, handle, use_logfmt=True, **kw)              # (the plan is built)
                torch.cuda.synchronize()
                comm.bar.wait()
                if rank == 0:
                    torch.cuda.set_sync_debug_mode('error')
                comm.bar.wait()
                try:
                    got = fused.combine(y, handle, use_logfmt=True, **kw)
                finally:
                    comm.bar.wait()
                    if rank == 0:
                        torch.cuda.set_sync_debug_mode(0)
                torch.cuda.synchronize()
                plain = fused.combine(y, handle, **kw)
                torch.cuda.synchronize()
                if not bool(torch.isfinite(want[0].float()).all()):
                    fails.append(f'amr={amr} case {i}: wrongly chosen input')
                if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
                    fails.append(f'amr={amr} case {i}: the fused steps differ from the codec kernels + bf16 epilogue')
                if same_bits(got[0], plain[0]) or not same_bits(got[1], plain[1]):
                    fails.append(f'amr={amr} case {i}: the flag changed nothing, or changed the passed-through weights')
            names = fused.kernels.names()
            if 'logfmt_pack_rows' not in names or 'cast_logfmt' in names or 'cast_back_logfmt' in names:
                fails.append(f'amr={amr}: wrapper calls {sorted(set(names))}')
            # ---- captured into a HIP graph and replayed (mailbox all-to-all: see MailComm)
            comm.bar.wait()
            kw = _cases(amr, recv_w, b0, b1)[0]
            ys = y.clone()
            gbuf = _ep_buffer(rank, comm, T, H, K, HipKernels(), amr)
            _, _, _, ghandle, _ = gbuf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
            torch.cuda.synchronize()
            mail.install(gbuf, rank)
            gbuf.combine(ys, ghandle, use_logfmt=True, **kw)                  # eager: the plan and the mailboxes
            torch.cuda.synchronize()
            mail.bar.wait()
            with capture_lock:                                                # one capture at a time, the others idle
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode='relaxed'):   # (the cached plan polls an event)
                    out = gbuf.combine(ys, ghandle, use_logfmt=True, **kw)
                torch.cuda.synchronize()
            mail.bar.wait()
            y2 = (torch.randn(recv_x.shape, generator=g) * 0.25).to(torch.bfloat16).cuda()
            ys.copy_(y2)
            torch.cuda.synchronize()
            for _ in range(2):
                for turn in range(comm.n):
                    if turn == rank:
                        graph.replay()
                        torch.cuda.synchronize()
                    mail.bar.wait()
            want = composed.combine(y2, handle_c, use_logfmt=True, **kw)
            torch.cuda.synchronize()
            if not (same_bits(out[0], want[0]) and same_bits(out[1], want[1])):
                fails.append(f'amr={amr}: the replayed graph differs')
            del graph
            comm.bar.wait()
        results[rank] = fails
    except Exception:
        results[rank] = fails + [traceback.format_exc()]
        comm.bar.abort()
        mail.bar.abort()


@pytest.mark.parametrize('world, H, K', [(2, 384, 3), (4, 2176, 8), (4, 384, 8), (2, 2176, 3)])
def test_use_logfmt_is_the_composition_of_the_codec_and_the_bf16_epilogue(world, H, K):
    from tests.sim import ThreadComm, run_threads
    comm, mail = ThreadComm(world), MailComm(world)
    results = run_threads(world, _ep_rank, (comm, mail, threading.Lock(), 129, H, K, 16), timeout=150)
    assert sorted(results) == list(range(world)), results
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad


def test_flag_has_no_effect_at_one_rank():
    from deepep_amd import ElasticBuffer
    T, H, K, E = 129, 384, 3, 8
    buf = ElasticBuffer(_group1(), num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    x, idx, w = routed_inputs(3, T, H, K, E, 'cuda')
    recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    a = buf.combine(recv_x, handle, topk_weights=recv_w, use_logfmt=True)
    b = buf.combine(recv_x, handle, topk_weights=recv_w)
    torch.cuda.synchronize()
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ----------------------------------------------------------------------------- quality
def _quality_rank(rank, comm, scale, T, H, K, E, results):
    from deepep_amd import ElasticBuffer, topk_idx_t
    from tests.sim import FakeGroup
    try:
        torch.cuda.set_device(0)
        g = torch.Generator().manual_seed(11 + rank)
        x = (torch.randn((T, H), generator=g) * scale).to(torch.bfloat16).cuda()
        w, idx = torch.topk(torch.rand((T, E), generator=g), K, dim=-1)
        idx, w = idx.to(topk_idx_t).cuda(), w.cuda()
        buf = ElasticBuffer(FakeGroup(rank, comm.n, comm), num_max_tokens_per_rank=T, hidden=H, num_topk=K,
                            allow_multiple_reduction=False)
        comm.install(buf, rank)
        recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
        exact = x.double() * w.double().sum(dim=1, keepdim=True)
        diffs = []
        for flag in (True, False):                                # identity experts: the expanded rows as they came
            out = buf.combine(recv_x, handle, topk_weights=recv_w, apply_topk_weights=True, use_logfmt=flag)[0]
            torch.cuda.synchronize()
            diffs.append(lf.calc_diff(exact.cpu(), out.cpu()))
        results[rank] = diffs
    except Exception:
        results[rank] = traceback.format_exc()
        comm.bar.abort()


@pytest.mark.parametrize('scale', [0.1, 0.25])
def test_quality_is_within_the_references_bound(scale):
    """The reference's own check (tests/legacy/test_low_latency.py:178-181): weighted single reduction with identity
    experts at EP = 4, calc_diff(x * sum(w), combined_x) < 1e-5."""
    from tests.sim import ThreadComm, run_threads
    comm = ThreadComm(4)
    results = run_threads(4, _quality_rank, (comm, scale, 128, 7168, 8, 32), timeout=120)
    assert sorted(results) == [0, 1, 2, 3], results
    print(f'randn * {scale}: calc_diff per rank (use_logfmt, bf16) = {results}')
    for rank, diffs in results.items():
        assert isinstance(diffs, list), diffs
        assert diffs[0] < 1e-5, (rank, diffs)
