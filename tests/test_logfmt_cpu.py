"""LogFMT-10 without a GPU: the stand-in's properties (tests/logfmt_ref.py follows deepep_amd/csrc/logfmt_codec.h), the
row layout, the additive C entries, the refusals that come before any kernel call, and ElasticBuffer.combine(...,
use_logfmt=True) on the CPU provider at one rank (no effect) and over 2 and 4 thread ranks: bit for bit the plain
combine whose phase-A rows went through the stand-in's encode and decode, with every row all-to-all of the combine
carrying rows of logfmt_row_layout's size."""
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests import logfmt_ref as lf
from tests.fp8_combine_ref import routed_inputs, same_bits
from tests.fp8_oracle_kernels import Spy
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 384, 3, 8


# ----------------------------------------------------------------------------- the stand-in
def _rows(seed: int, n: int = 9, hidden: int = 512) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, hidden), generator=g) * torch.exp2(torch.randint(-12, 12, (n, hidden // 128, 1), generator=g)
                                                           .float()).expand(n, hidden // 128, 128).reshape(n, hidden)
    x[0, :128] = torch.randn((128,), generator=g) * 0.01 + 3.0          # a narrow group
    x[1, :128] *= (torch.rand((128,), generator=g) > 0.5)               # a wide group: amin = 0
    x[2, :128] = torch.randn((128,), generator=g) * 1e-30               # > 32 binades below amax in the same group
    x[2, 0] = 1.0
    return x.to(torch.bfloat16)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_codes_are_in_range_and_bracket_their_value(dtype):
    x = _rows(1)
    code, sign, meta = lf.encode_ref(x, dtype)
    assert int(code.min()) >= 0 and int(code.max()) <= 511
    assert torch.equal(sign, lf.bf16_bits(x) >> 15)
    a = lf.bits_bf16(lf.magnitudes(x)).double()
    # every finite |x| inside [2^li, amax] lies between the decode of code - 1 and of code + 1
    below, _ = lf.decode_value((code - 1).clamp(min=0), meta, torch.float64)
    above, _ = lf.decode_value((code + 1).clamp(max=511), meta, torch.float64)
    li = lf.group_params(meta, torch.float64)[0].unsqueeze(2).expand(-1, -1, 128).reshape(x.shape)
    inside = (a > 0) & (torch.log2(a.clamp(min=1e-300)) >= li)
    assert int(inside.sum()) > x.numel() // 2
    ok = (below <= a * (1 + 1e-6)) & ((a <= above * (1 + 1e-6)) | (code == 511))
    assert bool(ok[inside].all())
    # and the decode of the code itself is the nearer grid point: the codes split at the arithmetic mean of two
    # grid points, which lies log2((1 + 2^s) / 2) / s <= 0.5 + s * ln(2) / 8 < 0.506 steps above the lower one
    # (s <= 32 / 510); 2e-6 for the fp32 logarithms
    step = lf.group_params(meta, torch.float64)[1].unsqueeze(2).expand(-1, -1, 128).reshape(x.shape)
    v, _ = lf.decode_value(code, meta, torch.float64)
    nz = inside & (code > 0)
    assert bool(((torch.log2(v[nz]) - torch.log2(a[nz])).abs() <= step[nz] * 0.506 + 2e-6).all())
    # magnitudes more than 32 binades below amax, and zeros, get code 0
    assert bool((code[(a == 0)] == 0).all()) and int(code[2, 1:128].max()) == 0


def test_fp32_and_float64_stand_ins_agree_to_one_code():
    x = (torch.randn((64, 1024), generator=torch.Generator().manual_seed(2)) * 0.1).to(torch.bfloat16)
    c32, _, m32 = lf.encode_ref(x, torch.float32)
    c64, _, m64 = lf.encode_ref(x, torch.float64)
    assert torch.equal(m32, m64)
    assert int((c32 - c64).abs().max()) <= 1 and float((c32 != c64).float().mean()) < 1e-3


def test_degenerate_and_non_finite_groups_are_exact():
    x = torch.zeros((6, 256), dtype=torch.bfloat16)
    x[1, :128] = 2.5                                                   # amax == amin
    x[1, 128:] = torch.tensor([-0.75, 0.75]).repeat(64)                # ... with both signs
    x[2, :128] = torch.randn(128)
    x[2, 5] = float('inf')
    x[3, :128] = torch.randn(128)
    x[3, 7] = float('nan')
    x[4, :128] = lf.bits_bf16(torch.full((128,), 0x0040))              # bf16 denormals: zeros everywhere
    x[5, :128] = torch.tensor([0.0, -3.0]).repeat(64)                  # amin == 0 is not degenerate
    for dtype in (torch.float32, torch.float64):
        code, sign, meta = lf.encode_ref(x, dtype)
        y = lf.decode_ref(code, sign, meta, dtype)
        assert int(meta[0, 0]) == 0 and bool((code[0] == 0).all()) and bool((y[0] == 0).all())
        assert int(meta[1, 0]) == 0x4020 | 0x4020 << 16 and bool((code[1] == 1).all())
        assert same_bits(y[1], x[1])
        assert int(meta[2, 0]) & 0xffff == 0x7f80 and int(meta[3, 0]) & 0xffff > 0x7f80       # a NaN is never dropped
        assert bool(torch.isnan(y[2, :128]).all()) and bool(torch.isnan(y[3, :128]).all())
        assert bool((y[2, 128:] == 0).all())
        assert int(meta[4, 0]) == 0 and bool((y[4, :128] == 0).all())
        assert int(meta[5, 0]) == 0x4040 and same_bits(y[5, 1:128:2], x[5, 1:128:2]) and bool((y[5, 0:128:2] == 0).all())
    code, _, _ = lf.encode_ref(x)
    assert bool((code[5, 1:128:2] == 511).all())


def test_reference_tests_structured_input_decodes_exactly():
    """tests/legacy/test_low_latency.py: constant rows of rank - 128, the last 128 columns holding the token index."""
    hidden = 512
    for rank in (0, 3, 127, 129, 200):
        x = torch.full((40, hidden), float(rank - 128), dtype=torch.bfloat16)
        x[:, -128:] = torch.arange(40).view(-1, 1).to(torch.bfloat16)
        for dtype in (torch.float32, torch.float64):
            planes, meta = lf.cast_ref(x, dtype)
            assert same_bits(lf.cast_back_ref(planes, meta, dtype), x)


def test_plane_pack_round_trips_and_places_the_bits():
    g = torch.Generator().manual_seed(3)
    code = torch.randint(0, 512, (5, 256), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (5, 256), generator=g, dtype=torch.int32)
    planes = lf.pack_planes(code, sign)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (5, 320)
    c2, s2 = lf.unpack_planes(planes)
    assert torch.equal(c2, code) and torch.equal(s2, sign)
    c = 77
    assert int(planes[2, c]) == int(code[2, c]) & 0xff
    assert (int(planes[2, 256 + c // 4]) >> (2 * (c & 3))) & 3 == int(sign[2, c]) << 1 | int(code[2, c]) >> 8


def test_layout_sizes():
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    assert logfmt_row_layout(7168, 8) == (9344, 9216, 32) and packed_row_layout(7168, 8)[0] == 14464
    assert logfmt_row_layout(7168, 8, False) == (9216, 9216, 0)
    assert logfmt_row_layout(7168, 8, True, single=True) == (9344, 9216, 32)
    assert logfmt_row_layout(128, 3) == (256 + 128, 256, 32)                 # 164 coded bytes -> two lines
    assert lf.logfmt_row_bytes(7168) == 9184 <= logfmt_row_layout(7168, 8, False)[0]
    for hidden in (128, 384, 2176, 7168):
        rb, w_off, pad = logfmt_row_layout(hidden, 8)
        assert rb % 128 == 0 and w_off % 128 == 0 and w_off >= lf.logfmt_row_bytes(hidden) > w_off - 128
    with pytest.raises(RuntimeError):
        logfmt_row_layout(192, 8)


# ----------------------------------------------------------------------------- the entries, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


ENTRIES = ('deepep_cast_logfmt', 'deepep_cast_back_logfmt', 'deepep_logfmt_pack_rows', 'deepep_combine_reduce_logfmt')


def test_logfmt_entries_are_additive(lib):
    from deepep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f'int {name}(' in header
    assert 'internode_ll.cu:557-638' in header and 'internode_ll.cu:672-712' in header
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    # the epilogue's arguments: deepep_combine_reduce's without mode and units_per_block, with (meta, stride)
    assert len(_lib.SIGNATURES['deepep_combine_reduce_logfmt'][1]) == len(_lib.SIGNATURES['deepep_combine_reduce'][1])


def test_logfmt_entries_reject_bad_arguments_with_a_message(lib):
    def rejected(fn, args, text):
        assert fn(*args) == -1 and text in lib.deepep_amd_last_error(), (args, lib.deepep_amd_last_error())

    # 16-byte aligned fake pointers: nothing is dereferenced, every rejection comes before a launch
    rejected(lib.deepep_cast_logfmt, (4096, 384, 4, 192, 8192, 16384, None), b'128')
    rejected(lib.deepep_cast_logfmt, (4096, 512, 4, 256, None, 16384, None), b'pointers')
    rejected(lib.deepep_cast_logfmt, (4096, 500, 4, 256, 8192, 16384, None), b'row stride')
    assert lib.deepep_cast_logfmt(None, 0, 0, 256, None, None, None) == 0
    rejected(lib.deepep_cast_back_logfmt, (4096, 320, 8192, 2, 4, 200, 16384, None), b'128')
    rejected(lib.deepep_cast_back_logfmt, (4096, 304, 8192, 2, 4, 256, 16384, None), b'row stride')
    rejected(lib.deepep_cast_back_logfmt, (4096, 320, 8192, 1, 4, 256, 16384, None), b'meta row stride')
    rejected(lib.deepep_logfmt_pack_rows, (4096, 640, 512, 4, 256, 128, 8192, 384, 256, None), b'weight tail')
    rejected(lib.deepep_logfmt_pack_rows, (4096, 640, 512, 4, 192, 128, 8192, 512, 384, None), b'128')
    good = dict(weighted=0, src=4096, num_src_rows=8, src_row_stride=640, meta=8192, meta_row_stride=4,
                table=None, table_stride=0, table_width=1, row_weights=None, bias0=None, bias1=None,
                out=16384, out_row_stride=512, num_units=8, hidden=512, wtable=None, wtable_stride=0, wsrc=None,
                out_weights=None, num_weights=0, out_weights_stride=0, weights_pad=0, error_flag=None, stream=None)
    fn = lib.deepep_combine_reduce_logfmt
    rejected(fn, list(dict(good, hidden=192).values()), b'128')
    rejected(fn, list(dict(good, meta=None).values()), b'null')
    rejected(fn, list(dict(good, src_row_stride=624).values()), b'row stride')
    rejected(fn, list(dict(good, meta_row_stride=3).values()), b'row stride')
    rejected(fn, list(dict(good, weighted=1).values()), b'row weights')
    assert fn(*dict(good, num_units=0, src=None, meta=None).values()) == 0


def test_public_functions_refuse_bad_input_before_any_launch():
    import deepep_amd
    bad_x = (torch.zeros((4, 256)), torch.zeros((4, 192), dtype=torch.bfloat16), torch.zeros((256,), dtype=torch.bfloat16),
             torch.zeros((4, 256), dtype=torch.bfloat16), None)                  # the last tensor: not on the GPU
    for x in bad_x:
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_to_logfmt(x)
    planes, meta = torch.zeros((4, 320), dtype=torch.uint8), torch.zeros((4, 2), dtype=torch.int32)
    for p, m in ((planes.float(), meta), (planes, meta.long()), (planes[:, :300], meta), (planes[:3], meta),
                 (planes, meta[:, :1]), (planes, meta), (planes[0], meta)):      # the sixth pair: not on the GPU
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_back_logfmt(p, m)


# ----------------------------------------------------------------------------- combine(use_logfmt=True)
@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29581')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _buffer(group, kernels=None, hidden=H, **kw):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=hidden, num_topk=K, **kw)
    buf._kernels = Spy(kernels if kernels is not None else lf.LogfmtOracleKernels())
    return buf


class LossyPhaseA(lf.Fp8CombineOracleKernels):
    """A provider that knows nothing of LogFMT: its phase A (MODE_LOCAL) rows go through the stand-in's encode and
    decode where it wrote them.  The plain combine over it is what combine(use_logfmt=True) has to equal."""
    name = 'oracle-lossy-phase-a'

    def combine_reduce(self, mode, src, out, num_units, *args, **kw):
        from deepep_amd.kernels import MODE_LOCAL
        super().combine_reduce(mode, src, out, num_units, *args, **kw)
        if mode == MODE_LOCAL and num_units:
            rows = out[:num_units].contiguous()
            out[:num_units] = lf.cast_back_ref(*lf.cast_ref(rows))


def _expert_rows(n: int, seed: int) -> torch.Tensor:
    return (torch.randn((n, H), generator=torch.Generator().manual_seed(seed)) * 0.25).to(torch.bfloat16)


def test_flag_has_no_effect_at_one_rank_and_names_nothing_new(group):
    x, idx, w = routed_inputs(1, T, H, K, E)
    for amr in (True, False):
        buf = _buffer(group, allow_multiple_reduction=amr)
        recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
        y = _expert_rows(recv_x.shape[0], 4)
        kw = dict(topk_weights=recv_w) if amr else dict(topk_weights=recv_w, apply_topk_weights=True)
        want = buf.combine(y, handle, **kw)
        n0 = len(buf.kernels.calls)
        got = buf.combine(y, handle, use_logfmt=True, **kw)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        calls = buf.kernels.calls[n0:]
        assert [c[0] for c in calls] == ['combine_reduce'] and 'src_logfmt_meta' not in dict(calls[0][2])


def test_combine_refuses_before_any_kernel_call(group):
    _, idx, w = routed_inputs(2, T, 256, K, E)
    x = (torch.randn((T, 192), generator=torch.Generator().manual_seed(2))).to(torch.bfloat16)
    buf = _buffer(group, hidden=192)
    recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    n0 = len(buf.kernels.calls)
    with pytest.raises(RuntimeError, match='use_logfmt needs hidden % 128 == 0'):
        buf.combine(recv_x, handle, topk_weights=recv_w, use_logfmt=True)
    assert len(buf.kernels.calls) == n0
    buf.combine(recv_x, handle, topk_weights=recv_w)                        # the call without the flag stays legal
    with pytest.raises(TypeError):
        buf.combine(recv_x, handle, recv_w, None, 0, 0, None, None, False, False, False, True)   # keyword-only


def _rank_thread(rank, comm, bypass, xgmi, results):
    try:
        fails = []
        x, idx, w = routed_inputs(10 + rank, T, H, K, E)
        from deepep_amd.handle import logfmt_row_layout, packed_row_layout
        for amr in (True, False):
            outs = []
            for provider in (lf.LogfmtOracleKernels(), LossyPhaseA()):
                buf = _buffer(FakeGroup(rank, comm.n, comm), provider, allow_multiple_reduction=amr)
                sizes = []

                def a2a(out, inp, os_=None, is_=None, sizes=sizes):
                    sizes.append(inp.shape[1] * inp.element_size())
                    comm.a2a(rank, out, inp, os_, is_)
                buf._a2a = a2a
                buf.local_bypass = bypass
                if xgmi:
                    buf.transport = 'xgmi'
                recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E,
                                                            do_expand=True)
                y = _expert_rows(recv_x.shape[0], 30 + rank)
                b0 = _expert_rows(T, 50 + rank)
                flag = isinstance(provider, lf.LogfmtOracleKernels)
                cases = [dict(topk_weights=recv_w), dict(topk_weights=recv_w, bias=(b0, b0)), dict()] if amr else \
                    [dict(topk_weights=recv_w, apply_topk_weights=True), dict(bias=b0)]
                for kw in cases:
                    del sizes[:]
                    n0 = len(buf.kernels.calls)
                    if xgmi and flag:
                        try:
                            buf.combine(y, handle, use_logfmt=True, **kw)
                            fails.append('no refusal over xgmi')
                        except RuntimeError as e:
                            if 'window transport' not in str(e) or len(buf.kernels.calls) != n0:
                                fails.append(f'xgmi refusal: {e}, {buf.kernels.names()[n0:]}')
                        continue
                    if xgmi:
                        continue
                    outs.append(buf.combine(y, handle, **(dict(use_logfmt=True) if flag else {}), **kw))
                    with_w = 'topk_weights' in kw
                    layout = logfmt_row_layout if flag else packed_row_layout
                    want = layout(H, K, with_w) if amr else layout(H, 1, with_w, single=True)
                    if not sizes or any(s != want[0] for s in sizes):
                        fails.append(f'{provider.name} amr={amr} {sorted(kw)}: all-to-all rows of {sizes} bytes, '
                                     f'not {want[0]}')
                    names = buf.kernels.names()[n0:]
                    if flag and ('logfmt_pack_rows' not in names or not any(
                            'src_logfmt_meta' in dict(c[2]) for c in buf.kernels.calls[n0:])):
                        fails.append(f'amr={amr}: the flag made the calls {names}')
                    if not flag and any('logfmt' in n for n in names):
                        fails.append(f'amr={amr}: a call without the flag made the calls {names}')
            half = len(outs) // 2
            for i in range(half):
                got, want = outs[i], outs[half + i]
                if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
                    fails.append(f'amr={amr} case {i}: use_logfmt differs from the stand-in composition')
                if not bool(torch.isfinite(want[0].float()).all()):
                    fails.append('wrongly chosen input')
        results[rank] = fails
    except Exception:
        results[rank] = [traceback.format_exc()]
        comm.bar.abort()


def _run(world, bypass, xgmi=False):
    comm = CpuComm(world)
    results = {}
    threads = [threading.Thread(target=_rank_thread, args=(r, comm, bypass, xgmi, results)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert sorted(results) == list(range(world))
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad


@pytest.mark.parametrize('world, bypass', [(2, True), (4, True), (4, False)])
def test_use_logfmt_equals_the_stand_in_composition(world, bypass):
    _run(world, bypass)


def test_xgmi_transport_refuses_the_flag_before_any_launch():
    _run(2, True, xgmi=True)
