"""ElasticBuffer.combine((x_fp8, x_scales), handle, ...) on the CPU stand-in (tests/fp8_combine_ref.py), at one rank
and over 4 thread ranks: the pair combine returns, bit for bit, what the combine of the cast-back rows returns.  Also:
the rejections come before any wrapper call, a bf16 x makes the wrapper calls it made before the pair existed (no
`src_sf` key anywhere), and deepep_combine_reduce_fp8 / deepep_combine_reduce_scatter_fp8 are exported, declared,
prototyped, documented and reject bad arguments without a GPU."""
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp8_combine_ref import (Fp8CombineOracleKernels, back_cpu, binade_rows, combine_differences,
                                   pair_combine_cases, pair_forms, routed_inputs)
from tests.fp8_oracle_kernels import Spy
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 512, 3, 8


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29578')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _buffer(group, **kw):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, **kw)
    buf._kernels = Spy(Fp8CombineOracleKernels())
    return buf


# ----------------------------------------------------------------------------- one rank
def test_pair_combine_equals_cast_back_route_one_rank(group):
    buf, single = _buffer(group), _buffer(group, allow_multiple_reduction=False)
    fails = pair_combine_cases(buf, routed_inputs(1, T, H, K, E), routed_inputs(2, 0, H, K, E), E, back_cpu,
                               single=single)
    assert not fails, fails
    assert 'combine_reduce' in buf.kernels.names() and 'combine_reduce' in single.kernels.names()


def test_independent_expert_rows_one_rank(group):
    """Expert rows that are not copies of the dispatched tokens (every slot its own row, so the order of the sum
    shows), in the three scale-factor forms."""
    buf = _buffer(group)
    x, idx, w = routed_inputs(3, T, H, K, E)
    recv_x, _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
    forms = pair_forms(binade_rows(recv_x.shape[0], H, 4))
    assert sorted(forms) == ['col_major', 'fp32', 'ue8m0']
    for name, pair in forms.items():
        for kw in (dict(), dict(apply_topk_weights=True)):
            bad = combine_differences(buf, pair, handle, back_cpu, topk_weights=recv_w, **kw)
            assert not bad, (name, kw, bad)


def test_rejections_come_before_any_wrapper_call(group):
    buf = _buffer(group)
    x, idx, w = routed_inputs(5, T, H, K, E)
    (q, sf), _, recv_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True,
                                                 cast_to_fp8=True)
    n = q.shape[0]
    before = len(buf.kernels.calls)
    wide = torch.zeros((n, H + 64), dtype=torch.uint8).view(torch.float8_e4m3fn)
    bad_pairs = (('first member not float8', (q.view(torch.uint8), sf)),
                 ('bf16 first member', (q.to(torch.bfloat16), sf)),
                 ('1-D rows', (q[0], sf)),
                 ('rows not contiguous', (wide[:, :H], sf)),
                 ('H % 128 != 0', (q[:, :192].contiguous(), sf[:, :2].contiguous())),
                 ('float64 factors', (q, sf.double())),
                 ('factor shape', (q, sf[:, :-1])),
                 ('factor rows', (q, sf[:-1])),
                 ('int32 factors, H % 512 != 0', (q[:, :384].contiguous(), torch.zeros((n, 1), dtype=torch.int32))),
                 ('int32 factor shape', (q, torch.zeros((n, H // 128), dtype=torch.int32))),
                 ('factors on another device', (q, sf.to('meta'))),
                 ('a triple', (q, sf, sf)),
                 ('not tensors', (q, None)))
    for what, pair in bad_pairs:
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.combine(pair, handle, topk_weights=recv_w)
        assert len(buf.kernels.calls) == before, what
    assert not combine_differences(buf, (q, sf), handle, back_cpu, topk_weights=recv_w)


def test_bf16_x_makes_the_wrapper_calls_it_made_before(group):
    """With a bf16 x no wrapper call carries a `src_sf` key, at one rank in both reduction modes: a provider that
    does not know the keyword (tests/oracle_kernels.OracleKernels) serves every such call."""
    from tests.oracle_kernels import OracleKernels
    x, idx, w = routed_inputs(6, T, H, K, E)
    for amr in (True, False):
        buf = _buffer(group, allow_multiple_reduction=amr)
        plain = _buffer(group, allow_multiple_reduction=amr)
        plain._kernels = Spy(OracleKernels())                  # its combine_reduce has no src_sf parameter
        outs = []
        for b in (buf, plain):
            recv_x, _, recv_w, handle, _ = b.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True)
            before = len(b.kernels.calls)
            kw = dict(topk_weights=recv_w, apply_topk_weights=True) if not amr else dict(topk_weights=recv_w)
            outs.append(b.combine(recv_x, handle, **kw))
            calls = b.kernels.calls[before:]
            assert calls and all('src_sf' not in dict(c[2]) for c in calls)
            outs.append(calls)
        assert torch.equal(outs[0][0], outs[2][0]) and outs[1] == outs[3]


# ----------------------------------------------------------------------------- 4 thread ranks
def _rank_thread(rank, comm, bypass, results):
    try:
        bufs = []
        for amr in (True, False):
            buf = _buffer(FakeGroup(rank, comm.n, comm), allow_multiple_reduction=amr)
            buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
            buf.local_bypass = bypass
            bufs.append(buf)
        fails = pair_combine_cases(bufs[0], routed_inputs(10 + rank, T, H, K, E),
                                   routed_inputs(20 + rank, 0 if rank == 1 else T, H, K, E), E, back_cpu,
                                   single=bufs[1])
        plain = [c for b in bufs for c in b.kernels.calls if c[0] == 'combine_reduce' and 'src_sf' not in dict(c[2])]
        if not plain:
            fails.append('phase B never ran as a bf16 call')
        results[rank] = fails
    except Exception:
        results[rank] = [traceback.format_exc()]
        comm.bar.abort()


@pytest.mark.parametrize('bypass', [True, False])
def test_pair_combine_equals_cast_back_route_four_ranks(bypass):
    comm = CpuComm(4)
    results = {}
    threads = [threading.Thread(target=_rank_thread, args=(r, comm, bypass, results)) for r in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert sorted(results) == [0, 1, 2, 3]
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad


# ----------------------------------------------------------------------------- the two entries, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


ENTRIES = ('deepep_combine_reduce_fp8', 'deepep_combine_reduce_scatter_fp8')


def test_fp8_combine_entries_are_exported_declared_prototyped_and_documented(lib):
    from deepep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert f'int {name}(' in header and f'`{name}`' in integration
        sibling = name[:-len('_fp8')]
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[sibling][1]) + 4
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays


def _reduce_args(**kw):
    # 16-byte aligned fake pointers: nothing is dereferenced, every rejection comes before a launch
    good = dict(mode=2, weighted=0, src=4096, num_src_rows=8, src_row_stride=512,
                sf=8192, sf_row_stride=4, sf_col_stride=1, sf_packed=0,
                table=None, table_stride=0, table_width=1, row_weights=None, bias0=None, bias1=None,
                out=16384, out_row_stride=512, num_units=8, hidden=512,
                wtable=None, wtable_stride=0, wsrc=None, out_weights=None, num_weights=0,
                out_weights_stride=0, weights_pad=0, units_per_block=0, error_flag=None, stream=None)
    assert set(kw) <= set(good)
    return list(dict(good, **kw).values())


def _scatter_args(**kw):
    good = dict(weighted=0, src=4096, num_src_rows=8, src_row_stride=512,
                sf=8192, sf_row_stride=4, sf_col_stride=1, sf_packed=0,
                table=None, table_stride=0, table_width=1, row_weights=None,
                out_rows=32768, num_units=8, hidden=512, wtable=None, wtable_stride=0, wsrc=None, num_weights=0,
                weights_offset=0, weights_pad=0, window_bases=65536, num_windows=1, window_bytes=1 << 20,
                error_flag=None, stream=None)
    assert set(kw) <= set(good)
    return list(dict(good, **kw).values())


@pytest.mark.parametrize('entry, args', [(ENTRIES[0], _reduce_args), (ENTRIES[1], _scatter_args)])
def test_fp8_combine_entries_reject_bad_arguments_with_a_message(lib, entry, args):
    fn = getattr(lib, entry)

    def rejected(text, **kw):
        assert fn(*args(**kw)) == -1, kw
        assert text in lib.deepep_amd_last_error(), (kw, lib.deepep_amd_last_error())

    rejected(b'128', hidden=192, src_row_stride=192)
    rejected(b'512', hidden=384, src_row_stride=384, sf_packed=1)
    rejected(b'scale factors', sf=None)
    rejected(b'scale factors', sf=8194)
    rejected(b'16-byte aligned', src=4104)
    rejected(b'row stride', src_row_stride=520)
    rejected(b'row stride', src_row_stride=256)
    assert fn(*args(num_units=0, src=None, sf=None)) == 0                  # no units: nothing to do, no launch
    assert fn(*args(num_units=-1)) == -1
