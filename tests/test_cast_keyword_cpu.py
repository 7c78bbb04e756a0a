"""ElasticBuffer.dispatch(..., cast_to_fp8=True) on the CPU stand-in, at one rank and over 4 thread ranks: the
keyword dispatch of a bf16 x returns, bit for bit, what the tuple dispatch of the CPU-cast pair
(tests/test_fp8_cast_gpu.cast_ref) returns with the other arguments equal -- rows, scale factors, routing,
weights and every handle field.  Also: the rejections come before any wrapper call, the flag-off path makes the
wrapper calls it made before the keyword existed, and deepep_cast_back_fp8 / deepep_amd.per_token_cast_back are
exported, declared, prototyped and reject bad arguments without a GPU."""
import os
import socket
import subprocess
import sys
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp8_oracle_kernels import CAST_WRAPPERS, Fp8OracleKernels, Spy, keyword_cases
from tests.sim import FakeGroup
from tests.test_fp8_cast_gpu import cast_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 256, 3, 8


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29572')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(rank: int, tokens: int = T):
    """bf16 rows, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(100 + rank)
    x = (torch.randn((tokens, H), generator=g) * 3).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x, idx.to(topk_idx_t), w


def _buffer(group):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = Spy(Fp8OracleKernels())
    return buf


def _keyword_cases(buf, rank: int, empty_rank: int = 0):
    return keyword_cases(buf, _inputs(rank), _inputs(rank, 0 if rank == empty_rank else T), E)


# ----------------------------------------------------------------------------- one rank
def test_keyword_equals_tuple_dispatch_one_rank(group):
    buf = _buffer(group)
    fails = _keyword_cases(buf, 0)
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names


def test_rejections_come_before_any_wrapper_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for what, xin, kw in (('a tuple x', cast_ref(x), dict(cast_to_fp8=True)),
                          ('a dtype other than bf16', x.float(), dict(cast_to_fp8=True)),
                          ('H % 128 != 0', x[:, :192].contiguous(), dict(cast_to_fp8=True)),
                          ('fp8_round_scale alone', x, dict(fp8_round_scale=True))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.dispatch(xin, **kw, **base)
        assert buf.kernels.calls == [], what


def test_flag_off_makes_the_same_wrapper_calls(group):
    """Omitting the keywords and passing cast_to_fp8=False record the same wrapper calls (names, argument shapes
    and dtypes), for a bf16 x and for the FP8 pair, fresh and cached; no cast wrapper is among them."""
    x, idx, w = _inputs(0)
    for xin in (x, cast_ref(x)):
        for more in (dict(), dict(do_expand=True, expert_alignment=16, do_zero_padding=True), dict(do_cpu_sync=False)):
            recorded = []
            for flags in (dict(), dict(cast_to_fp8=False, fp8_round_scale=False)):
                buf = _buffer(group)
                handle = buf.dispatch(xin, topk_idx=idx, topk_weights=w, num_experts=E, **more, **flags)[3]
                buf.dispatch(xin, handle=handle, do_expand=handle.do_expand, **flags)
                recorded.append(buf.kernels.calls)
            assert recorded[0] == recorded[1] and recorded[0]
            assert not set(c[0] for c in recorded[0]) & set(CAST_WRAPPERS)
            assert [c[0] for c in recorded[0]].count('dispatch_copy') == 2


def test_routing_width_matches_the_environment():
    from deepep_amd import topk_idx_t
    assert topk_idx_t == (torch.int32 if os.environ.get('EP_NUM_TOPK_IDX_BITS') == '32' else torch.int64)


def test_keyword_with_32_bit_routing():
    """EP_NUM_TOPK_IDX_BITS is read when deepep_amd is imported: the one-rank cases again in a fresh process with
    int32 routing (the stand-in asserts, as the HIP wrappers do, that the casting wrappers get int64 routing)."""
    with socket.socket() as sock:                              # this process may hold the fixture's own port
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, EP_NUM_TOPK_IDX_BITS='32', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    here = os.path.relpath(os.path.abspath(__file__), ROOT)
    run = subprocess.run([sys.executable, '-m', 'pytest', '-q',
                          f'{here}::test_routing_width_matches_the_environment',
                          f'{here}::test_keyword_equals_tuple_dispatch_one_rank'],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and '2 passed' in run.stdout, run.stdout[-3000:] + run.stderr[-1000:]


# ----------------------------------------------------------------------------- 4 thread ranks
class CpuComm:
    """all_to_all_single among threads that each drive one rank on the CPU (tests/sim.ThreadComm without streams)."""

    def __init__(self, n: int):
        self.n = n
        self.bar = threading.Barrier(n, timeout=120)
        self.slots = [None] * n

    def a2a(self, rank, out, inp, out_splits=None, in_splits=None):
        splits = in_splits if in_splits is not None else [inp.shape[0] // self.n] * self.n
        self.slots[rank] = (inp, splits)
        self.bar.wait()
        pos = 0
        for s in range(self.n):
            sinp, ssplits = self.slots[s]
            start, cnt = sum(ssplits[:rank]), ssplits[rank]
            out[pos:pos + cnt].copy_(sinp[start:start + cnt])
            pos += cnt
        assert pos == out.shape[0], (pos, out.shape)
        self.bar.wait()


def _rank_thread(rank, comm, bypass, results):
    try:
        buf = _buffer(FakeGroup(rank, comm.n, comm))
        buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
        buf.local_bypass = bypass
        fails = _keyword_cases(buf, rank, empty_rank=1)
        names = buf.kernels.names()
        if 'dispatch_pack_cast' not in names or 'dispatch_copy_cast' in names or 'cast_fp8' in names:
            fails.append(f'EP > 1 casts in the pack only, got {sorted(set(names))}')
        results[rank] = fails
    except Exception:
        results[rank] = [traceback.format_exc()]
        comm.bar.abort()


@pytest.mark.parametrize('bypass', [True, False])
def test_keyword_equals_tuple_dispatch_four_ranks(bypass):
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


# ----------------------------------------------------------------------------- the cast back, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_cast_back_entry_is_exported_declared_and_prototyped(lib):
    import deepep_amd
    from deepep_amd import _lib
    from deepep_amd.kernels import HipKernels
    assert hasattr(lib, 'deepep_cast_back_fp8') and 'deepep_cast_back_fp8' in _lib.SIGNATURES
    assert 'int deepep_cast_back_fp8(' in open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    assert 'per_token_cast_back' in deepep_amd.__all__ and callable(deepep_amd.per_token_cast_back)
    assert callable(getattr(HipKernels, 'cast_back_fp8'))
    # 16-byte aligned fake pointers: nothing is dereferenced, every rejection comes before a launch
    good = dict(q=16, q_stride=128, sf=32, sf_row=1, sf_col=1, rows=4, hidden=128, out=48, stream=None)

    def call(**kw):
        return lib.deepep_cast_back_fp8(*dict(good, **kw).values())

    assert call(hidden=192, q_stride=192) == -1 and b'128' in lib.deepep_amd_last_error()
    assert call(hidden=0) == -1 and call(rows=-1) == -1
    assert call(q=None) == -1 and call(out=None) == -1 and call(sf=None) == -1
    assert call(q=24) == -1 and call(out=56) == -1 and call(sf=34) == -1 and b'aligned' in lib.deepep_amd_last_error()
    assert call(q_stride=112) == -1 and b'stride' in lib.deepep_amd_last_error()
    assert call(q_stride=136) == -1                                        # not 16-byte aligned
    assert call(sf_row=-1) == -1 and call(sf_col=-1) == -1
    assert call(rows=0, q=None, sf=None, out=None) == 0                    # no rows: nothing to do


def test_public_cast_back_rejects_bad_arguments_before_loading_the_library(monkeypatch):
    import deepep_amd
    from deepep_amd import _lib

    def no_load(*a, **kw):
        raise AssertionError('the library was loaded')

    monkeypatch.setattr(_lib, 'load', no_load)
    q = torch.zeros((4, 256), dtype=torch.float8_e4m3fn)
    sf = torch.ones((4, 2), dtype=torch.float32)
    for what, args in (('not a tensor', (None, sf)),
                       ('bf16 rows', (q.to(torch.bfloat16), sf)),
                       ('1-D rows', (q[0], sf)),
                       ('H % 128 != 0', (q[:, :192], sf)),
                       ('packed UE8M0 scale factors', (q, torch.zeros((4, 2), dtype=torch.int32))),
                       ('scale factor shape', (q, torch.ones((4, 3), dtype=torch.float32))),
                       ('1-D scale factors', (q, torch.ones((8,), dtype=torch.float32)))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_back(*args)
    with pytest.raises(RuntimeError, match='UE8M0'):
        deepep_amd.per_token_cast_back(q, torch.zeros((4, 2), dtype=torch.int32))
    # no rows: an empty bf16 tensor, no launch and no library
    out = deepep_amd.per_token_cast_back(q[:0], sf[:0])
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 256)
