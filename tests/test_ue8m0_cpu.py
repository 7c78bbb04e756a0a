"""Packed UE8M0 scale factors without a GPU: the torch reference of the packed form (tests/ue8m0_ref.pack_ref /
unpack_ref); ElasticBuffer.dispatch(..., cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True) on the CPU
stand-in, at one rank and over 4 thread ranks, against the tuple dispatch of (cast_ref q, pack_ref sf) -- bit for
bit, every handle field and the scale-factor strides included; the rejections before any wrapper call; the flag-off
wrapper calls; the four C-ABI entries exported, prototyped, declared and rejecting bad arguments before a launch; and
the argument checks of the two public functions."""
import inspect
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp8_oracle_kernels import CAST_WRAPPERS, Fp8OracleKernels, Spy
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm
from tests.test_fp8_cast_gpu import cast_ref
from tests.ue8m0_ref import UE8M0, Ue8m0OracleKernels, pack_ref, ue8m0_cases, ue8m0_pair, unpack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 512, 3, 8
ENTRIES = ('deepep_cast_fp8_ue8m0', 'deepep_cast_back_fp8_ue8m0', 'deepep_dispatch_pack_cast_ue8m0',
           'deepep_dispatch_copy_cast_ue8m0')


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29576')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(rank: int, tokens: int = T, hidden: int = H):
    """bf16 rows, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(300 + rank)
    x = (torch.randn((tokens, hidden), generator=g) * 3).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x, idx.to(topk_idx_t), w


def _buffer(group, kernels=Ue8m0OracleKernels):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = Spy(kernels())
    return buf


# ----------------------------------------------------------------------------- the packed form
def test_pack_and_unpack_round_trip_over_every_exponent_byte():
    exp = torch.arange(1, 255, dtype=torch.int32)
    exp = torch.cat([exp, exp[:2]]).view(2, 128)               # 256 = 2 rows of 128 groups
    sf = (exp << 23).view(torch.float32)
    assert bool(((sf > 0) & sf.isfinite()).all())
    packed = pack_ref(sf)
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (2, 32)
    # byte j (little-endian) of element p is group 4p + j
    assert packed[0, 0].item() == 1 | 2 << 8 | 3 << 16 | 4 << 24
    assert torch.equal(packed.view(torch.uint8).view(2, 128).to(torch.int32), exp)
    back = unpack_ref(packed)
    assert back.dtype == torch.float32 and torch.equal(back.view(torch.int32), sf.view(torch.int32))
    assert torch.equal(pack_ref(back), packed)
    # any strides: the column-major tensor unpacks to the same factors
    col = torch.empty_strided((2, 32), (1, 4), dtype=torch.int32)
    col.copy_(packed)
    assert torch.equal(unpack_ref(col).view(torch.int32), sf.view(torch.int32))
    assert unpack_ref(torch.zeros((1, 1), dtype=torch.int32)).view(torch.int32).eq(0).all()      # byte 0: +0.0f


def test_the_pack_of_the_cast_unpacks_to_itself():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((9, 1536), generator=g) * 3).to(torch.bfloat16)
    x[0, :128] = 0                                             # the 1e-4 clamp: the smallest exponent byte
    x[1, 128:256] = torch.finfo(torch.bfloat16).max            # the largest finite bf16: the largest
    x[2, 256:384] = 448.0                                      # amax / 448 an exact power of two
    q, sf = cast_ref(x, True)
    packed = pack_ref(sf)
    assert tuple(packed.shape) == (9, 3)
    assert torch.equal(unpack_ref(packed).view(torch.int32), sf.view(torch.int32))
    exp = packed.view(torch.uint8)
    assert int(exp.min()) == 105 and int(exp.max()) == 247     # 0 and 255 never come out of the cast
    assert exp.view(9, 12)[2, 2].item() == 127                 # 448 / 448 = 2^0


# ----------------------------------------------------------------------------- one rank
def test_keyword_equals_tuple_dispatch_one_rank(group):
    buf = _buffer(group)
    fails = ue8m0_cases(buf, _inputs(0), _inputs(0, 0), E)
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names
    flagged = [c for c in buf.kernels.calls if c[0] == 'dispatch_copy_cast']
    assert flagged and all(dict(c[2]).get('ue8m0') is True and dict(c[2]).get('round_scale') is True for c in flagged)


def test_rejections_come_before_any_wrapper_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for what, xin, kw in (('fp8_use_ue8m0 alone', x, dict(fp8_use_ue8m0=True)),
                          ('without fp8_round_scale', x, dict(cast_to_fp8=True, fp8_use_ue8m0=True)),
                          ('without cast_to_fp8', ue8m0_pair(x), dict(fp8_use_ue8m0=True)),
                          ('H % 512 != 0', x[:, :384].contiguous(), UE8M0),
                          ('a tuple x', ue8m0_pair(x), UE8M0)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.dispatch(xin, **kw, **base)
        assert buf.kernels.calls == [], what
    params = list(inspect.signature(type(buf).dispatch).parameters.values())
    assert params[-1].name == 'fp8_use_ue8m0' and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and \
        params[-1].default is False                            # keyword-only, last, off


def test_flag_off_makes_the_same_wrapper_calls(group):
    """With fp8_use_ue8m0 absent and with it False the wrapper calls (names, argument shapes, dtypes and values) are
    the same and no wrapper is handed a `ue8m0` keyword -- on a provider that does not know it."""
    x, idx, w = _inputs(0)
    for xin, flags in ((x, dict()), (cast_ref(x), dict()), (ue8m0_pair(x), dict()),
                       (x, dict(cast_to_fp8=True)), (x, dict(cast_to_fp8=True, fp8_round_scale=True))):
        for more in (dict(), dict(do_expand=True, expert_alignment=16, do_zero_padding=True), dict(do_cpu_sync=False)):
            recorded = []
            for off in (dict(), dict(fp8_use_ue8m0=False)):
                buf = _buffer(group, Fp8OracleKernels)
                handle = buf.dispatch(xin, topk_idx=idx, topk_weights=w, num_experts=E, **more, **flags, **off)[3]
                buf.dispatch(xin, handle=handle, do_expand=handle.do_expand, **flags, **off)
                recorded.append(buf.kernels.calls)
            assert recorded[0] == recorded[1] and recorded[0]
            assert not any('ue8m0' in dict(c[2]) for c in recorded[0])
            if not flags:
                assert not set(c[0] for c in recorded[0]) & set(CAST_WRAPPERS)


# ----------------------------------------------------------------------------- 4 thread ranks
def _rank_thread(rank, comm, bypass, results):
    try:
        buf = _buffer(FakeGroup(rank, comm.n, comm))
        buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
        buf.local_bypass = bypass
        fails = ue8m0_cases(buf, _inputs(rank), _inputs(rank, 0 if rank == 1 else T), E)
        names = buf.kernels.names()
        if 'dispatch_pack_cast' not in names or 'dispatch_copy_cast' in names or 'cast_fp8' in names:
            fails.append(f'EP > 1 casts in the pack only, got {sorted(set(names))}')
        if not all(dict(c[2]).get('ue8m0') is True for c in buf.kernels.calls if c[0] == 'dispatch_pack_cast'):
            fails.append('a casting pack without ue8m0')
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


# ----------------------------------------------------------------------------- the C-ABI, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_entries_are_exported_prototyped_declared_and_documented(lib):
    from deepep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f'int {name}(' in header and f'`{name}`' in integration, name
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays


def _rejects(lib, name, good, cases):
    """Every case (argument overrides) returns DEEPEP_ERR_INVALID_ARG; the pointers are fake (nothing is dereferenced:
    every rejection comes before a launch), so the good arguments themselves are never passed."""
    fn = getattr(lib, name)
    for kw in cases:
        assert set(kw) <= set(good), kw
        assert fn(*dict(good, **kw).values()) == -1, (name, kw)


def test_entries_reject_bad_arguments_before_a_launch(lib):
    from deepep_amd.kernels import RowLayout
    err = lib.deepep_amd_last_error
    good = dict(x=16, stride=1024, rows=4, hidden=512, q=32, sf=52, stream=None)
    _rejects(lib, 'deepep_cast_fp8_ue8m0', good, [dict(hidden=768, stride=1536)])
    assert b'512' in err() and b'cast_fp8_ue8m0' in err()
    _rejects(lib, 'deepep_cast_fp8_ue8m0', good, [dict(hidden=128), dict(hidden=0), dict(rows=-1), dict(x=None),
                                                  dict(q=None), dict(sf=None), dict(x=24), dict(q=40), dict(sf=54)])
    assert b'aligned' in err()
    _rejects(lib, 'deepep_cast_fp8_ue8m0', good, [dict(stride=1008), dict(stride=1032)])
    assert b'stride' in err()
    assert lib.deepep_cast_fp8_ue8m0(*dict(good, rows=0, x=None, q=None, sf=None).values()) == 0

    good = dict(q=16, q_stride=512, sf=36, sf_row=1, sf_col=1, rows=4, hidden=512, out=48, stream=None)
    _rejects(lib, 'deepep_cast_back_fp8_ue8m0', good, [dict(hidden=768, q_stride=768)])
    assert b'512' in err() and b'cast_back_fp8_ue8m0' in err()
    _rejects(lib, 'deepep_cast_back_fp8_ue8m0', good,
             [dict(hidden=256), dict(hidden=0), dict(rows=-1), dict(q=None), dict(out=None), dict(sf=None),
              dict(q=24), dict(out=56), dict(sf=38), dict(q_stride=496), dict(q_stride=520), dict(sf_row=-1),
              dict(sf_col=-1)])
    assert lib.deepep_cast_back_fp8_ue8m0(*dict(good, rows=0, q=None, sf=None, out=None).values()) == 0

    lay = RowLayout.make(512, 4, K)
    good = dict(x=16, stride=1024, hidden=512, idx=64, w=None, tokens=4, topk=K, src_base=0, dst_slot=128,
                send_offsets=256, ranks=1, packed=512, dest_bases=None, row_bytes=lay.row_bytes, dest_rows=4,
                sf_off=lay.sf_off, idx_off=lay.idx_off, w_off=lay.w_off, src_off=lay.src_off, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_pack_cast_ue8m0', good, [dict(hidden=768, stride=1536)])
    assert b'512' in err() and b'dispatch_pack_cast_ue8m0' in err()
    _rejects(lib, 'deepep_dispatch_pack_cast_ue8m0', good,
             [dict(hidden=384, stride=768), dict(x=None), dict(x=24), dict(stride=1016), dict(packed=520),
              dict(sf_off=510), dict(sf_off=508), dict(idx_off=lay.sf_off), dict(topk=0), dict(ranks=65),
              dict(row_bytes=lay.src_off)])
    assert lib.deepep_dispatch_pack_cast_ue8m0(*dict(good, tokens=0).values()) == 0

    good = dict(packed=16, row_bytes=128, w_off=0, recv=4, topk=K, meta=64, expanded=0, x=128, stride=1024, hidden=512,
                max_tokens=4, recv_x=256, recv_sf=516, recv_w=None, out_rows=4, inv=None, offsets=None, end=None,
                experts=0, row_map=None, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_copy_cast_ue8m0', good, [dict(hidden=768, stride=1536)])
    assert b'512' in err() and b'dispatch_copy_cast_ue8m0' in err()
    _rejects(lib, 'deepep_dispatch_copy_cast_ue8m0', good,
             [dict(hidden=128, stride=256), dict(x=None), dict(x=136), dict(stride=1016), dict(recv_x=None),
              dict(recv_x=264), dict(recv_sf=None), dict(recv_sf=518), dict(meta=None), dict(max_tokens=0),
              dict(inv=1024)])
    assert lib.deepep_dispatch_copy_cast_ue8m0(*dict(good, recv=0).values()) == 0


# ----------------------------------------------------------------------------- the public functions
class _Loaded(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    from deepep_amd import _lib

    def no_load(*a, **kw):
        raise _Loaded()

    monkeypatch.setattr(_lib, 'load', no_load)


def test_public_cast_checks_its_arguments_before_loading_the_library(no_library):
    import deepep_amd
    x = torch.zeros((4, 512), dtype=torch.bfloat16)
    for what, args, kw in (('use_ue8m0 without round_scale', (x,), dict(use_ue8m0=True)),
                           ('H % 512 != 0', (x[:, :384],), dict(round_scale=True, use_ue8m0=True)),
                           ('H % 128 != 0', (x[:, :448],), dict(round_scale=True, use_ue8m0=True)),
                           ('float rows', (x.float(),), dict(round_scale=True, use_ue8m0=True))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_to_fp8(*args, **kw)
    with pytest.raises(_Loaded):                               # well-formed: on to the library
        deepep_amd.per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True)


def test_public_cast_back_takes_well_shaped_packed_scale_factors_only(no_library):
    import deepep_amd
    q = torch.zeros((4, 1024), dtype=torch.float8_e4m3fn)
    with pytest.raises(_Loaded):                               # past the dtype and shape checks
        deepep_amd.per_token_cast_back(q, torch.zeros((4, 2), dtype=torch.int32))
    with pytest.raises(_Loaded):                               # any strides
        deepep_amd.per_token_cast_back(q, torch.zeros((2, 4), dtype=torch.int32).t())
    q256 = torch.zeros((4, 256), dtype=torch.float8_e4m3fn)
    for what, args in (('a wrong shape', (q, torch.zeros((4, 8), dtype=torch.int32))),
                       ('a wrong row count', (q, torch.zeros((3, 2), dtype=torch.int32))),
                       ('1-D', (q, torch.zeros((8,), dtype=torch.int32))),
                       ('H = 256', (q256, torch.zeros((4, 2), dtype=torch.int32))),
                       ('H = 256, no element', (q256, torch.zeros((4, 0), dtype=torch.int32))),
                       ('H = 640', (torch.zeros((4, 640), dtype=torch.float8_e4m3fn),
                                    torch.zeros((4, 1), dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match='Assertion failed') as info:
            deepep_amd.per_token_cast_back(*args)
        assert 'UE8M0' in str(info.value), what
    for dtype in (torch.int64, torch.uint8, torch.float16):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_back(q, torch.zeros((4, 2), dtype=dtype))
    out = deepep_amd.per_token_cast_back(q[:0], torch.zeros((0, 2), dtype=torch.int32))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 1024)
