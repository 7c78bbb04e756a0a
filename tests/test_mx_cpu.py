"""MXFP8 (fp8_group_size=32) without a GPU: the oracle pair (tests/mx_ref.mx_pair) against a direct per-32 restatement
of the rule; ElasticBuffer.dispatch(..., cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True,
fp8_group_size=32) on the CPU stand-in, at one rank and over 4 thread ranks, against the tuple dispatch of mx_pair(x)
-- bit for bit, every handle field and the scale-factor strides included; the rejections before any kernel call; the
four C-ABI entries exported, prototyped, declared, documented and rejecting bad arguments before a launch; and the
argument checks of the two public functions."""
import inspect
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp8_oracle_kernels import Spy
from tests.mx_ref import MX, MxOracleKernels, mx_back_ref, mx_cases, mx_factors, mx_pair
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm
from tests.test_fp8_cast_gpu import cast_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 384, 3, 8              # 384: no multiple of 512, three dwords of exponent bytes a row
ENTRIES = ('deepep_cast_fp8_mx', 'deepep_cast_back_fp8_mx', 'deepep_dispatch_pack_cast_mx',
           'deepep_dispatch_copy_cast_mx')
BF16_MAX = torch.finfo(torch.bfloat16).max


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29578')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(rank: int, tokens: int = T, hidden: int = H):
    """bf16 rows, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(500 + rank)
    x = (torch.randn((tokens, hidden), generator=g) * 3).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x, idx.to(topk_idx_t), w


def _buffer(group, kernels=MxOracleKernels):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = Spy(kernels())
    return buf


# ----------------------------------------------------------------------------- the oracle
def _direct(x: torch.Tensor):
    """The rule restated per 32 columns (include/deepep_amd.h, deepep_cast_fp8_mx)."""
    m, n = x.shape
    view = x.view(m, -1, 32)
    amax = view.abs().float().amax(dim=2).clamp(1e-4)
    bits = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    scale = ((127 - e) << 23).view(torch.float32)
    q = (view.float() * scale.unsqueeze(2)).to(torch.float8_e4m3fn).view(m, n).contiguous()
    return q, (e + 127).to(torch.uint8)


def test_the_oracle_pair_is_the_per_32_rule_and_differs_from_the_per_128_cast():
    g = torch.Generator().manual_seed(3)
    Tn, Hn = 37, 640
    x = torch.randn((Tn, Hn), generator=g) * torch.exp2(torch.randint(-20, 20, (Tn, Hn // 32, 1), generator=g).float()
                                                        ).expand(Tn, Hn // 32, 32).reshape(Tn, Hn)
    x[:, :32] = torch.randn((Tn, 32), generator=g) * 1e-6          # under the 1e-4 clamp
    x[:, 32:64] = x[:, 32:64].clamp(-1, 1)
    x[:, 32 + 5] = 448.0 * 2.0 ** -4                               # amax / 448 an exact power of two
    x[:, 64:96] = x[:, 64:96].clamp(-1, 1)
    x[:, 64 + 17] = -BF16_MAX
    x = x.to(torch.bfloat16)
    q, sf = mx_pair(x)
    q_d, sf_d = _direct(x)
    assert sf.dtype == torch.uint8 and tuple(sf.shape) == (Tn, Hn // 32) and sf.is_contiguous()
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (Tn, Hn)
    assert torch.equal(sf, sf_d) and torch.equal(q.view(torch.uint8), q_d.view(torch.uint8))
    assert int(sf.min()) == 105 and int(sf.max()) == 247 and bool((sf[:, 0] == 105).all()) and bool((sf[:, 2] == 247).all())
    assert bool((sf[:, 1] == 123).all())                           # 448 * 2^-4: no round up
    # a cast that ignores the group size gives other e4m3fn bytes on such input
    assert not torch.equal(q.view(torch.uint8), cast_ref(x, True)[0].view(torch.uint8))
    # the free view torch's MX operators take, and the cast back of the pair
    assert sf.view(torch.float8_e8m0fnu).dtype == torch.float8_e8m0fnu
    back = mx_back_ref(q, sf)
    assert back.dtype == torch.bfloat16 and tuple(back.shape) == (Tn, Hn)
    want = (q.float().view(Tn, -1, 32) * mx_factors(sf).unsqueeze(2)).view(Tn, Hn).to(torch.bfloat16)
    assert torch.equal(back.view(torch.int16), want.view(torch.int16))
    assert torch.equal(mx_back_ref(q, sf.view(torch.float8_e8m0fnu)).view(torch.int16), back.view(torch.int16))


# ----------------------------------------------------------------------------- one rank
def test_keyword_equals_tuple_dispatch_one_rank(group):
    buf = _buffer(group)
    fails = mx_cases(buf, _inputs(0), _inputs(0, 0), E)
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast' in names and 'dispatch_pack_cast' not in names and 'cast_fp8' not in names
    flagged = [c for c in buf.kernels.calls if c[0] == 'dispatch_copy_cast']
    assert flagged and all(dict(c[2]).get('mx') is True and dict(c[2]).get('round_scale') is True and
                           'ue8m0' not in dict(c[2]) for c in flagged)


def test_rejections_come_before_any_kernel_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    cast = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True)
    for what, xin, kw in (('fp8_group_size=64', x, dict(cast, fp8_group_size=64)),
                          ('fp8_group_size=0', x, dict(cast, fp8_group_size=0)),
                          ('32 without fp8_use_ue8m0', x, dict(cast_to_fp8=True, fp8_round_scale=True,
                                                               fp8_group_size=32)),
                          ('32 without fp8_round_scale', x, dict(cast_to_fp8=True, fp8_group_size=32)),
                          ('32 without cast_to_fp8', x, dict(fp8_group_size=32)),
                          ('H % 128 != 0', x[:, :96].contiguous(), MX),
                          ('a tuple x', mx_pair(x), MX)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.dispatch(xin, **kw, **base)
        assert buf.kernels.calls == [], what
    p = inspect.signature(type(buf).dispatch).parameters['fp8_group_size']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 128


def test_combine_rejects_mx_scale_factors_before_any_kernel_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    (q, sf), _, ex_w, handle, _ = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True, **MX)
    assert sf.dtype == torch.uint8 and tuple(sf.shape) == (q.shape[0], H // 32)
    before = len(buf.kernels.calls)
    for pair in ((q, sf), (q, sf.view(torch.float8_e8m0fnu))):
        with pytest.raises(RuntimeError, match='per_token_cast_back'):
            buf.combine(pair, handle, topk_weights=ex_w)
    assert len(buf.kernels.calls) == before


class _Loaded(Exception):
    pass


class _NoLib:
    def __getattr__(self, name):
        raise _Loaded(name)


def _hip_wrappers():
    """HipKernels without a library: a call that passes the wrapper's own checks raises _Loaded at the entry."""
    from deepep_amd.kernels import HipKernels
    k = HipKernels.__new__(HipKernels)
    k.lib = _NoLib()
    return k


def test_wrappers_reject_mx_with_ue8m0_and_without_round_scale():
    """The checks of the HIP wrappers themselves, before the library is touched (CPU tensors: the device check of
    cast_fp8 comes first, so its rejections are read from the message)."""
    from deepep_amd.kernels import RowLayout
    k = _hip_wrappers()
    x, idx, w = _inputs(0)
    idx = idx.to(torch.int64)
    xb = x.view(torch.uint8).view(T, 2 * H)
    slot = torch.zeros((T, 1), dtype=torch.int32)
    off = torch.zeros((1,), dtype=torch.int32)
    lay = RowLayout.make(H, H // 32, K)
    packed = torch.zeros((T, lay.row_bytes), dtype=torch.uint8)
    meta = torch.zeros((T, K + 2), dtype=torch.int32)
    rx, rsf = torch.zeros((T, H), dtype=torch.uint8), torch.zeros((T, H // 32), dtype=torch.uint8)

    class Cuda:                                                # a stand-in idx that passes the routing check
        is_cuda, dtype, shape = True, torch.int64, idx.shape

        def is_contiguous(self):
            return True

    for kw, text in ((dict(round_scale=True, mx=True, ue8m0=True), 'exclude each other'),
                     (dict(round_scale=False, mx=True), 'round_scale')):
        with pytest.raises(RuntimeError, match=text):
            k.dispatch_pack_cast(xb, Cuda(), w, 0, slot, off, packed, lay, **kw)
        with pytest.raises(RuntimeError, match=text):
            k.dispatch_copy_cast(packed, lay, T, meta, False, rx, rsf, None, x_direct=xb, num_max_tokens=T, **kw)
    # (the fp32 layout's H / 128 * 4 scale bytes are MXFP8's H / 32: the packed UE8M0 layout is the other one)
    with pytest.raises(RuntimeError, match='H / 32'):
        k.dispatch_pack_cast(xb, Cuda(), w, 0, slot, off, packed, RowLayout.make(H, H // 128, K), round_scale=True,
                             mx=True)
    with pytest.raises(RuntimeError, match='H / 32'):
        k.dispatch_copy_cast(packed, lay, T, meta, False, rx, rsf[:, :3].contiguous(), None, x_direct=xb,
                             num_max_tokens=T, round_scale=True, mx=True)
    with pytest.raises(_Loaded, match='deepep_dispatch_copy_cast_mx'):              # well-formed: on to the entry
        k.dispatch_copy_cast(packed, lay, T, meta, False, rx, rsf, None, x_direct=xb, num_max_tokens=T,
                             round_scale=True, mx=True)
    with pytest.raises(_Loaded, match='deepep_dispatch_pack_cast_mx'):
        k.dispatch_pack_cast(xb, Cuda(), w, 0, slot, off, packed, lay, round_scale=True, mx=True)


# ----------------------------------------------------------------------------- 4 thread ranks
def _rank_thread(rank, comm, bypass, results):
    try:
        buf = _buffer(FakeGroup(rank, comm.n, comm))
        buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
        buf.local_bypass = bypass
        fails = mx_cases(buf, _inputs(rank), _inputs(rank, 0 if rank == 1 else T), E)
        names = buf.kernels.names()
        if 'dispatch_pack_cast' not in names or 'dispatch_copy_cast' in names or 'cast_fp8' in names:
            fails.append(f'EP > 1 casts in the pack only, got {sorted(set(names))}')
        if not all(dict(c[2]).get('mx') is True for c in buf.kernels.calls if c[0] == 'dispatch_pack_cast'):
            fails.append('a casting pack without mx')
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
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-3] + '_ue8m0'], name       # the siblings' arguments
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
    good = dict(x=16, stride=768, rows=4, hidden=384, q=32, sf=52, stream=None)
    _rejects(lib, 'deepep_cast_fp8_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'cast_fp8_mx' in err()
    _rejects(lib, 'deepep_cast_fp8_mx', good, [dict(hidden=160, stride=320), dict(hidden=0), dict(rows=-1),
                                               dict(x=None), dict(q=None), dict(sf=None), dict(x=24), dict(q=40),
                                               dict(sf=54)])
    assert b'aligned' in err()
    _rejects(lib, 'deepep_cast_fp8_mx', good, [dict(stride=752), dict(stride=776)])
    assert b'stride' in err()
    assert lib.deepep_cast_fp8_mx(*dict(good, rows=0, x=None, q=None, sf=None).values()) == 0

    good = dict(q=16, q_stride=384, sf=36, sf_row=12, sf_col=1, rows=4, hidden=384, out=48, stream=None)
    _rejects(lib, 'deepep_cast_back_fp8_mx', good, [dict(hidden=96, q_stride=96)])
    assert b'multiple of 128' in err() and b'cast_back_fp8_mx' in err()
    _rejects(lib, 'deepep_cast_back_fp8_mx', good,
             [dict(hidden=0), dict(rows=-1), dict(q=None), dict(out=None), dict(sf=None), dict(q=24), dict(out=56),
              dict(sf=38), dict(q_stride=368), dict(q_stride=392), dict(sf_row=-1), dict(sf_col=-1),
              dict(sf_row=13), dict(sf_row=14)])                # contiguous columns: rows start on 4 bytes
    assert b'4-byte' in err()
    assert lib.deepep_cast_back_fp8_mx(*dict(good, rows=0, q=None, sf=None, out=None).values()) == 0

    lay = RowLayout.make(384, 384 // 32, K)
    good = dict(x=16, stride=768, hidden=384, idx=64, w=None, tokens=4, topk=K, src_base=0, dst_slot=128,
                send_offsets=256, ranks=1, packed=512, dest_bases=None, row_bytes=lay.row_bytes, dest_rows=4,
                sf_off=lay.sf_off, idx_off=lay.idx_off, w_off=lay.w_off, src_off=lay.src_off, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_pack_cast_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_pack_cast_mx' in err()
    _rejects(lib, 'deepep_dispatch_pack_cast_mx', good,
             [dict(x=None), dict(x=24), dict(stride=760), dict(packed=520), dict(sf_off=382), dict(sf_off=380),
              dict(idx_off=lay.sf_off), dict(idx_off=lay.sf_off + 8), dict(topk=0), dict(ranks=65),
              dict(row_bytes=lay.src_off)])                     # idx_off + 8: under the hidden / 32 = 12 exponent bytes
    assert lib.deepep_dispatch_pack_cast_mx(*dict(good, tokens=0).values()) == 0

    good = dict(packed=16, row_bytes=128, w_off=0, recv=4, topk=K, meta=64, expanded=0, x=128, stride=768, hidden=384,
                max_tokens=4, recv_x=256, recv_sf=516, recv_w=None, out_rows=4, inv=None, offsets=None, end=None,
                experts=0, row_map=None, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_copy_cast_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_copy_cast_mx' in err()
    _rejects(lib, 'deepep_dispatch_copy_cast_mx', good,
             [dict(x=None), dict(x=136), dict(stride=760), dict(recv_x=None), dict(recv_x=264), dict(recv_sf=None),
              dict(recv_sf=518), dict(meta=None), dict(max_tokens=0), dict(inv=1024)])
    assert lib.deepep_dispatch_copy_cast_mx(*dict(good, recv=0).values()) == 0


# ----------------------------------------------------------------------------- the public functions
@pytest.fixture
def no_library(monkeypatch):
    from deepep_amd import _lib

    def no_load(*a, **kw):
        raise _Loaded()

    monkeypatch.setattr(_lib, 'load', no_load)


def test_public_cast_checks_its_arguments_before_loading_the_library(no_library):
    import deepep_amd
    x = torch.zeros((4, 384), dtype=torch.bfloat16)
    full = dict(round_scale=True, use_ue8m0=True)
    for what, args, kw in (('group_size=64', (x,), dict(full, group_size=64)),
                           ('group_size=16', (x,), dict(full, group_size=16)),
                           ('32 without use_ue8m0', (x,), dict(round_scale=True, group_size=32)),
                           ('32 without round_scale', (x,), dict(group_size=32)),
                           ('H % 128 != 0', (x[:, :96],), dict(full, group_size=32)),
                           ('float rows', (x.float(),), dict(full, group_size=32))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_to_fp8(*args, **kw)
    with pytest.raises(TypeError):                             # keyword-only
        deepep_amd.per_token_cast_to_fp8(x, True, True, 32)
    with pytest.raises(_Loaded):                               # well-formed: on to the library
        deepep_amd.per_token_cast_to_fp8(x, group_size=32, **full)
    with pytest.raises(_Loaded):                               # 128 stays the default
        deepep_amd.per_token_cast_to_fp8(x, group_size=128)


def test_public_cast_back_takes_well_shaped_mx_scale_factors_only(no_library):
    import deepep_amd
    q = torch.zeros((4, 384), dtype=torch.float8_e4m3fn)
    for sf in (torch.zeros((4, 12), dtype=torch.uint8), torch.zeros((4, 12), dtype=torch.uint8).view(torch.float8_e8m0fnu),
               torch.zeros((12, 4), dtype=torch.uint8).t()):   # either dtype, any strides
        with pytest.raises(_Loaded):
            deepep_amd.per_token_cast_back(q, sf)
    for what, sf in (('the per-128 shape', torch.zeros((4, 3), dtype=torch.uint8)),
                     ('a wrong row count', torch.zeros((3, 12), dtype=torch.uint8)),
                     ('1-D', torch.zeros((48,), dtype=torch.uint8)),
                     ('e8m0 of the wrong shape', torch.zeros((4, 3), dtype=torch.uint8).view(torch.float8_e8m0fnu))):
        with pytest.raises(RuntimeError, match='Assertion failed') as info:
            deepep_amd.per_token_cast_back(q, sf)
        assert 'MXFP8' in str(info.value), what
    out = deepep_amd.per_token_cast_back(q[:0], torch.zeros((0, 12), dtype=torch.uint8))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 384)
