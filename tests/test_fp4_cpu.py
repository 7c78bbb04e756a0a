"""MXFP4 (cast_to_fp4) without a GPU: the reference pair (tests/fp4_ref.fp4_pair, the threshold table) against a
second, independent restatement of the rule (nearest magnitude by argmin, ties to the even code) and against the error
bound the format implies; the free views; ElasticBuffer.dispatch(..., cast_to_fp4=True) on the CPU stand-in, at one
rank and over 4 thread ranks, against the tuple dispatch of fp4_pair(x) -- bit for bit, every handle field and the
scale-factor strides included; the rejections before any kernel call; the four C-ABI entries exported, prototyped,
declared, documented and rejecting bad arguments before a launch; the argument checks of the two public functions; and
no FP4 wrapper named on any other path."""
import inspect
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp4_ref import (E2M1_VALUES, FP4, FP4_WRAPPERS, Fp4OracleKernels, fp4_back_ref, fp4_cases, fp4_codes,
                           fp4_pack, fp4_pair)
from tests.fp8_oracle_kernels import Spy
from tests.mx_ref import MX, mx_factors
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 384, 3, 8              # 384: three dwords of exponent bytes a row
ENTRIES = ('deepep_cast_fp4_mx', 'deepep_cast_back_fp4_mx', 'deepep_dispatch_pack_cast_fp4_mx',
           'deepep_dispatch_copy_cast_fp4_mx')
BF16_MAX = torch.finfo(torch.bfloat16).max
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29579')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(rank: int, tokens: int = T, hidden: int = H):
    """bf16 rows whose 32-column groups differ by binades, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(700 + rank)
    scale = torch.exp2(torch.randint(-6, 6, (tokens, hidden // 32, 1), generator=g).float()).expand(
        tokens, hidden // 32, 32).reshape(tokens, hidden)
    x = (torch.randn((tokens, hidden), generator=g) * 3 * scale).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x, idx.to(topk_idx_t), w


def _buffer(group, kernels=Fp4OracleKernels):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = Spy(kernels())
    return buf


# ----------------------------------------------------------------------------- the reference
def _direct(x: torch.Tensor):
    """The rule restated without the threshold table: the code is the argmin of |m - magnitude| in float64 (exact for
    fp32 m), a tie going to the even code."""
    m_, n = x.shape
    v = x.float().view(m_, -1, 32)
    amax = v.abs().amax(dim=2).clamp(1e-4)
    bits = (amax * torch.tensor(1.0 / 6.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    m = (v.abs() * torch.exp2(-e.float()).unsqueeze(2)).double()
    dist_ = (m.unsqueeze(3) - torch.tensor(E2M1_VALUES, dtype=torch.float64)).abs()
    # ties: prefer the even code -- order the candidates even codes first, argmin takes the first minimum
    order = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    code = order[dist_[..., order].argmin(dim=3)].to(torch.uint8)
    sign = torch.signbit(v).to(torch.uint8) << 3
    return (code | sign).view(m_, n), (e + 127).to(torch.uint8)


def _oracle_input():
    g = torch.Generator().manual_seed(4)
    Tn, Hn = 37, 640
    x = torch.randn((Tn, Hn), generator=g) * torch.exp2(torch.randint(-20, 20, (Tn, Hn // 32, 1), generator=g).float()
                                                        ).expand(Tn, Hn // 32, 32).reshape(Tn, Hn)
    x[:, :32] = torch.randn((Tn, 32), generator=g) * 1e-6          # under the 1e-4 clamp
    x[:, 32:64] = x[:, 32:64].clamp(-1, 1) * 2.0 ** -4
    x[:, 32 + 5] = 6.0 * 2.0 ** -4                                 # amax / 6 an exact power of two
    x[:, 64:96] = x[:, 64:96].clamp(-1, 1)
    x[:, 64 + 17] = -BF16_MAX
    # every tie point times the group's scale 2^3 (amax 6 * 2^3), both signs; -0.0 and a negative value that rounds
    # to zero
    x[:, 96:128] = 0.0
    x[:, 96] = 48.0
    for j, t in enumerate(TIES):
        x[:, 97 + 2 * j] = t * 8
        x[:, 98 + 2 * j] = -t * 8
    x[:, 120] = -0.0
    x[:, 121] = -0.1 * 8
    return x.to(torch.bfloat16)


def test_the_reference_pair_equals_an_independent_restatement():
    x = _oracle_input()
    Tn, Hn = x.shape
    codes, sf = fp4_codes(x)
    codes_d, sf_d = _direct(x)
    assert sf.dtype == torch.uint8 and tuple(sf.shape) == (Tn, Hn // 32) and sf.is_contiguous()
    assert torch.equal(sf, sf_d) and torch.equal(codes, codes_d)
    assert bool((sf[:, 0] == 112).all()) and int(sf.min()) == 112          # the 1e-4 clamp
    assert bool((sf[:, 1] == 123).all())                                   # 6 * 2^-4: no round up
    assert bool((sf[:, 2] == 253).all()) and int(sf.max()) == 253          # the largest finite bf16
    assert bool((sf[:, 3] == 130).all())
    # the tie points: to the even code, both signs
    want = (0, 2, 2, 4, 4, 6, 6)
    for j, c in enumerate(want):
        assert bool((codes[:, 97 + 2 * j] == c).all()) and bool((codes[:, 98 + 2 * j] == (c | 8)).all()), TIES[j]
    assert bool((codes[:, 96] == 7).all())
    assert bool((codes[:, 120] == 8).all()) and bool((codes[:, 121] == 8).all())    # the sign of x is kept
    # the packed rows: column 2j in bits 3:0 of byte j
    q, sf_p = fp4_pair(x)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (Tn, Hn // 2) and torch.equal(sf_p, sf)
    assert torch.equal(q & 0xf, codes[:, 0::2]) and torch.equal(q >> 4, codes[:, 1::2])
    assert torch.equal(fp4_pack(codes), q)


def test_the_cast_back_of_the_pair_is_within_half_the_widest_spacing():
    """|back(pair(x)) - x| <= 2^e of the group: half the widest code spacing (4 .. 6) is 1, scaled by the factor.
    (Over finite results: a group whose amax is above 2^127 has e = 126, and its codes 6 and 7 decode to 2^128 and
    above, past the largest fp32 -- so the largest group here has its amax two binades below the largest bf16.)"""
    first = _oracle_input()
    first[:, 64 + 17] = -BF16_MAX / 4
    x = torch.cat([first, _inputs(1, 37, 640)[0]])
    q, sf = fp4_pair(x)
    back = fp4_back_ref(q, sf)
    assert back.dtype == torch.bfloat16 and back.shape == x.shape
    bound = mx_factors(sf).double().unsqueeze(2).expand(-1, -1, 32).reshape(x.shape)
    err = (back.double() - x.double()).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err > 0).any())


def test_views_are_free_and_typed_pairs_cast_back_alike():
    x = _oracle_input()
    q, sf = fp4_pair(x)
    q4, sf8 = q.view(torch.float4_e2m1fn_x2), sf.view(torch.float8_e8m0fnu)
    assert q4.dtype == torch.float4_e2m1fn_x2 and q4.data_ptr() == q.data_ptr() and tuple(q4.shape) == tuple(q.shape)
    assert sf8.dtype == torch.float8_e8m0fnu and sf8.data_ptr() == sf.data_ptr()
    back = fp4_back_ref(q, sf)
    assert torch.equal(fp4_back_ref(q4, sf8).view(torch.int16), back.view(torch.int16))
    assert torch.equal(fp4_back_ref(q, sf.t().contiguous().t()).view(torch.int16), back.view(torch.int16))


# ----------------------------------------------------------------------------- one rank
def test_keyword_equals_tuple_dispatch_one_rank(group):
    buf = _buffer(group)
    fails = fp4_cases(buf, _inputs(0), _inputs(0, 0), E)
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast_fp4' in names and 'dispatch_pack_cast_fp4' not in names and 'cast_fp4' not in names
    assert 'dispatch_copy_cast' not in names and 'dispatch_pack_cast' not in names


def test_rejections_come_before_any_kernel_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for what, xin, kw in (('with cast_to_fp8', x, dict(FP4, cast_to_fp8=True)),
                          ('with fp8_round_scale', x, dict(FP4, fp8_round_scale=True)),
                          ('with fp8_use_ue8m0', x, dict(FP4, fp8_use_ue8m0=True)),
                          ('with fp8_group_size=32', x, dict(FP4, fp8_group_size=32)),
                          ('with the MX flags', x, dict(FP4, **MX)),
                          ('a tuple x', fp4_pair(x), FP4),
                          ('H % 128 != 0', x[:, :96].contiguous(), FP4),
                          ('H % 128 != 0 (64)', x[:, :64].contiguous(), FP4),
                          ('float x', x.float(), FP4),
                          ('uint8 x', fp4_pair(x)[0], FP4)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.dispatch(xin, **kw, **base)
        assert buf.kernels.calls == [], what
    p = inspect.signature(type(buf).dispatch).parameters
    assert p['cast_to_fp4'].kind is inspect.Parameter.KEYWORD_ONLY and p['cast_to_fp4'].default is False
    assert list(p)[-1] == 'fp8_use_ue8m0'


class _Loaded(Exception):
    pass


class _NoLib:
    def __getattr__(self, name):
        raise _Loaded(name)


def test_no_fp4_wrapper_is_named_on_other_paths(group):
    """HipKernels without a library: a call dies at the first entry it looks up.  A provider that lacks the FP4
    wrappers (the MX stand-in) serves FP8, MXFP8 and bf16 dispatches, and the spy never sees an *_fp4 name."""
    from deepep_amd.kernels import Fp4Kernels, HipKernels
    from tests.mx_ref import MxOracleKernels
    assert set(FP4_WRAPPERS) == {n for n, v in vars(Fp4Kernels).items() if callable(v) and not n.startswith('_')}
    assert not set(FP4_WRAPPERS) & set(vars(HipKernels)) and issubclass(HipKernels, Fp4Kernels)
    assert not any(hasattr(MxOracleKernels, n) for n in FP4_WRAPPERS)
    buf = _buffer(group, MxOracleKernels)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for kw in (dict(), dict(do_expand=True), dict(cast_to_fp8=True), dict(MX), dict(MX, do_expand=True)):
        buf.dispatch(x, **kw, **base)
    assert buf.kernels.calls and not any(n.endswith('_fp4') for n in buf.kernels.names())
    hip = HipKernels.__new__(HipKernels)
    hip.lib = _NoLib()
    buf._kernels = Spy(hip)
    for kw in (dict(), dict(cast_to_fp8=True), dict(MX)):
        # (CPU tensors: the first wrapper's own device check, or the first entry looked up, ends the call)
        with pytest.raises((RuntimeError, _Loaded)) as info:
            buf.dispatch(x, **kw, **base)
        assert 'fp4' not in str(info.value)
    assert buf.kernels.calls and not any(n.endswith('_fp4') for n in buf.kernels.names())


# ----------------------------------------------------------------------------- 4 thread ranks
def _rank_thread(rank, comm, bypass, results):
    try:
        buf = _buffer(FakeGroup(rank, comm.n, comm))
        buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
        buf.local_bypass = bypass
        fails = fp4_cases(buf, _inputs(rank), _inputs(rank, 0 if rank == 1 else T), E)
        names = buf.kernels.names()
        if 'dispatch_pack_cast_fp4' not in names or 'dispatch_copy_cast_fp4' in names or 'cast_fp4' in names:
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


# ----------------------------------------------------------------------------- the C-ABI, without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_entries_are_exported_prototyped_declared_and_documented(lib):
    import deepep_amd
    from deepep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f'int {name}(' in header and f'`{name}`' in integration, name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('_fp4_mx', '_fp8_mx' if 'dispatch' not in name
                                                                     else '_mx')], name     # the siblings' arguments
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    assert {'per_token_cast_to_fp4', 'per_token_cast_back_fp4'} <= set(deepep_amd.__all__)


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
    _rejects(lib, 'deepep_cast_fp4_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'cast_fp4_mx' in err()
    _rejects(lib, 'deepep_cast_fp4_mx', good, [dict(hidden=64, stride=128), dict(hidden=160, stride=320),
                                               dict(hidden=0), dict(rows=-1), dict(x=None), dict(q=None),
                                               dict(sf=None), dict(x=24), dict(q=40), dict(sf=54)])
    assert b'aligned' in err()
    _rejects(lib, 'deepep_cast_fp4_mx', good, [dict(stride=752), dict(stride=776)])
    assert b'stride' in err()
    assert lib.deepep_cast_fp4_mx(*dict(good, rows=0, x=None, q=None, sf=None).values()) == 0

    good = dict(q=16, q_stride=192, sf=36, sf_row=12, sf_col=1, rows=4, hidden=384, out=48, stream=None)
    _rejects(lib, 'deepep_cast_back_fp4_mx', good, [dict(hidden=96, q_stride=48)])
    assert b'multiple of 128' in err() and b'cast_back_fp4_mx' in err()
    _rejects(lib, 'deepep_cast_back_fp4_mx', good,
             [dict(hidden=0), dict(hidden=64), dict(rows=-1), dict(q=None), dict(out=None), dict(sf=None), dict(q=24),
              dict(out=56), dict(sf=38), dict(q_stride=176), dict(q_stride=200), dict(sf_row=-1), dict(sf_col=-1),
              dict(sf_row=13), dict(sf_row=14)])                # contiguous columns: rows start on 4 bytes
    assert b'4-byte' in err()
    _rejects(lib, 'deepep_cast_back_fp4_mx', good, [dict(q_stride=176)])           # below hidden / 2 = 192
    assert b'hidden / 2' in err()
    assert lib.deepep_cast_back_fp4_mx(*dict(good, rows=0, q=None, sf=None, out=None).values()) == 0

    lay = RowLayout.make(384 // 2, 384 // 32, K)
    assert lay.sf_off == 192
    good = dict(x=16, stride=768, hidden=384, idx=64, w=None, tokens=4, topk=K, src_base=0, dst_slot=128,
                send_offsets=256, ranks=1, packed=512, dest_bases=None, row_bytes=lay.row_bytes, dest_rows=4,
                sf_off=lay.sf_off, idx_off=lay.idx_off, w_off=lay.w_off, src_off=lay.src_off, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_pack_cast_fp4_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_pack_cast_fp4_mx' in err()
    _rejects(lib, 'deepep_dispatch_pack_cast_fp4_mx', good,
             [dict(hidden=64, stride=128), dict(x=None), dict(x=24), dict(stride=760), dict(packed=520),
              dict(sf_off=190), dict(sf_off=188), dict(idx_off=lay.sf_off), dict(idx_off=lay.sf_off + 8),
              dict(topk=0), dict(ranks=65), dict(row_bytes=lay.src_off)])   # + 8: under the 12 exponent bytes
    assert b'row layout' in err()
    assert lib.deepep_dispatch_pack_cast_fp4_mx(*dict(good, tokens=0).values()) == 0

    good = dict(packed=16, row_bytes=128, w_off=0, recv=4, topk=K, meta=64, expanded=0, x=128, stride=768, hidden=384,
                max_tokens=4, recv_x=256, recv_sf=516, recv_w=None, out_rows=4, inv=None, offsets=None, end=None,
                experts=0, row_map=None, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_copy_cast_fp4_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_copy_cast_fp4_mx' in err()
    _rejects(lib, 'deepep_dispatch_copy_cast_fp4_mx', good,
             [dict(hidden=0), dict(hidden=64, stride=128), dict(x=None), dict(x=136), dict(stride=760),
              dict(recv_x=None), dict(recv_x=264), dict(recv_sf=None), dict(recv_sf=518), dict(meta=None),
              dict(max_tokens=0), dict(inv=1024)])
    assert lib.deepep_dispatch_copy_cast_fp4_mx(*dict(good, recv=0).values()) == 0


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
    for what, arg in (('H % 128 != 0', x[:, :96]), ('H = 64', x[:, :64]), ('float rows', x.float()),
                      ('1-D', x[0]), ('no columns', x[:, :0]), ('a pair', (x, x))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_to_fp4(arg)
    with pytest.raises(_Loaded):                               # well-formed: on to the library
        deepep_amd.per_token_cast_to_fp4(x)
    q, sf = deepep_amd.per_token_cast_to_fp4(x[:0])            # no rows: no launch
    assert (q.dtype, tuple(q.shape), sf.dtype, tuple(sf.shape)) == (torch.uint8, (0, 192), torch.uint8, (0, 12))


def test_public_cast_back_takes_both_dtypes_of_rows_and_scales(no_library):
    import deepep_amd
    q = torch.zeros((4, 192), dtype=torch.uint8)
    sf = torch.zeros((4, 12), dtype=torch.uint8)
    for rows in (q, q.view(torch.float4_e2m1fn_x2), torch.zeros((4, 256), dtype=torch.uint8)[:, :192]):
        for scales in (sf, sf.view(torch.float8_e8m0fnu), torch.zeros((12, 4), dtype=torch.uint8).t()):
            with pytest.raises(_Loaded):
                deepep_amd.per_token_cast_back_fp4(rows, scales)
    for what, rows, scales in (('e4m3fn rows', q.view(torch.float8_e4m3fn), sf),
                               ('bf16 rows', torch.zeros((4, 192), dtype=torch.bfloat16), sf),
                               ('H % 128 != 0', q[:, :48], sf[:, :3]),
                               ('the per-128 shape', q, sf[:, :3]),
                               ('a wrong row count', q, sf[:3]),
                               ('1-D scales', q, sf.reshape(-1)),
                               ('fp32 scales', q, sf.float()),
                               ('int32 scales', q, torch.zeros((4, 3), dtype=torch.int32)),
                               ('no scales', q, None)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_back_fp4(rows, scales)
    out = deepep_amd.per_token_cast_back_fp4(q[:0], sf[:0])
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 384)
