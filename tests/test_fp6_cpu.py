"""MXFP6 (cast_to_fp6) without a GPU: the reference pair (tests/fp6_ref.fp6_pair, the threshold table) against a
second, independent restatement of the rule (nearest magnitude by argmin, ties to the even code), the range facts of
the ceiling rule over every positive finite bf16, the error bound the format implies and the accuracy against MXFP4;
ElasticBuffer.dispatch(..., cast_to_fp6=True) on the CPU stand-in, at one rank and over 4 thread ranks, against the
tuple dispatch of fp6_pair(x) -- bit for bit, every handle field and the scale-factor strides included; the rejections
before any kernel call; the C-ABI entries exported, prototyped, declared, documented and rejecting bad arguments before
a launch; the argument checks of the two public functions; and no FP6 wrapper named on any other path."""
import inspect
import os
import threading
import traceback

import pytest
import torch
import torch.distributed as dist

from tests.fp6_ref import (E2M3_TIES, E2M3_VALUES, FP6, FP6_WRAPPERS, Fp6OracleKernels, fp6_back_ref, fp6_cases,
                           fp6_codes, fp6_pack, fp6_pair, fp6_unpack)
from tests.fp8_oracle_kernels import Spy
from tests.mx_ref import MX, mx_factors
from tests.sim import FakeGroup
from tests.test_cast_keyword_cpu import CpuComm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, K, E = 33, 384, 3, 8              # 384: three dwords of exponent bytes a row
ENTRIES = ('deepep_cast_fp6_mx', 'deepep_cast_back_fp6_mx', 'deepep_dispatch_pack_cast_fp6_mx',
           'deepep_dispatch_copy_cast_fp6_mx')
BF16_MAX = torch.finfo(torch.bfloat16).max


@pytest.fixture(scope='module')
def group():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29581')
        dist.init_process_group('gloo', rank=0, world_size=1)
    return dist.group.WORLD


def _inputs(rank: int, tokens: int = T, hidden: int = H):
    """bf16 rows whose 32-column groups differ by binades, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(900 + rank)
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


def _buffer(group, kernels=Fp6OracleKernels):
    from deepep_amd import ElasticBuffer
    buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K)
    buf._kernels = Spy(kernels())
    return buf


# ----------------------------------------------------------------------------- the reference
def _table():
    """The 32 magnitudes from the bit fields, not from tests/fp6_ref."""
    out = []
    for c in range(32):
        ee, mmm = c >> 3, c & 7
        out.append(mmm / 8 if ee == 0 else (1 + mmm / 8) * 2 ** (ee - 1))
    return out


def _direct(x: torch.Tensor):
    """The rule restated without the threshold table: the code is the argmin of |m - magnitude| in float64 (exact for
    fp32 m), a tie going to the even code."""
    m_, n = x.shape
    v = x.float().view(m_, -1, 32)
    amax = v.abs().amax(dim=2).clamp(1e-4)
    bits = (amax * torch.tensor(1.0 / 7.5, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    m = (v.abs() * torch.exp2(-e.float()).unsqueeze(2)).double()
    dist_ = (m.unsqueeze(3) - torch.tensor(_table(), dtype=torch.float64)).abs()
    # ties: prefer the even code -- order the candidates even codes first, argmin takes the first minimum
    order = torch.tensor(list(range(0, 32, 2)) + list(range(1, 32, 2)))
    code = order[dist_[..., order].argmin(dim=3)].to(torch.uint8)
    sign = torch.signbit(v).to(torch.uint8) << 5
    return (code | sign).view(m_, n), (e + 127).to(torch.uint8)


def _oracle_input():
    g = torch.Generator().manual_seed(6)
    Tn, Hn = 37, 640
    x = torch.randn((Tn, Hn), generator=g) * torch.exp2(torch.randint(-20, 20, (Tn, Hn // 32, 1), generator=g).float()
                                                        ).expand(Tn, Hn // 32, 32).reshape(Tn, Hn)
    x[:, :32] = torch.randn((Tn, 32), generator=g) * 1e-6          # under the 1e-4 clamp
    x[:, 32:64] = x[:, 32:64].clamp(-1, 1) * 2.0 ** -4
    x[:, 32 + 5] = 7.5 * 2.0 ** -4                                 # amax / 7.5 an exact power of two
    x[:, 64:96] = x[:, 64:96].clamp(-1, 1)
    x[:, 64 + 17] = -BF16_MAX
    # every tie point times the group's scale 2^3 (amax 7.5 * 2^3): group 3 the positive ones, group 4 the negative
    # ones; group 5: -0.0 and a negative value that rounds to zero
    x[:, 96:192] = 0.0
    x[:, 96] = x[:, 128] = x[:, 160] = 60.0
    for j, t in enumerate(E2M3_TIES):
        x[:, 97 + j] = t * 8
        x[:, 129 + j] = -t * 8
    x[:, 161] = -0.0
    x[:, 162] = -0.05 * 8
    return x.to(torch.bfloat16)


def test_the_table_and_the_tie_points():
    assert list(E2M3_VALUES) == _table() and E2M3_VALUES[31] == 7.5 and len(E2M3_TIES) == 31
    assert E2M3_TIES[0] == 0.0625 and E2M3_TIES[1] == 0.1875 and E2M3_TIES[30] == 7.25
    # every tie point times 8 is a bf16 (so _oracle_input holds the ties themselves)
    t = torch.tensor(E2M3_TIES) * 8
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    # fp32(1 / 7.5): the quotient of the two fp32 values, as the kernels' constant
    import numpy as np
    assert np.float32(1.0) / np.float32(7.5) == np.float32(1.0 / 7.5) == torch.tensor(1.0 / 7.5).item()


def test_the_reference_pair_equals_an_independent_restatement():
    x = _oracle_input()
    Tn, Hn = x.shape
    codes, sf = fp6_codes(x)
    codes_d, sf_d = _direct(x)
    assert sf.dtype == torch.uint8 and tuple(sf.shape) == (Tn, Hn // 32) and sf.is_contiguous()
    assert torch.equal(sf, sf_d) and torch.equal(codes, codes_d)
    assert bool((sf[:, 0] == 111).all()) and int(sf.min()) == 111          # the 1e-4 clamp
    assert bool((sf[:, 1] == 123).all())                                   # 7.5 * 2^-4: no round up
    assert bool((sf[:, 2] == 253).all()) and int(sf.max()) == 253          # the largest finite bf16
    assert bool((sf[:, 3:6] == 130).all())
    # the tie points: to the even code, both signs
    for j in range(31):
        c = j + 1 if j & 1 else j
        assert bool((codes[:, 97 + j] == c).all()) and bool((codes[:, 129 + j] == (c | 32)).all()), E2M3_TIES[j]
    assert bool((codes[:, 96] == 31).all())
    assert bool((codes[:, 161] == 32).all()) and bool((codes[:, 162] == 32).all())    # the sign of x is kept
    # the packed rows: column c of a group in bits 6c + 5 : 6c of its 24 bytes, little-endian
    q, sf_p = fp6_pair(x)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (Tn, 3 * Hn // 4) and torch.equal(sf_p, sf)
    assert torch.equal(fp6_pack(codes), q) and torch.equal(fp6_unpack(q), codes.long())
    grp = q[:, 72:96].long()                                               # group 3 as one 192-bit integer
    for r in (0, Tn - 1):
        n = sum(int(b) << (8 * i) for i, b in enumerate(grp[r]))
        assert [(n >> (6 * c)) & 63 for c in range(32)] == codes[r, 96:128].tolist()
    assert torch.equal(q[:, 72] & 63, codes[:, 96]) and torch.equal(q[:, 74] >> 2, codes[:, 99])


def test_the_ceiling_rule_keeps_every_bf16_amax_in_range():
    """Over every positive finite bf16 as a group's amax: the byte stays in 111..253, the scaled amax in (3.75, 7.5],
    so no element saturates -- re-derived here, then read off the reference pair."""
    bits = torch.arange(1, 0x7f80, dtype=torch.int32).to(torch.int16)
    vals = bits.view(torch.bfloat16)
    n = vals.numel()
    amax = vals.float().clamp(min=1e-4)
    b = (amax * torch.tensor(1.0 / 7.5, dtype=torch.float32)).view(torch.int32)
    e = ((b >> 23) & 0xff) - 127 + ((b & 0x7fffff) != 0).to(torch.int32)
    scaled = amax.double() * torch.exp2(-e.double())
    assert float(scaled.min()) > 3.75 and float(scaled.max()) <= 7.5
    assert int(e.min()) + 127 == 111 and int(e.max()) + 127 == 253
    x = torch.zeros((-(-n // 4), 128), dtype=torch.bfloat16)
    x.view(-1, 32)[:n, 7] = vals
    codes, sf = fp6_codes(x)
    assert torch.equal(sf.view(-1)[:n].int(), e + 127) and int(sf.min()) == 111 and int(sf.max()) == 253
    pin = codes.view(-1, 32)[:n, 7][vals.float() >= 1e-4]      # (below the clamp the clamp is the amax)
    assert int(pin.min()) >= 23 and int(pin.max()) == 31       # 3.75 is code 23; above it, never past 7.5


def test_the_cast_back_of_the_pair_is_within_half_the_widest_spacing():
    """|back(pair(x)) - x| <= 0.25 * 2^e of the group: half the widest code spacing (4 .. 7.5 in steps of 0.5), scaled
    by the factor.  (Over finite results: a group whose amax is above 2^127 has e = 126, and its largest codes decode
    past the largest fp32 -- so the largest group here has its amax two binades below the largest bf16.)"""
    first = _oracle_input()
    first[:, 64 + 17] = -BF16_MAX / 4
    x = torch.cat([first, _inputs(1, 37, 640)[0]])
    q, sf = fp6_pair(x)
    back = fp6_back_ref(q, sf)
    assert back.dtype == torch.bfloat16 and back.shape == x.shape
    bound = 0.25 * mx_factors(sf).double().unsqueeze(2).expand(-1, -1, 32).reshape(x.shape)
    err = (back.double() - x.double()).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err > 0).any())


def test_mxfp6_is_closer_than_mxfp4():
    from tests.fp4_ref import fp4_back_ref, fp4_pair
    from tests.logfmt_ref import calc_diff
    torch.manual_seed(0)
    x = torch.randn(64, 1024).to(torch.bfloat16)
    d6 = calc_diff(fp6_back_ref(*fp6_pair(x)).float(), x.float())
    d4 = calc_diff(fp4_back_ref(*fp4_pair(x)).float(), x.float())
    print(f'calc_diff: MXFP6 {d6:.3e}, MXFP4 {d4:.3e}')
    assert 0 < d6 < d4


def test_typed_and_strided_scales_cast_back_alike():
    x = _oracle_input()
    q, sf = fp6_pair(x)
    sf8 = sf.view(torch.float8_e8m0fnu)
    assert sf8.dtype == torch.float8_e8m0fnu and sf8.data_ptr() == sf.data_ptr()
    back = fp6_back_ref(q, sf)
    assert torch.equal(fp6_back_ref(q, sf8).view(torch.int16), back.view(torch.int16))
    assert torch.equal(fp6_back_ref(q, sf.t().contiguous().t()).view(torch.int16), back.view(torch.int16))


# ----------------------------------------------------------------------------- one rank
def test_keyword_equals_tuple_dispatch_one_rank(group):
    buf = _buffer(group)
    fails = fp6_cases(buf, _inputs(0), _inputs(0, 0), E)
    assert not fails, fails
    names = buf.kernels.names()
    assert 'dispatch_copy_cast_fp6' in names and 'dispatch_pack_cast_fp6' not in names and 'cast_fp6' not in names
    assert 'dispatch_copy_cast' not in names and 'dispatch_pack_cast' not in names
    assert not any(n.endswith('_fp4') for n in names)


def test_rejections_come_before_any_kernel_call(group):
    buf = _buffer(group)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for what, xin, kw in (('with cast_to_fp8', x, dict(FP6, cast_to_fp8=True)),
                          ('with cast_to_fp4', x, dict(FP6, cast_to_fp4=True)),
                          ('with fp8_round_scale', x, dict(FP6, fp8_round_scale=True)),
                          ('with fp8_use_ue8m0', x, dict(FP6, fp8_use_ue8m0=True)),
                          ('with fp8_group_size=32', x, dict(FP6, fp8_group_size=32)),
                          ('with the MX flags', x, dict(FP6, **MX)),
                          ('a tuple x', fp6_pair(x), FP6),
                          ('H % 128 != 0', x[:, :96].contiguous(), FP6),
                          ('H % 128 != 0 (64)', x[:, :64].contiguous(), FP6),
                          ('float x', x.float(), FP6),
                          ('uint8 x', fp6_pair(x)[0], FP6)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            buf.dispatch(xin, **kw, **base)
        assert buf.kernels.calls == [], what
    p = inspect.signature(type(buf).dispatch).parameters
    assert p['cast_to_fp6'].kind is inspect.Parameter.KEYWORD_ONLY and p['cast_to_fp6'].default is False
    assert list(p)[-1] == 'fp8_use_ue8m0'


class _Loaded(Exception):
    pass


class _NoLib:
    def __getattr__(self, name):
        raise _Loaded(name)


def test_no_fp6_wrapper_is_named_on_other_paths(group):
    """HipKernels without a library: a call dies at the first entry it looks up.  A provider that lacks the FP6
    wrappers (the FP4 stand-in) serves bf16, FP8, MXFP8 and MXFP4 dispatches, and the spy never sees an *_fp6 name."""
    from deepep_amd.kernels import Fp4Kernels, Fp6Kernels, HipKernels
    from tests.fp4_ref import FP4, Fp4OracleKernels
    assert set(FP6_WRAPPERS) == {n for n, v in vars(Fp6Kernels).items() if callable(v) and not n.startswith('_')}
    assert not set(FP6_WRAPPERS) & (set(vars(HipKernels)) | set(vars(Fp4Kernels))) and issubclass(HipKernels, Fp6Kernels)
    assert not any(hasattr(Fp4OracleKernels, n) for n in FP6_WRAPPERS)
    buf = _buffer(group, Fp4OracleKernels)
    x, idx, w = _inputs(0)
    base = dict(topk_idx=idx, topk_weights=w, num_experts=E)
    for kw in (dict(), dict(do_expand=True), dict(cast_to_fp8=True), dict(MX), dict(FP4), dict(FP4, do_expand=True)):
        buf.dispatch(x, **kw, **base)
    assert buf.kernels.calls and not any(n.endswith('_fp6') for n in buf.kernels.names())
    hip = HipKernels.__new__(HipKernels)
    hip.lib = _NoLib()
    buf._kernels = Spy(hip)
    for kw in (dict(), dict(cast_to_fp8=True), dict(MX), dict(FP4)):
        # (CPU tensors: the first wrapper's own device check, or the first entry looked up, ends the call)
        with pytest.raises((RuntimeError, _Loaded)) as info:
            buf.dispatch(x, **kw, **base)
        assert 'fp6' not in str(info.value)
    assert buf.kernels.calls and not any(n.endswith('_fp6') for n in buf.kernels.names())


# ----------------------------------------------------------------------------- 4 thread ranks
def _rank_thread(rank, comm, bypass, results):
    try:
        buf = _buffer(FakeGroup(rank, comm.n, comm))
        buf._a2a = lambda out, inp, os_=None, is_=None: comm.a2a(rank, out, inp, os_, is_)
        buf.local_bypass = bypass
        fails = fp6_cases(buf, _inputs(rank), _inputs(rank, 0 if rank == 1 else T), E)
        names = buf.kernels.names()
        if 'dispatch_pack_cast_fp6' not in names or 'dispatch_copy_cast_fp6' in names or 'cast_fp6' in names:
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
    for name in ENTRIES + ('deepep_cast_fp6_mx_stores',):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert f'int {name}(' in header and f'`{name}`' in integration, name
    for name in ENTRIES:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('_fp6_mx', '_fp4_mx')], name   # the siblings'
    assert '6c + 5 : 6c' in header and 'v_cvt_scalef32_pk32_fp6_bf16' in header    # the order, and whose it is
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    assert {'per_token_cast_to_fp6', 'per_token_cast_back_fp6'} <= set(deepep_amd.__all__)
    assert any('fp6_cast.hip' in s for s in _lib.SOURCES)                  # in the source hash: no stale binary


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
    _rejects(lib, 'deepep_cast_fp6_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'cast_fp6_mx' in err()
    _rejects(lib, 'deepep_cast_fp6_mx', good, [dict(hidden=64, stride=128), dict(hidden=160, stride=320),
                                               dict(hidden=0), dict(rows=-1), dict(x=None), dict(q=None),
                                               dict(sf=None), dict(x=24), dict(q=40), dict(sf=54)])
    assert b'aligned' in err()
    _rejects(lib, 'deepep_cast_fp6_mx', good, [dict(stride=752), dict(stride=776)])
    assert b'stride' in err()
    assert lib.deepep_cast_fp6_mx(*dict(good, rows=0, x=None, q=None, sf=None).values()) == 0
    good = dict(x=16, stride=768, rows=4, hidden=384, q=32, sf=52, store_bytes=16, stream=None)
    _rejects(lib, 'deepep_cast_fp6_mx_stores', good, [dict(store_bytes=4), dict(store_bytes=0), dict(store_bytes=24)])
    assert b'store_bytes' in err()
    _rejects(lib, 'deepep_cast_fp6_mx_stores', good, [dict(hidden=96, stride=192), dict(q=40), dict(store_bytes=8, x=24)])
    assert lib.deepep_cast_fp6_mx_stores(*dict(good, rows=0).values()) == 0

    good = dict(q=16, q_stride=288, sf=36, sf_row=12, sf_col=1, rows=4, hidden=384, out=48, stream=None)
    _rejects(lib, 'deepep_cast_back_fp6_mx', good, [dict(hidden=96, q_stride=80)])
    assert b'multiple of 128' in err() and b'cast_back_fp6_mx' in err()
    _rejects(lib, 'deepep_cast_back_fp6_mx', good,
             [dict(hidden=0), dict(hidden=64), dict(rows=-1), dict(q=None), dict(out=None), dict(sf=None), dict(q=24),
              dict(out=56), dict(sf=38), dict(q_stride=272), dict(q_stride=296), dict(sf_row=-1), dict(sf_col=-1),
              dict(sf_row=13), dict(sf_row=14)])                # contiguous columns: rows start on 4 bytes
    assert b'4-byte' in err()
    _rejects(lib, 'deepep_cast_back_fp6_mx', good, [dict(q_stride=272)])           # below 3 * hidden / 4 = 288
    assert b'3 * hidden / 4' in err()
    assert lib.deepep_cast_back_fp6_mx(*dict(good, rows=0, q=None, sf=None, out=None).values()) == 0

    lay = RowLayout.make(3 * 384 // 4, 384 // 32, K)
    assert lay.sf_off == 288
    good = dict(x=16, stride=768, hidden=384, idx=64, w=None, tokens=4, topk=K, src_base=0, dst_slot=128,
                send_offsets=256, ranks=1, packed=512, dest_bases=None, row_bytes=lay.row_bytes, dest_rows=4,
                sf_off=lay.sf_off, idx_off=lay.idx_off, w_off=lay.w_off, src_off=lay.src_off, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_pack_cast_fp6_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_pack_cast_fp6_mx' in err()
    _rejects(lib, 'deepep_dispatch_pack_cast_fp6_mx', good,
             [dict(hidden=64, stride=128), dict(x=None), dict(x=24), dict(stride=760), dict(packed=520),
              dict(sf_off=286), dict(sf_off=284), dict(sf_off=192), dict(idx_off=lay.sf_off),
              dict(idx_off=lay.sf_off + 8), dict(topk=0), dict(ranks=65), dict(row_bytes=lay.src_off)])
    assert b'row layout' in err()
    assert lib.deepep_dispatch_pack_cast_fp6_mx(*dict(good, tokens=0).values()) == 0

    good = dict(packed=16, row_bytes=128, w_off=0, recv=4, topk=K, meta=64, expanded=0, x=128, stride=768, hidden=384,
                max_tokens=4, recv_x=256, recv_sf=516, recv_w=None, out_rows=4, inv=None, offsets=None, end=None,
                experts=0, row_map=None, flag=None, stream=None)
    _rejects(lib, 'deepep_dispatch_copy_cast_fp6_mx', good, [dict(hidden=96, stride=192)])
    assert b'multiple of 128' in err() and b'dispatch_copy_cast_fp6_mx' in err()
    _rejects(lib, 'deepep_dispatch_copy_cast_fp6_mx', good,
             [dict(hidden=0), dict(hidden=64, stride=128), dict(x=None), dict(x=136), dict(stride=760),
              dict(recv_x=None), dict(recv_x=264), dict(recv_sf=None), dict(recv_sf=518), dict(meta=None),
              dict(max_tokens=0), dict(inv=1024)])
    assert lib.deepep_dispatch_copy_cast_fp6_mx(*dict(good, recv=0).values()) == 0


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
            deepep_amd.per_token_cast_to_fp6(arg)
    with pytest.raises(_Loaded):                               # well-formed: on to the library
        deepep_amd.per_token_cast_to_fp6(x)
    q, sf = deepep_amd.per_token_cast_to_fp6(x[:0])            # no rows: no launch
    assert (q.dtype, tuple(q.shape), sf.dtype, tuple(sf.shape)) == (torch.uint8, (0, 288), torch.uint8, (0, 12))


def test_public_cast_back_takes_strided_rows_and_both_dtypes_of_scales(no_library):
    import deepep_amd
    q = torch.zeros((4, 288), dtype=torch.uint8)
    sf = torch.zeros((4, 12), dtype=torch.uint8)
    for rows in (q, torch.zeros((4, 320), dtype=torch.uint8)[:, :288]):
        for scales in (sf, sf.view(torch.float8_e8m0fnu), torch.zeros((12, 4), dtype=torch.uint8).t()):
            with pytest.raises(_Loaded):
                deepep_amd.per_token_cast_back_fp6(rows, scales)
    for what, rows, scales in (('e4m3fn rows', q.view(torch.float8_e4m3fn), sf),
                               ('fp4 rows', q.view(torch.float4_e2m1fn_x2), sf),
                               ('bf16 rows', torch.zeros((4, 288), dtype=torch.bfloat16), sf),
                               ('H % 128 != 0', q[:, :72], sf[:, :3]),
                               ('rows of H / 2 bytes', q[:, :192], sf),
                               ('the per-128 shape', q, sf[:, :3]),
                               ('a wrong row count', q, sf[:3]),
                               ('1-D scales', q, sf.reshape(-1)),
                               ('fp32 scales', q, sf.float()),
                               ('int32 scales', q, torch.zeros((4, 3), dtype=torch.int32)),
                               ('no scales', q, None)):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_back_fp6(rows, scales)
    out = deepep_amd.per_token_cast_back_fp6(q[:0], sf[:0])
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 384)
