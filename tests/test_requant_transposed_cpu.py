"""requant_mxfp8_transposed / requant_mxfp4_transposed / requant_mxfp6_transposed without a GPU: the references'
self-checks at the GPU tests' smallest shapes, every argument rejection raises before the library is loaded, and the
entries stand in every layer (the public names and their deep_ep aliases, the C header, the ctypes table, the source
hash and the build list) with the ABI version unchanged, the wrappers on their own mixin and the cast backs'
conversions stated once."""
import os
import re

import pytest
import torch

from tests.requant_t_ref import ALL, BY_NAME, code_difference, pair_and_ref, rounding_difference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
forms = pytest.mark.parametrize('form', ALL, ids=repr)
PUBLIC = ('requant_mxfp8_transposed', 'requant_mxfp4_transposed', 'requant_mxfp6_transposed')
ENTRIES = {'deepep_requant_fp8_mx_transposed': 11, 'deepep_requant_fp4_mx_transposed': 10,
           'deepep_requant_fp6_mx_transposed': 10}


# ----------------------------------------------------------------------------- the references alone
@pytest.mark.parametrize('N,H', [(128, 128), (384, 640)])
@pytest.mark.parametrize('name', ['fp32', 'mx', 'fp4', 'fp6'])
def test_requantised_codes_are_not_the_transposed_input_codes(name, N, H):
    """(i) measured 0.91 / 0.92 (MXFP8), 0.81 / 0.82 (FP4), 0.88 / 0.90 (FP6) at these shapes."""
    share = code_difference(BY_NAME[name], N, H)
    assert share > 0.5, f'only {share:.2f} of the codes differ from the transposed input codes'


@pytest.mark.parametrize('N,H', [(128, 128), (384, 640)])
def test_the_cast_backs_rounding_shows_in_the_reference(N, H):
    """(ii) measured 2.0 % and 2.4 % of the q_t bytes at these shapes."""
    share = rounding_difference(N, H)
    assert share > 0.005, f'only {share:.4f} of the bytes change under a truncating cast back'


@forms
def test_the_reference_has_the_contracts_shapes(form):
    N, H = 128, 512
    (q, sf), (q_t, sf_t) = pair_and_ref(form, N, H)
    assert tuple(q.shape) == (N, form.row_bytes(H))
    assert q_t.dtype == torch.uint8 and tuple(q_t.shape) == (H, form.row_bytes(N))
    assert sf_t.dtype == torch.uint8 and tuple(sf_t.shape) == (H, N // 32)


# ----------------------------------------------------------------------------- rejections
@pytest.fixture
def no_library(monkeypatch):
    from deepep_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', refuse)


def _rows(form, N, H, dtype=None):
    dtype = dtype or (torch.uint8 if form.fmt else torch.float8_e4m3fn)
    return torch.zeros((N, form.row_bytes(H)), dtype=torch.uint8).view(dtype)


def _factors(form, N, H):
    if form.name == 'fp32':
        return torch.ones((N, H // 128), dtype=torch.float32)
    if form.name == 'ue8m0':
        return torch.zeros((N, H // 512), dtype=torch.int32)
    return torch.zeros((N, H // 32), dtype=torch.uint8)


def _cases(form):
    """(id, rows, factors) that the public function must refuse."""
    N, H = 128, 512
    q, sf = _rows(form, N, H), _factors(form, N, H)
    cols = sf.shape[1]
    wrong_row_dtype = torch.float8_e4m3fn if form.fmt else torch.uint8
    cases = [
        ('rows_none', None, sf),
        ('rows_1d', q[0], sf),
        ('rows_3d', q.view(2, 64, -1), sf),
        ('rows_dtype', _rows(form, N, H, wrong_row_dtype), sf),
        ('rows_bf16', torch.zeros((N, H), dtype=torch.bfloat16), sf),
        ('h0', _rows(form, N, 0), _factors(form, N, 0)),
        ('h64', _rows(form, N, 64), torch.zeros((N, 2), dtype=sf.dtype)),
        ('h192', _rows(form, N, 192), torch.zeros((N, 6), dtype=sf.dtype)),
        ('n64', _rows(form, 64, H), _factors(form, 64, H)),
        ('n130', _rows(form, 130, H), _factors(form, 130, H)),
        ('sf_none', q, None),
        ('sf_bf16', q, torch.zeros((N, cols), dtype=torch.bfloat16)),
        ('sf_int64', q, torch.zeros((N, cols), dtype=torch.int64)),
        ('sf_1d', q, sf[:, 0]),
        ('sf_rows', q, _factors(form, N + 128, H)),
        ('sf_cols', q, torch.zeros((N, cols + 1), dtype=sf.dtype)),
        ('sf_other_device', q, sf.to('meta')),
        ('cpu', q, sf),
    ]
    if form.name == 'ue8m0':
        cases.append(('h640_packed', _rows(form, N, 640), torch.zeros((N, 1), dtype=torch.int32)))
        cases.append(('h128_packed', _rows(form, N, 128), torch.zeros((N, 1), dtype=torch.int32)))
    if form.fmt:                                            # FP4 and FP6 take exponent bytes per 32 columns only
        cases.append(('sf_fp32', q, torch.ones((N, H // 128), dtype=torch.float32)))
        cases.append(('sf_packed', q, torch.zeros((N, H // 512), dtype=torch.int32)))
    return cases


@pytest.mark.parametrize('form,case', [(f, c) for f in ALL for c in _cases(f)],
                         ids=lambda v: repr(v) if not isinstance(v, tuple) else v[0])
def test_rejections_raise_before_the_library_is_loaded(no_library, form, case):
    import deepep_amd
    _, q, sf = case
    with pytest.raises(RuntimeError, match=f'^Assertion failed: {form.public} '):
        getattr(deepep_amd, form.public)(q, sf)


@forms
def test_strided_columns_and_misaligned_rows_are_refused(no_library, monkeypatch, form):
    """The stride checks stand behind the device check: tensors that claim to be on the GPU stand for GPU tensors."""
    import deepep_amd
    N, H = 128, 512
    sf = _factors(form, N, H)
    wide = _rows(form, N, 2 * H)
    odd = torch.zeros(N * (form.row_bytes(H) + 8), dtype=torch.uint8).as_strided(
        (N, form.row_bytes(H)), (form.row_bytes(H) + 8, 1)).view(wide.dtype)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    for q in (wide[:, ::2], odd):
        with pytest.raises(RuntimeError, match=f'^Assertion failed: {form.public} '):
            getattr(deepep_amd, form.public)(q, sf)


@forms
def test_no_rows_need_no_library(no_library, monkeypatch, form):
    """N == 0 returns the shapes and dtypes without loading the library (an empty tensor that claims to be on the GPU
    stands for one here)."""
    import deepep_amd
    H = 512
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    q_t, sf_t = getattr(deepep_amd, form.public)(_rows(form, 0, H), _factors(form, 0, H))
    assert tuple(q_t.shape) == (H, 0) and tuple(sf_t.shape) == (H, 0)
    assert q_t.dtype == (torch.uint8 if form.fmt else torch.float8_e4m3fn) and sf_t.dtype == torch.uint8


# ----------------------------------------------------------------------------- every layer
def test_the_names_are_public_and_aliased():
    import deep_ep
    import deepep_amd
    assert {f.public for f in ALL} == set(PUBLIC)
    for name in PUBLIC:
        assert name in deepep_amd.__all__
        assert getattr(deep_ep, name) is getattr(deepep_amd, name)
    assert deepep_amd.__build_version__ == '0.8.0'


def test_the_c_entries_are_declared_in_the_header_and_in_the_table():
    import __graft_entry__ as entry
    from deepep_amd import _lib
    with open(os.path.join(ROOT, 'include', 'deepep_amd.h')) as f:
        header = f.read()
    assert {f.entry for f in ALL} == set(ENTRIES)
    for name, count in ENTRIES.items():
        decl = re.search(r'\nint %s\(([^;]*)\);' % name, header)
        assert decl is not None, name
        params = [p.strip() for p in decl.group(1).replace('\n', ' ').split(',')]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._I and len(args) == len(params) == count
        for p, a in zip(params, args):
            want = _lib._P if ('*' in p or 'deepep_stream_t' in p) else _lib._I64 if p.startswith('int64_t') else _lib._I
            assert a is want, (name, p)
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for form, value in (('FP32', _lib.SF_FORM_FP32), ('UE8M0_PACKED', _lib.SF_FORM_UE8M0_PACKED), ('MX', _lib.SF_FORM_MX)):
        assert re.search(r'#define DEEPEP_SF_FORM_%s +%d\b' % (form, value), header)
    # additive: the version stays
    assert _lib.ABI_VERSION == 14 and re.search(r'#define DEEPEP_AMD_ABI_VERSION 14\b', header)
    # built, and in the source hash (no stale binary): the kernel file and the headers it shares with the cast backs
    assert any(s.endswith('requant_t.hip') for s in entry.HIP_SOURCES)
    for name in ('requant_t.hip', 'fp4_dequant.h', 'fp6_dequant.h', 'fp8_dequant.h'):
        assert any(s.endswith(os.sep + name) for s in _lib.SOURCES), name


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_the_c_entries_are_exported_and_reject_bad_arguments_without_a_gpu(lib, name):
    """An error code with text, nothing launched (the pointers are never dereferenced on the host: aligned numbers
    stand for them)."""
    fn = getattr(lib, name)
    fp8 = ENTRIES[name] == 11
    row = {'deepep_requant_fp8_mx_transposed': 128, 'deepep_requant_fp4_mx_transposed': 64,
           'deepep_requant_fp6_mx_transposed': 96}[name]
    q, sf, q_t, sf_t = 0x1000, 0x2000, 0x3000, 0x4000

    def call(q=q, stride=256, sf=sf, rs=4, cs=1, form=2, q_t=q_t, sf_t=sf_t, n=128, h=128):
        return fn(q, stride, sf, rs, cs, *((form,) if fp8 else ()), q_t, sf_t, n, h, None)

    assert lib.deepep_amd_abi_version() == 14
    assert call(q=None, sf=None, q_t=None, sf_t=None, n=0) == 0               # no rows: DEEPEP_OK, no launch
    cases = [(dict(h=0), b'hidden'), (dict(h=192), b'hidden'), (dict(n=64), b'num_rows'), (dict(n=-128), b'num_rows'),
             (dict(q=None), b'null or misaligned'), (dict(sf=None), b'null or misaligned'),
             (dict(q=q + 8), b'null or misaligned'), (dict(q_t=q_t + 4), b'null or misaligned'),
             (dict(sf_t=sf_t + 2), b'null or misaligned'), (dict(stride=row - 16), b'row stride'),
             (dict(stride=row + 8), b'row stride'), (dict(rs=-4), b'negative'), (dict(cs=-1), b'negative'),
             (dict(stride=(1 << 24) + 16), b'2^24'), (dict(stride=1 << 26, h=1 << 25), b'2^24'),
             (dict(n=1 << 29), b'2^29')]
    if fp8:
        cases += [(dict(form=3), b'sf_form'), (dict(form=-1), b'sf_form'), (dict(form=1, h=640), b'512'),
                  (dict(form=0, sf=sf + 2), b'null or misaligned'), (dict(form=1, h=512, sf=sf + 1), b'null or misaligned')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        text = lib.deepep_amd_last_error()
        assert name[len('deepep_'):].encode() in text and word in text, (kw, text)


def test_the_wrappers_live_on_their_own_mixin():
    from deepep_amd import kernels
    from deepep_amd.kernels import HipKernels, RequantTransposedKernels
    names = sorted({f.wrapper for f in ALL})
    public = sorted(n for n, v in vars(RequantTransposedKernels).items() if callable(v) and not n.startswith('_'))
    assert public == names
    others = [c for c in vars(kernels).values()
              if isinstance(c, type) and c.__name__.endswith('Kernels') and c is not RequantTransposedKernels]
    assert HipKernels in others and len(others) >= 6
    for cls in others:
        for name in names:
            assert name not in vars(cls), (cls.__name__, name)
    assert issubclass(HipKernels, RequantTransposedKernels)
    for name in names:
        assert getattr(HipKernels, name) is getattr(RequantTransposedKernels, name)


def test_the_cast_backs_conversions_are_stated_once():
    """dequant8_fp4 and dequant32_fp6 live in headers of their own, as fp8_dequant.h's do, and both users include
    them; requant_t.hip names no conversion to fp32 itself."""
    csrc = os.path.join(ROOT, 'deepep_amd', 'csrc')
    files = [n for n in sorted(os.listdir(csrc)) if n.endswith(('.hip', '.h'))]
    text = {n: open(os.path.join(csrc, n)).read() for n in files}
    for needle, home in (('dequant8_fp4(uint32_t', 'fp4_dequant.h'), ('void dequant32_fp6(', 'fp6_dequant.h'),
                         ('__builtin_amdgcn_cvt_scalef32_pk_f32_fp4', 'fp4_dequant.h'),
                         ('__builtin_amdgcn_cvt_scalef32_pk32_f32_fp6', 'fp6_dequant.h'),
                         ('__builtin_amdgcn_cvt_pk_f32_fp8', 'fp8_dequant.h')):
        assert [n for n in files if needle in text[n]] == [home], needle
    for user, header in (('fp4_cast.hip', 'fp4_dequant.h'), ('fp6_cast.hip', 'fp6_dequant.h'),
                         ('requant_t.hip', 'fp4_dequant.h'), ('requant_t.hip', 'fp6_dequant.h')):
        assert f'#include "{header}"' in text[user], (user, header)
    code = re.sub(r'//[^\n]*', '', text['requant_t.hip'])
    for call in ('deepep::dequant8(', 'deepep::dequant8_fp4(', 'deepep::dequant32_fp6('):
        assert call in code, call
    assert 'convertvector' not in code and '6.0f' not in code and '7.5f' not in code and '448' not in code
