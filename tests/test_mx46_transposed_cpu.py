"""cast_to_mxfp4_transposed / cast_to_mxfp6_transposed without a GPU: the reference's inputs tell the token axis from
the column axis at the GPU tests' shapes, the contract restated per block and column, every argument rejection raises
before the library is loaded, and the entries stand in every layer (the public names and their deep_ep aliases, the C
header, the ctypes table, the source hash and the build list) with the ABI version unchanged, the wrappers on their own
mixin and every shared definition stated once."""
import os
import re

import pytest
import torch

from tests.mxt46_ref import FORMATS, FP4, FP6
from tests.mxt_ref import mxt_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fmts = pytest.mark.parametrize('fmt', FORMATS, ids=repr)


@fmts
@pytest.mark.parametrize('N,H', [(128, 128), (384, 640), (640, 128), (128, 7168)])
def test_the_inputs_tell_the_two_axes_apart(fmt, N, H):
    x = mxt_input(N, H, 1000 + H)
    fmt.self_check(x)
    if (N, H) == (384, 640):
        # and plain randn rows would not: one binade, so far more codes of the two pairs agree
        plain = torch.randn((N, H), generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
        assert fmt.axis_difference(plain) < fmt.axis_difference(x)


@fmts
def test_the_reference_restated_per_block_and_column(fmt):
    """The pair of the transposed matrix against the contract's words, per (block g of 32 tokens, column c): the
    exponent byte sf_t[c, g] from the block's amax under the ceiling rule, and the code of token 32g + r in its place
    -- FP4: nibble r & 1 of byte 16g + r / 2; FP6: bits 6r + 5 : 6r of the 192-bit string at bytes [24g, 24g + 24)."""
    N, H = 256, 128
    x = mxt_input(N, H, 1)
    q_t, sf_t = fmt.transposed_pair(x)
    assert tuple(q_t.shape) == (H, fmt.row_bytes(N)) and tuple(sf_t.shape) == (H, N // 32)
    f = x.float()
    amax = f.view(N // 32, 32, H).abs().amax(dim=1).clamp_min(1e-4)           # [block, column]
    bits = (amax * torch.tensor(1.0 / fmt.max_value, dtype=torch.float32)).view(torch.int32)
    byte = ((bits >> 23) & 0xff) + ((bits & 0x7fffff) != 0).to(torch.int32)
    assert torch.equal(sf_t, byte.to(torch.uint8).t().contiguous())
    # the codes: the row-wise code function of the transposed matrix is the contract's table applied per column
    codes, _ = fmt.codes(x.t().contiguous())                                  # [column, token]
    for c in (0, 37, 127):
        for g in (0, 3, 7):
            block = q_t[c, fmt.block_bytes * g:fmt.block_bytes * (g + 1)].tolist()
            if fmt is FP4:
                got = [(block[r // 2] >> (4 * (r & 1))) & 0xf for r in range(32)]
            else:
                word = int.from_bytes(bytes(block), 'little')
                got = [(word >> (6 * r)) & 63 for r in range(32)]
            assert got == codes[c, 32 * g:32 * g + 32].tolist(), (c, g)
    # the sign rule: -0.0 keeps its sign bit
    x = torch.zeros((128, 128), dtype=torch.bfloat16)
    x[5, 9] = -0.0
    assert int(fmt.unpack(fmt.transposed_pair(x)[0])[9, 5]) == 1 << (fmt.bits - 1)


@pytest.fixture
def no_library(monkeypatch):
    from deepep_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', refuse)


def _bf16(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


@pytest.mark.parametrize('make', [
    lambda: None,
    lambda: _bf16(128),                                   # 1-D
    lambda: _bf16(2, 128, 128),                           # 3-D
    lambda: torch.zeros((128, 128), dtype=torch.float16),
    lambda: torch.zeros((128, 128), dtype=torch.float32),
    lambda: _bf16(128, 0),                                # H > 0
    lambda: _bf16(128, 64),                               # H % 128
    lambda: _bf16(128, 192),
    lambda: _bf16(64, 128),                               # N % 128
    lambda: _bf16(130, 128),
    lambda: _bf16(128, 256)[:, ::2],                      # column stride 2
    lambda: _bf16(128, 128).t(),                          # column stride 128
    lambda: _bf16(128 * 132)[:128 * 132].as_strided((128, 128), (132, 1)),    # row stride no multiple of 8
    lambda: _bf16(128, 128),                              # not on the GPU
], ids=['none', '1d', '3d', 'fp16', 'fp32', 'h0', 'h64', 'h192', 'n64', 'n130', 'colstride2', 'transposed',
        'rowstride132', 'cpu'])
@pytest.mark.parametrize('with_rowwise', [False, True])
@fmts
def test_rejections_raise_before_the_library_is_loaded(no_library, fmt, make, with_rowwise):
    import deepep_amd
    with pytest.raises(RuntimeError, match=f'^Assertion failed: {fmt.public} '):
        getattr(deepep_amd, fmt.public)(make(), with_rowwise=with_rowwise)


@fmts
def test_no_rows_need_no_library(no_library, monkeypatch, fmt):
    """N == 0 returns the shapes and dtypes without loading the library (an empty tensor that claims to be on the GPU
    stands for one here)."""
    import deepep_amd
    x = _bf16(0, 256)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    q_t, sf_t = getattr(deepep_amd, fmt.public)(x)
    (q, sf), (q_t2, sf_t2) = getattr(deepep_amd, fmt.public)(x, with_rowwise=True)
    for t, shape in ((q_t, (256, 0)), (sf_t, (256, 0)), (q_t2, (256, 0)), (sf_t2, (256, 0)),
                     (q, (0, fmt.row_bytes(256))), (sf, (0, 8))):
        assert t.dtype == torch.uint8 and tuple(t.shape) == shape


@fmts
def test_the_name_is_public_and_aliased(fmt):
    import deep_ep
    import deepep_amd
    assert fmt.public in deepep_amd.__all__
    assert getattr(deep_ep, fmt.public) is getattr(deepep_amd, fmt.public)


@fmts
def test_the_c_entry_is_declared_in_the_header_and_in_the_table(fmt):
    import __graft_entry__ as entry
    from deepep_amd import _lib
    with open(os.path.join(ROOT, 'include', 'deepep_amd.h')) as f:
        header = f.read()
    decl = re.search(r'\nint %s\(([^;]*)\);' % fmt.entry, header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[fmt.entry]
    assert res is _lib._I and len(args) == len(params) == 9
    for p, a in zip(params, args):
        want = _lib._P if ('*' in p or 'deepep_stream_t' in p) else _lib._I64 if p.startswith('int64_t') else _lib._I
        assert a is want, p
    # the argument list of the MXFP8 entry
    assert (res, args) == _lib.SIGNATURES['deepep_cast_fp8_mx_transposed']
    # additive: the version stays
    assert _lib.ABI_VERSION == 14 and re.search(r'#define DEEPEP_AMD_ABI_VERSION 14\b', header)
    # built, and in the source hash (no stale binary): the kernel file and the headers it shares with the row-wise casts
    assert any(s.endswith('fp46_cast_t.hip') for s in entry.HIP_SOURCES)
    for name in ('fp46_cast_t.hip', 'fp4_cast_common.h', 'fp6_cast_common.h'):
        assert any(s.endswith(os.sep + name) for s in _lib.SOURCES), name
    assert fmt.entry in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


@fmts
def test_the_c_entry_is_exported_and_rejects_bad_arguments_without_a_gpu(lib, fmt):
    """The checks of deepep_cast_fp8_mx_transposed: an error code with text, nothing launched (the pointers are never
    dereferenced on the host: 16-byte aligned numbers stand for them)."""
    fn = getattr(lib, fmt.entry)
    assert lib.deepep_amd_abi_version() == 14
    x, q_t, sf_t, q, sf = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert fn(None, 256, None, None, None, None, 0, 128, None) == 0          # no rows: DEEPEP_OK, no launch
    for args, word in (
            ((x, 256, q_t, sf_t, None, None, 128, 0, None), b'hidden'),
            ((x, 256, q_t, sf_t, None, None, 128, 192, None), b'hidden'),
            ((x, 256, q_t, sf_t, None, None, 64, 128, None), b'num_rows'),
            ((x, 256, q_t, sf_t, None, None, -128, 128, None), b'num_rows'),
            ((None, 256, q_t, sf_t, None, None, 128, 128, None), b'null or misaligned'),
            ((x + 8, 256, q_t, sf_t, None, None, 128, 128, None), b'null or misaligned'),
            ((x, 256, q_t + 4, sf_t, None, None, 128, 128, None), b'null or misaligned'),
            ((x, 256, q_t, sf_t + 2, None, None, 128, 128, None), b'null or misaligned'),
            ((x, 256, q_t, sf_t, q, None, 128, 128, None), b'both q and sf'),
            ((x, 256, q_t, sf_t, None, sf, 128, 128, None), b'both q and sf'),
            ((x, 256, q_t, sf_t, q + 8, sf, 128, 128, None), b'misaligned row-wise'),
            ((x, 256, q_t, sf_t, q, sf + 1, 128, 128, None), b'misaligned row-wise'),
            ((x, 248, q_t, sf_t, None, None, 128, 128, None), b'row stride'),
            ((x, 264, q_t, sf_t, None, None, 128, 128, None), b'row stride'),
            ((x, (1 << 24) + 16, q_t, sf_t, None, None, 128, 128, None), b'2^24'),
            ((x, 1 << 26, q_t, sf_t, None, None, 128, 1 << 25, None), b'2^24'),
            ((x, 256, q_t, sf_t, None, None, 1 << 29, 128, None), b'2^29')):
        assert fn(*args) == -1, args
        text = lib.deepep_amd_last_error()
        assert fmt.wrapper.encode() in text and word in text, (args, text)


def test_the_wrappers_live_on_their_own_mixin():
    from deepep_amd.kernels import (Fp4Kernels, Fp6Kernels, HipKernels, LogfmtKernels, TransposedCastKernels,
                                    TransposedFp4Fp6Kernels)
    names = sorted(f.wrapper for f in FORMATS)
    public = sorted(n for n, v in vars(TransposedFp4Fp6Kernels).items() if callable(v) and not n.startswith('_'))
    assert public == names
    for cls in (HipKernels, Fp4Kernels, Fp6Kernels, LogfmtKernels, TransposedCastKernels):
        for name in names:
            assert name not in vars(cls), (cls.__name__, name)
    assert issubclass(HipKernels, TransposedFp4Fp6Kernels)
    for name in names:
        assert getattr(HipKernels, name) is getattr(TransposedFp4Fp6Kernels, name)


def test_the_shared_definitions_are_not_restated():
    """The scale rules, the two conversions and a lane's cast of a group have one definition each, in the shared
    headers; neither the row-wise files nor the transposed one states a rule's constant or names a conversion."""
    csrc = os.path.join(ROOT, 'deepep_amd', 'csrc')
    files = ('fp4_cast.hip', 'fp6_cast.hip', 'fp46_cast_t.hip', 'fp4_cast_common.h', 'fp6_cast_common.h',
             'cast_common.h')
    text = {n: open(os.path.join(csrc, n)).read() for n in files}
    for needle, home in (('uint32_t cvt8_fp4(', 'fp4_cast_common.h'), ('struct Fp4Lane', 'fp4_cast_common.h'),
                         ('> cast_group_fp4(', 'fp4_cast_common.h'), ('uint32_t fp4_exp_byte(', 'fp4_cast_common.h'),
                         ('kFp4Max = 6.0f', 'fp4_cast_common.h'), ('kFp4MaxRcp = 1.0f / kFp4Max', 'fp4_cast_common.h'),
                         ('__builtin_amdgcn_cvt_scalef32_pk_fp4_bf16', 'fp4_cast_common.h'),
                         ('u32x6 cvt32_fp6(', 'fp6_cast_common.h'), ('struct Fp6Lane', 'fp6_cast_common.h'),
                         ('Fp6Lane cast_group_fp6(', 'fp6_cast_common.h'), ('uint32_t fp6_exp_byte(', 'fp6_cast_common.h'),
                         ('kFp6Max = 7.5f', 'fp6_cast_common.h'), ('kFp6MaxRcp = 1.0f / kFp6Max', 'fp6_cast_common.h'),
                         ('__builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16', 'fp6_cast_common.h'),
                         ('float amax_floor(', 'cast_common.h')):
        assert [n for n in files if needle in text[n]] == [home], needle
    for n in ('fp4_cast.hip', 'fp6_cast.hip', 'fp46_cast_t.hip'):
        code = re.sub(r'//[^\n]*', '', text[n])
        assert '6.0f' not in code and '7.5f' not in code and '0x7fffffu' not in code, n
    assert '#include "fp4_cast_common.h"' in text['fp4_cast.hip']
    assert '#include "fp6_cast_common.h"' in text['fp6_cast.hip']
    assert '#include "fp4_cast_common.h"' in text['fp46_cast_t.hip']
    assert '#include "fp6_cast_common.h"' in text['fp46_cast_t.hip']
