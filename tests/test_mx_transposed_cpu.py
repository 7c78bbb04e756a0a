"""cast_to_mxfp8_transposed without a GPU: the reference's inputs tell the token axis from the column axis, every
argument rejection raises before the library is loaded, and the entry stands in every layer (the public name and its
deep_ep alias, the C header, the ctypes table, the source hash and the build list) with the ABI version unchanged and
the wrapper on its own mixin."""
import os
import re

import pytest
import torch

from tests.mxt_ref import axis_difference, mxt_input, mxt_pair, self_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_inputs_tell_the_two_axes_apart():
    x = mxt_input(256, 384, 0)
    self_check(x)
    # and plain randn rows would not: one binade, so most bytes of the two pairs agree
    plain = torch.randn((256, 384), generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert axis_difference(plain) < axis_difference(x)


def test_the_reference_restated_per_block_and_column():
    """mx_pair of the transposed matrix against the contract's words: per (block of 32 tokens, column)."""
    x = mxt_input(128, 128, 1)
    q_t, sf_t = mxt_pair(x)
    f = x.float()
    amax = f.view(4, 32, 128).abs().amax(dim=1).clamp_min(1e-4)               # [block, column]
    bits = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    assert torch.equal(sf_t, (e + 127).to(torch.uint8).t().contiguous())
    scaled = f.view(4, 32, 128) * torch.exp2(-e.float()).unsqueeze(1)
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).view(128, 128)
    assert torch.equal(q_t, q.t().contiguous())


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
def test_rejections_raise_before_the_library_is_loaded(no_library, make, with_rowwise):
    import deepep_amd
    with pytest.raises(RuntimeError, match='^Assertion failed: cast_to_mxfp8_transposed'):
        deepep_amd.cast_to_mxfp8_transposed(make(), with_rowwise=with_rowwise)


def test_the_name_is_public_and_aliased():
    import deep_ep
    import deepep_amd
    assert 'cast_to_mxfp8_transposed' in deepep_amd.__all__
    assert deep_ep.cast_to_mxfp8_transposed is deepep_amd.cast_to_mxfp8_transposed


def test_the_c_entry_is_declared_in_the_header_and_in_the_table():
    import __graft_entry__ as entry
    from deepep_amd import _lib
    with open(os.path.join(ROOT, 'include', 'deepep_amd.h')) as f:
        header = f.read()
    decl = re.search(r'\nint deepep_cast_fp8_mx_transposed\(([^;]*)\);', header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES['deepep_cast_fp8_mx_transposed']
    assert res is _lib._I and len(args) == len(params) == 9
    for p, a in zip(params, args):
        want = _lib._P if ('*' in p or 'deepep_stream_t' in p) else _lib._I64 if p.startswith('int64_t') else _lib._I
        assert a is want, p
    # additive: the version stays
    assert _lib.ABI_VERSION == 14 and re.search(r'#define DEEPEP_AMD_ABI_VERSION 14\b', header)
    # built, and in the source hash (no stale binary): the kernel file and the header it shares with fp8_cast.hip
    assert any(s.endswith('fp8_cast_t.hip') for s in entry.HIP_SOURCES)
    for name in ('fp8_cast_t.hip', 'fp8_cast_common.h'):
        assert any(s.endswith(os.sep + name) for s in _lib.SOURCES), name


def test_the_wrapper_lives_on_its_own_mixin():
    from deepep_amd.kernels import Fp4Kernels, Fp6Kernels, HipKernels, LogfmtKernels, TransposedCastKernels
    public = sorted(n for n, v in vars(TransposedCastKernels).items() if callable(v) and not n.startswith('_'))
    assert public == ['cast_fp8_mx_transposed']
    for cls in (HipKernels, Fp4Kernels, Fp6Kernels, LogfmtKernels):
        assert 'cast_fp8_mx_transposed' not in vars(cls), cls.__name__
    assert issubclass(HipKernels, TransposedCastKernels)
    assert HipKernels.cast_fp8_mx_transposed is TransposedCastKernels.cast_fp8_mx_transposed


def test_the_shared_definitions_are_not_restated():
    """The scale rule, the exponent byte and the e4m3fn conversion have one definition each, in the shared headers."""
    csrc = os.path.join(ROOT, 'deepep_amd', 'csrc')
    text = {n: open(os.path.join(csrc, n)).read() for n in ('fp8_cast.hip', 'fp8_cast_t.hip', 'fp8_cast_common.h',
                                                             'cast_common.h')}
    for needle, home in (('void group_scales(', 'fp8_cast_common.h'), ('u32x2 cvt8(', 'fp8_cast_common.h'),
                         ('uint32_t ue8m0_byte(', 'cast_common.h'), ('struct SfFormat<Sf::kExp32>', 'fp8_cast_common.h')):
        assert [n for n, t in text.items() if needle in t] == [home], needle
    for n in ('fp8_cast.hip', 'fp8_cast_t.hip'):
        assert '#include "fp8_cast_common.h"' in text[n]
        assert '__builtin_amdgcn_cvt_pk_fp8_f32' not in text[n]
