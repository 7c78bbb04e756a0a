"""The table of FP8 scale-factor formats (deepep_amd.kernels.SfFormat) without a GPU: its entries exist with the
argument lists it promises, its shapes are the documented ones, and its two lookups resolve as the wrappers'
keywords and the scale-factor dtypes say."""
import ctypes

import pytest
import torch

from deepep_amd import _lib
from deepep_amd.kernels import (MX_SF_DTYPES, SF_FORMATS, SF_FP32, SF_MXFP8, SF_UE8M0, RowLayout, sf_format,
                                sf_format_of)

ENTRIES = ('cast_fp8', 'cast_back_fp8', 'dispatch_pack_cast', 'dispatch_copy_cast')
# where the plain entries take round_scale (include/deepep_amd.h: the int after hidden); the cast back never does
ROUND_SCALE_AT = {'cast_fp8': 4, 'dispatch_pack_cast': 3, 'dispatch_copy_cast': 10}
# the documented scale-factor tensors of a row of H columns: dtype, elements, bytes
DOCUMENTED = {SF_FP32: (torch.float32, lambda H: H // 128, lambda H: H // 128 * 4),
              SF_UE8M0: (torch.int32, lambda H: H // 512, lambda H: H // 128),
              SF_MXFP8: (torch.uint8, lambda H: H // 32, lambda H: H // 32)}


def test_the_table_holds_the_three_formats():
    assert SF_FORMATS == (SF_FP32, SF_UE8M0, SF_MXFP8)
    assert [f.suffix for f in SF_FORMATS] == ['', '_ue8m0', '_mx']
    assert [f.kw for f in SF_FORMATS] == [{}, {'ue8m0': True}, {'mx': True}]
    assert [f.multiple for f in SF_FORMATS] == [128, 512, 128]
    assert [f.needs_round_scale for f in SF_FORMATS] == [False, True, True]


@pytest.mark.parametrize('fmt', SF_FORMATS, ids=lambda f: f.name)
def test_entries_exist_and_take_round_scale_where_the_table_says(fmt):
    """The entries of a format that needs round_scale are the plain entries' without that one int argument; the cast
    back never takes it."""
    for entry in ENTRIES:
        assert 'deepep_' + entry + fmt.suffix in _lib.SIGNATURES, (entry, fmt.name)
        res, args = _lib.SIGNATURES['deepep_' + entry + fmt.suffix]
        expected = list(_lib.SIGNATURES['deepep_' + entry][1])
        if fmt.needs_round_scale and entry in ROUND_SCALE_AT:
            assert expected.pop(ROUND_SCALE_AT[entry]) is ctypes.c_int
        assert res is ctypes.c_int and args == expected, (entry, fmt.name)
    assert fmt.scale_arg(True) == (() if fmt.needs_round_scale else (1,))
    assert fmt.scale_arg(False) == (() if fmt.needs_round_scale else (0,))


@pytest.mark.parametrize('fmt,H', [(f, H) for f in SF_FORMATS for H in (128, 512, 640, 7168) if H % f.multiple == 0],
                         ids=lambda v: getattr(v, 'name', v))
def test_shapes_are_the_documented_ones(fmt, H):
    """(a hidden size that is no multiple of the format's is no case: packed UE8M0 takes 512 and 7168 only)"""
    dtype, elems, row_bytes = DOCUMENTED[fmt]
    assert fmt.dtype == dtype and fmt.elems(H) == elems(H) and fmt.row_bytes(H) == row_bytes(H)
    assert fmt.row_bytes(H) == fmt.elems(H) * torch.empty((), dtype=dtype).element_size()
    fmt.require('test', H, True)
    # the packed row of a casting dispatch: what ElasticBuffer._dispatch builds for the format
    for K in (1, 8):
        assert RowLayout.make(H, fmt.row_bytes(H), K) == RowLayout.make(H, row_bytes(H), K)
        assert RowLayout.make(H, fmt.row_bytes(H), K).sf_bytes == row_bytes(H)


def test_require_names_the_multiple_and_round_scale():
    for fmt in SF_FORMATS:
        with pytest.raises(RuntimeError, match=f'multiple of {fmt.multiple}'):
            fmt.require('test', fmt.multiple + 64, True)
    SF_FP32.require('test', 128, False)
    for fmt in (SF_UE8M0, SF_MXFP8):
        with pytest.raises(RuntimeError, match='round_scale'):
            fmt.require('test', 512, False)


def test_lookup_from_the_wrappers_keywords():
    assert sf_format() is SF_FP32 and sf_format(ue8m0=True) is SF_UE8M0 and sf_format(mx=True) is SF_MXFP8
    for fmt in SF_FORMATS:
        assert sf_format(**fmt.kw) is fmt
    with pytest.raises(RuntimeError, match='exclude each other'):
        sf_format(ue8m0=True, mx=True)
    with pytest.raises(RuntimeError, match='dispatch_pack_cast'):
        sf_format(True, True, 'dispatch_pack_cast')


def test_lookup_from_a_scale_factor_dtype():
    assert torch.uint8 in MX_SF_DTYPES
    for dtype in MX_SF_DTYPES:
        assert sf_format_of(dtype) is SF_MXFP8
    assert sf_format_of(torch.int32) is SF_UE8M0 and sf_format_of(torch.float32) is SF_FP32
    for fmt in SF_FORMATS:
        assert sf_format_of(fmt.dtype) is fmt
    for dtype in (torch.int64, torch.float16, torch.bfloat16, torch.int8, torch.float8_e4m3fn):
        assert sf_format_of(dtype) is None
