"""The table of MX element formats (deepep_amd.kernels.MxFormat) without a GPU: it holds the three formats with the
instruction's numbers and the documented row shapes, every family of C entries exists for every format, and the lookup
from a code dtype and a row's bytes resolves as the grouped GEMMs' format inference always has."""
import pytest
import torch

from deepep_amd import _lib
from deepep_amd.kernels import FP4_ROW_DTYPES, MX_FORMATS, MXFP4, MXFP6, MXFP8, RowLayout, mx_format_of

FP4X2 = getattr(torch, 'float4_e2m1fn_x2', None)
# the C entries of a format, family by family; the row-wise FP8 entries carry the format in `_fp8_mx` or in `_mx` alone
FAMILIES = ('cast_{}_mx', 'cast_back_{}_mx', 'dispatch_pack_cast_{}_mx', 'dispatch_copy_cast_{}_mx',
            'cast_{}_mx_transposed', 'requant_{}_mx_transposed')
FP8_NAMES = {'dispatch_pack_cast_{}_mx': 'dispatch_pack_cast_mx', 'dispatch_copy_cast_{}_mx': 'dispatch_copy_cast_mx'}


def test_the_table_holds_the_three_formats():
    assert MX_FORMATS == (MXFP8, MXFP6, MXFP4)
    assert [m.name for m in MX_FORMATS] == ['fp8', 'fp6', 'fp4']
    assert [m.number for m in MX_FORMATS] == [0, 2, 4] == [_lib.MX_FP8, _lib.MX_FP6, _lib.MX_FP4]
    assert [m.block_bytes for m in MX_FORMATS] == [32, 24, 16]
    assert [m.row_dtypes for m in MX_FORMATS] == [(torch.float8_e4m3fn,), (torch.uint8,), FP4_ROW_DTYPES]
    assert [m.out_dtype for m in MX_FORMATS] == [torch.float8_e4m3fn, torch.uint8, torch.uint8]
    assert [m.row_what for m in MX_FORMATS] == ['H', '3 * H / 4', 'H / 2']
    assert [m.row_words('N') for m in MX_FORMATS] == ['N', '3 * N / 4', 'N / 2']
    assert torch.uint8 in FP4_ROW_DTYPES and all(m.out_dtype in m.row_dtypes for m in MX_FORMATS)


@pytest.mark.parametrize('H', [128, 640, 7168])
def test_row_bytes_are_the_documented_ones(H):
    assert [m.row_bytes(H) for m in MX_FORMATS] == [H, 3 * H // 4, H // 2]
    for m in MX_FORMATS:
        assert m.elems(m.row_bytes(H)) == H
        # the packed row of a casting dispatch: what ElasticBuffer._dispatch builds for the format
        assert RowLayout.make(m.row_bytes(H), H // 32, 8).x_bytes == m.row_bytes(H)
    # a row that is no whole number of 128 elements never comes back as a multiple of 128
    for m in MX_FORMATS:
        for extra in range(1, m.row_bytes(128)):
            assert m.elems(m.row_bytes(H) + extra) % 128 != 0, (m.name, extra)


@pytest.mark.parametrize('mx', MX_FORMATS, ids=lambda m: m.name)
def test_every_family_has_the_formats_entry(mx):
    for family in FAMILIES:
        name = FP8_NAMES.get(family, family.format('fp8')) if mx is MXFP8 else family.format(mx.name)
        assert 'deepep_' + name in _lib.SIGNATURES, (mx.name, family)
    if mx is not MXFP8:
        # the FP4 / FP6 entries of a family take the same arguments
        for family in FAMILIES:
            assert _lib.SIGNATURES['deepep_' + family.format(mx.name)] == _lib.SIGNATURES['deepep_' + family.format('fp4')]


def test_lookup_from_a_code_dtype_and_a_rows_bytes():
    """C = 128 elements (four scale factors): the nine (dtype, row bytes) cases, written out."""
    cases = [(torch.float8_e4m3fn, 128, MXFP8), (torch.float8_e4m3fn, 96, None), (torch.float8_e4m3fn, 64, None),
             (torch.uint8, 128, None), (torch.uint8, 96, MXFP6), (torch.uint8, 64, MXFP4)]
    if FP4X2 is not None:
        cases += [(FP4X2, 128, None), (FP4X2, 96, None), (FP4X2, 64, MXFP4)]
    for dtype, row, want in cases:
        assert mx_format_of(dtype, row, 128) is want, (dtype, row)
    # other lengths: a row's bytes against 32 * the scale factors, not against each other
    assert mx_format_of(torch.uint8, 96, 192) is MXFP4 and mx_format_of(torch.uint8, 96, 96) is None
    assert mx_format_of(torch.uint8, 3584, 7168) is MXFP4 and mx_format_of(torch.uint8, 5376, 7168) is MXFP6
    assert mx_format_of(torch.float8_e4m3fn, 7168, 7168) is MXFP8


def test_lookup_of_ambiguous_and_impossible_rows():
    # an empty row with no scale factors fits FP4 and FP6 alike: FP4 is asked first, as it always was
    assert mx_format_of(torch.uint8, 0, 0) is MXFP4 and mx_format_of(torch.float8_e4m3fn, 0, 0) is MXFP8
    if FP4X2 is not None:
        assert mx_format_of(FP4X2, 0, 0) is MXFP4
    for dtype in (torch.int8, torch.bfloat16, torch.float16, torch.int32, torch.float8_e5m2):
        for row in (0, 64, 96, 128):
            assert mx_format_of(dtype, row, 128 if row else 0) is None, (dtype, row)
    for row in (0, 63, 65, 95, 97, 127, 129, 256):
        assert mx_format_of(torch.uint8, row, 128) is None, row


def test_the_grouped_gemms_infer_the_format_through_the_table():
    """_mx_operand on CPU tensors (it launches nothing): the format's number for each of the three, and the message
    that names the three row shapes."""
    from deepep_amd import _mx_operand
    sf = torch.zeros((4, 4), dtype=torch.uint8)
    for mx in MX_FORMATS:
        q = torch.zeros((4, mx.row_bytes(128)), dtype=mx.out_dtype)
        assert _mx_operand('test', 'a', (q, sf), 1)[2:] == (mx.number, (4,), 128)
    fp4 = 'uint8 / float4_e2m1fn_x2' if FP4X2 is not None else 'uint8'
    with pytest.raises(RuntimeError, match=rf'float8_e4m3fn \[128\], {fp4} \[64\] or uint8 \[96\], '
                                           r'not torch.uint8 \[128\]'):
        _mx_operand('test', 'a', (torch.zeros((4, 128), dtype=torch.uint8), sf), 1)
