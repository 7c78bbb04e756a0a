"""combine(use_logfmt=True) over the window transport, without a GPU: the additive C entry
deepep_combine_reduce_scatter_logfmt (declared, bound and exported with deepep_combine_reduce_scatter's arguments), its
refusals before any launch, and the keyword that routes HipKernels.combine_reduce_scatter to it without a new public
wrapper."""
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'deepep_combine_reduce_scatter_logfmt'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_the_entry_is_additive(lib):
    from deepep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    assert hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES and f'int {ENTRY}(' in header
    assert 'internode_ll.cu:557-638' in header[header.index('deepep_combine_reduce_scatter storing LogFMT'):
                                               header.index(f'int {ENTRY}(')]
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES['deepep_combine_reduce_scatter']
    assert len(_lib.SIGNATURES[ENTRY][1]) == 22
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    assert '#define DEEPEP_AMD_ABI_VERSION 14' in header


def test_the_entry_refuses_bad_arguments_with_a_message(lib):
    fn = getattr(lib, ENTRY)
    H = 512
    coded = H * 5 // 4 + H // 32                                            # 656
    # 16-byte aligned fake pointers: nothing is dereferenced, every refusal comes before a launch
    good = dict(weighted=0, src=4096, num_src_rows=8, src_row_stride=H, table=None, table_stride=0, table_width=1,
                row_weights=None, out_rows=8192, num_units=8, hidden=H, wtable=None, wtable_stride=0, wsrc=12288,
                num_weights=8, weights_offset=768, weights_pad=32, window_bases=16384, num_windows=2,
                window_bytes=1 << 20, error_flag=None, stream=None)

    def refused(text, **kw):
        args = list(dict(good, **kw).values())
        assert fn(*args) == -1 and text in lib.deepep_amd_last_error(), (kw, lib.deepep_amd_last_error())

    refused(b'multiple of 128', hidden=192, src_row_stride=192)
    refused(b'multiple of 128', hidden=0)
    refused(b'out_rows', out_rows=None)
    refused(b'windows', window_bases=None)
    refused(b'windows', num_windows=0)
    refused(b'unaligned src', src=4100)
    refused(b'row stride', src_row_stride=H - 8)
    refused(b'row stride', src_row_stride=H + 4)
    refused(b'weights_offset', weights_offset=coded - 16)                   # below the coded bytes
    refused(b'weights_offset', weights_offset=coded + 8)                    # past them, not 16-byte aligned
    refused(b'row weights', weighted=1)
    refused(b'table width', table=20480, table_width=33, table_stride=33)
    # the window must hold one wire row: max(coded, weights_offset + 4 * weights_pad) = 896 bytes
    refused(b'896 bytes', window_bytes=895)
    refused(b'656 bytes', window_bytes=655, num_weights=0, wsrc=None)       # without weights: the coded bytes
    assert fn(*dict(good, num_units=0, src=None, out_rows=None, window_bases=None).values()) == 0


def test_the_wrapper_takes_a_keyword_and_no_public_method_is_new():
    from deepep_amd.kernels import Fp4Kernels, HipKernels, LogfmtKernels
    p = inspect.signature(HipKernels.combine_reduce_scatter).parameters['dst_logfmt']
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(HipKernels._combine_reduce_scatter_logfmt)
    public = lambda cls: sorted(n for n, v in vars(cls).items() if callable(v) and not n.startswith('_'))
    assert public(LogfmtKernels) == ['cast_back_logfmt', 'cast_logfmt', 'logfmt_pack_rows']
    assert public(Fp4Kernels) == ['cast_back_fp4', 'cast_fp4', 'dispatch_copy_cast_fp4', 'dispatch_pack_cast_fp4']
    assert not [n for n in public(HipKernels) if 'scatter_logfmt' in n]


def test_a_logfmt_row_fits_the_window_of_the_bf16_combine():
    """logfmt_row_layout's rows are the smaller ones with the same weight tail, so a LogFMT combine runs in the window
    the bf16 combine sized."""
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    for H, K in ((7168, 8), (384, 3), (128, 1)):
        for single in (False, True):
            lf, pk = logfmt_row_layout(H, K, True, single), packed_row_layout(H, K, True, single)
            assert lf[0] <= pk[0] and lf[1] % 128 == 0 and lf[1] >= H * 5 // 4 + H // 32 and lf[2] == pk[2]
    assert logfmt_row_layout(7168, 8)[0] == 9344 and packed_row_layout(7168, 8)[0] == 14464
