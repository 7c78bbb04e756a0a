"""deepep_dispatch_copy_cast (the one-rank dispatch copy with the FP8 cast on the way) without a GPU: the
entry point is exported, declared and prototyped, and it and its wrapper (HipKernels.dispatch_copy_cast) reject
bad arguments before anything is launched."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_copy_cast_entry_is_exported_and_rejects_bad_arguments_without_a_gpu(lib):
    """16-byte aligned fake pointers: nothing is dereferenced, every rejection comes before a launch."""
    from deepep_amd import _lib
    assert hasattr(lib, 'deepep_dispatch_copy_cast') and 'deepep_dispatch_copy_cast' in _lib.SIGNATURES
    assert 'int deepep_dispatch_copy_cast(' in open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    assert lib.deepep_amd_abi_version() == _lib.ABI_VERSION == 14          # additive: the version stays
    good = dict(packed=16, row=128, w_off=32, N=4, K=2, meta=32, expanded=0, x=48, stride=256, hidden=128, rs=0,
                t_max=4, recv_x=64, recv_sf=80, recv_w=96, out_rows=4, inv=None, offsets=None, end=None, epr=0,
                row_map=None, flag=None, stream=None)

    def call(**kw):
        return lib.deepep_dispatch_copy_cast(*dict(good, **kw).values())

    assert call(hidden=192, stride=384) == -1 and b'128' in lib.deepep_amd_last_error()
    assert call(hidden=0) == -1
    assert call(x=None) == -1 and b'x null' in lib.deepep_amd_last_error()
    assert call(x=56) == -1                                                # x not 16-byte aligned
    assert call(stride=240) == -1 and b'stride' in lib.deepep_amd_last_error()
    assert call(stride=264) == -1                                          # stride not 16-byte aligned
    assert call(recv_x=None) == -1 and call(recv_x=72) == -1
    assert call(recv_sf=None) == -1 and call(recv_sf=82) == -1             # the scale factors are required
    assert call(meta=None) == -1 and call(t_max=0) == -1 and call(K=33) == -1 and call(out_rows=-1) == -1
    assert call(packed=None) == -1                                         # weights come from the packed rows
    assert call(w_off=126) == -1 and call(w_off=124) == -1                 # weights misaligned / past the row
    assert call(inv=112) == -1                                             # blocked tables: expanded only ...
    assert call(inv=112, expanded=1) == -1                                 # ... and all three of them
    assert call(N=-1) == -1
    assert call(N=0, x=None, recv_x=None, recv_sf=None) == 0               # no rows: nothing to do


def test_copy_cast_wrapper_checks_its_arguments_on_the_host(lib):
    """Every check of HipKernels.dispatch_copy_cast comes before the library call: CPU tensors suffice."""
    from deepep_amd.kernels import HipKernels, RowLayout
    kern = HipKernels()
    T, H, K = 4, 128, 2
    layout = RowLayout.make(0, 0, K)
    packed = torch.zeros((T, layout.row_bytes), dtype=torch.uint8)
    meta = torch.full((T, K + 2), -1, dtype=torch.int32)
    good = dict(recv_x_bytes=torch.zeros((T, H), dtype=torch.uint8),
                recv_sf_bytes=torch.zeros((T, H // 128 * 4), dtype=torch.uint8),
                recv_w=torch.zeros((T, K)), x_direct=torch.zeros((T, 2 * H), dtype=torch.uint8), num_max_tokens=T)

    def call(**kw):
        # num_recv = 0: should a check not fire, the entry point returns before it launches anything
        kern.dispatch_copy_cast(packed, layout, 0, meta, False, **dict(good, **kw))

    for match, kw in (('x_direct', dict(x_direct=None)),
                      ('sf_direct', dict(sf_direct=torch.zeros((T, 4), dtype=torch.uint8))),
                      ('bf16', dict(x_direct=torch.zeros((T, H), dtype=torch.bfloat16))),       # not the byte view
                      ('128', dict(x_direct=torch.zeros((T, 384), dtype=torch.uint8))),         # hidden = 192
                      ('unit column stride', dict(x_direct=torch.zeros((2 * H, T), dtype=torch.uint8).t())),
                      ('outputs', dict(recv_sf_bytes=None)),
                      ('outputs', dict(recv_x_bytes=torch.zeros((T, 2 * H), dtype=torch.uint8))),
                      ('outputs', dict(recv_sf_bytes=torch.zeros((T + 1, H // 128 * 4), dtype=torch.uint8))),
                      ('blocked copy tables', dict(inv=torch.zeros((T,), dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
