"""The FP8 cast without a GPU: the C-ABI entry points' rejections (deepep_cast_fp8,
deepep_dispatch_pack_cast), the public function's argument checks, and the torch restatement the GPU tests
compare with (the default mode is workloads.per_token_cast_to_fp8, the reference's
deep_ep/utils/math.py:30-39; round_scale restates calculate_fp8_scales(round_scale=true),
csrc/kernels/legacy/utils.cuh:494-503)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from workloads import per_token_cast_to_fp8  # noqa: E402


def cast_ref(x: torch.Tensor, round_scale: bool = False):
    """(q float8_e4m3fn [T, H], sf float32 [T, H / 128]) of a bf16 x on the CPU, H % 128 == 0."""
    assert x.device.type == 'cpu' and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0
    m, n = x.shape
    if m == 0:
        return torch.empty((0, n), dtype=torch.float8_e4m3fn), torch.empty((0, n // 128), dtype=torch.float32)
    if not round_scale:
        return per_token_cast_to_fp8(x)
    view = x.view(m, -1, 128)
    amax = view.abs().float().amax(dim=2).clamp(1e-4)
    bits = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    sf = ((e + 127) << 23).view(torch.float32)
    scale = ((127 - e) << 23).view(torch.float32)
    q = (view.float() * scale.unsqueeze(2)).to(torch.float8_e4m3fn).view(m, n).contiguous()
    return q, sf.contiguous()


def test_round_scale_restatement_is_a_power_of_two_cover():
    """The restatement itself: sf is a power of two, amax / 448 <= sf < 2 * amax / 448 (so nothing
    saturates), and dequantising is within one e4m3 step of the input."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((9, 384), generator=g) * 3).to(torch.bfloat16)
    x[0, :128] = 0
    q, sf = cast_ref(x, True)
    amax = x.view(9, 3, 128).abs().float().amax(dim=2).clamp(1e-4)
    assert torch.equal(sf.view(torch.int32) & 0x7fffff, torch.zeros((9, 3), dtype=torch.int32))
    lo = amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)
    assert bool((sf >= lo).all()) and bool((sf < 2 * lo).all())
    back = q.float().view(9, 3, 128) * sf.unsqueeze(2)
    assert bool(((back - x.float().view(9, 3, 128)).abs() <= sf.unsqueeze(2) * 16).all())   # half a step at 448: 16
    assert not bool(q.float().isnan().any())


def test_public_cast_rejects_bad_inputs_without_a_gpu():
    """deepep_amd.per_token_cast_to_fp8 checks its input before it touches the library or the GPU."""
    import deepep_amd
    assert 'per_token_cast_to_fp8' in deepep_amd.__all__
    for bad in (torch.zeros((4, 128)), torch.zeros((4, 192), dtype=torch.bfloat16),
                torch.zeros((128,), dtype=torch.bfloat16),
                (torch.zeros((4, 128), dtype=torch.float8_e4m3fn), torch.zeros((4, 1)))):
        with pytest.raises(RuntimeError, match='Assertion failed'):
            deepep_amd.per_token_cast_to_fp8(bad)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from deepep_amd import _lib
    return _lib.load()


def test_entry_points_are_exported_and_reject_bad_arguments_without_a_gpu(lib):
    """16-byte aligned fake pointers: nothing is dereferenced, every rejection comes before a launch."""
    from deepep_amd import _lib
    assert hasattr(lib, 'deepep_cast_fp8') and hasattr(lib, 'deepep_dispatch_pack_cast')
    assert 'deepep_cast_fp8' in _lib.SIGNATURES and 'deepep_dispatch_pack_cast' in _lib.SIGNATURES
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    assert 'int deepep_cast_fp8(' in header and 'int deepep_dispatch_pack_cast(' in header
    cast = lib.deepep_cast_fp8
    # (x, row stride, rows, hidden, round_scale, q, sf, stream)
    assert cast(16, 384, 4, 192, 0, 32, 64, None) == -1 and b'128' in lib.deepep_amd_last_error()   # hidden % 128
    assert cast(16, 256, 4, 0, 0, 32, 64, None) == -1
    assert cast(None, 256, 4, 128, 0, 32, 64, None) == -1 and b'pointers' in lib.deepep_amd_last_error()
    assert cast(16, 256, 4, 128, 0, None, 64, None) == -1
    assert cast(16, 256, 4, 128, 0, 32, None, None) == -1
    assert cast(24, 256, 4, 128, 0, 32, 64, None) == -1                  # x not 16-byte aligned
    assert cast(16, 256, 4, 128, 0, 40, 64, None) == -1                  # q not 16-byte aligned
    assert cast(16, 256, 4, 128, 0, 32, 66, None) == -1                  # sf not 4-byte aligned
    assert cast(16, 240, 4, 128, 0, 32, 64, None) == -1 and b'stride' in lib.deepep_amd_last_error()   # < hidden * 2
    assert cast(16, 264, 4, 128, 0, 32, 64, None) == -1                  # stride not 16-byte aligned
    assert cast(16, 256, -1, 128, 0, 32, 64, None) == -1
    assert cast(None, 0, 0, 128, 0, None, None, None) == 0               # no rows: nothing to do
    pack = lib.deepep_dispatch_pack_cast
    # RowLayout.make(128, 4, 2): sf 128, idx 144, weights 160, src 176, row 256
    good = dict(x=16, stride=256, hidden=128, rs=0, idx=32, w=None, T=4, K=2, base=0, slot=48, off=64, R=2, packed=80,
                bases=None, row=256, rows=8, sf_off=128, idx_off=144, w_off=160, src_off=176, flag=None, stream=None)

    def call(**kw):
        return pack(*dict(good, **kw).values())

    assert call(hidden=192, stride=384) == -1 and b'128' in lib.deepep_amd_last_error()
    assert call(x=None) == -1
    assert call(x=24) == -1
    assert call(stride=240) == -1 and b'stride' in lib.deepep_amd_last_error()
    assert call(stride=264) == -1
    assert call(packed=None) == -1
    assert call(packed=88) == -1
    assert call(rows=-1) == -1
    assert call(sf_off=64) == -1                                         # scale factors over the fp8 bytes
    assert call(idx_off=128) == -1                                       # indices over the scale factors
    assert call(row=176) == -1                                           # row ends before its last field
    assert call(K=33) == -1
    assert call(R=65) == -1
    assert call(T=0) == 0                                                # no tokens: nothing to do
