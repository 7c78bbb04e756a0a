"""grouped_gemm_mx / grouped_gemm_mx_wgrad without a GPU: every argument check raises its RuntimeError before the
library is loaded, the format inference included; and the names reach every layer."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, E4M3 = torch.uint8, torch.float8_e4m3fn


@pytest.fixture
def no_library(monkeypatch):
    from deepep_amd import _lib
    monkeypatch.setattr(_lib, 'load', lambda *a, **k: pytest.fail('the library was loaded'))


def pair(lead, C, fmt='fp8', dtype=None, sf_dtype=U8):
    row = {'fp8': C, 'fp4': C // 2, 'fp6': C * 3 // 4}[fmt]
    return (torch.zeros((*lead, row), dtype=dtype or (E4M3 if fmt == 'fp8' else U8)),
            torch.zeros((*lead, C // 32), dtype=sf_dtype))


ENDS = torch.zeros(2, dtype=torch.int32)
A, B = pair((256,), 256), pair((2, 128), 256)
FPROP_CASES = {
    'not a pair': (A[0], B, ENDS, {}),
    'sf dtype': (pair((256,), 256, sf_dtype=torch.int32), B, ENDS, {}),
    'b is 2-D': (A, pair((256,), 256), ENDS, {}),
    'row bytes of no format': ((torch.zeros((256, 100), dtype=U8), A[1]), B, ENDS, {}),
    'K % 128': (pair((256,), 160), pair((2, 128), 160), ENDS, {}),
    'K differs': (A, pair((2, 128), 384), ENDS, {}),
    'N % 128': (pair((200,), 256), B, ENDS, {}),
    'O % 128': (A, pair((2, 64), 256), ENDS, {}),
    'out dtype': (A, B, ENDS, dict(out_dtype=torch.float16)),
    'ends dtype': (A, B, ENDS.long(), {}),
    'alignment': (A, B, ENDS, dict(expert_alignment=64)),
    'b not contiguous': (A, tuple(t.transpose(0, 1).contiguous().transpose(0, 1) for t in B), ENDS, {}),
    'a column stride': ((torch.zeros((256, 512), dtype=E4M3)[:, ::2], A[1]), B, ENDS, {}),
    'not on the GPU': (A, B, ENDS, {}),
}


DY, X = pair((128,), 256, 'fp4'), pair((256,), 256, 'fp6')
WGRAD_CASES = {
    'N differs': (DY, pair((256,), 384, 'fp6'), ENDS, {}),
    'not on the GPU': (DY, X, ENDS, {}),
}


CASES = [('grouped_gemm_mx', k, v) for k, v in FPROP_CASES.items()] + \
        [('grouped_gemm_mx_wgrad', k, v) for k, v in WGRAD_CASES.items()]


@pytest.mark.parametrize('name,case,args', CASES, ids=[f'{n}-{c}' for n, c, _ in CASES])
def test_argument_checks_raise_before_the_library(no_library, name, case, args):
    import deepep_amd
    x, y, ends, kw = args
    with pytest.raises(RuntimeError, match=f'^Assertion failed: {name} '):
        getattr(deepep_amd, name)(x, y, ends, **kw)


def test_no_tokens_need_no_library(no_library, monkeypatch):
    import deepep_amd
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    out = deepep_amd.grouped_gemm_mx(pair((0,), 256, 'fp6'), B, ENDS, out_dtype=torch.float32)
    assert tuple(out.shape) == (0, 128) and out.dtype == torch.float32
    dw = deepep_amd.grouped_gemm_mx_wgrad(pair((128,), 0), pair((256,), 0, 'fp4'), ENDS)
    assert tuple(dw.shape) == (2, 128, 256) and dw.dtype == torch.float32 and not dw.any()


def test_the_names_reach_every_layer():
    import __graft_entry__ as entry
    import deep_ep
    import deepep_amd
    from deepep_amd import _lib
    from deepep_amd.kernels import GroupedGemmMxKernels, HipKernels
    for name in ('grouped_gemm_mx', 'grouped_gemm_mx_wgrad'):
        assert name in deepep_amd.__all__ and getattr(deep_ep, name) is getattr(deepep_amd, name)
    assert 'grouped_gemm_mx' in vars(GroupedGemmMxKernels) and issubclass(HipKernels, GroupedGemmMxKernels)
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    decl = re.search(r'\nint deepep_grouped_gemm_mx\(([^;]*)\);', header)
    assert decl and len(decl.group(1).split(',')) == len(_lib.SIGNATURES['deepep_grouped_gemm_mx'][1]) == 20
    for word in ('MX_FP8', 'MX_FP6', 'MX_FP4', 'GEMM_FPROP', 'GEMM_WGRAD'):
        assert re.search(r'#define DEEPEP_%s +%d\b' % (word, getattr(_lib, word)), header)
    assert _lib.ABI_VERSION == 14                                # additive
    assert all(any(s.endswith('grouped_gemm_mx.hip') for s in srcs) for srcs in (entry.HIP_SOURCES, _lib.SOURCES))
    assert 'deepep_grouped_gemm_mx' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
