"""grouped_gemm_mx_decode without a GPU: every argument check raises its RuntimeError before the library is loaded, and
the name reaches every layer."""
import os
import re

import pytest
import torch

from tests.test_grouped_gemm_mx_cpu import ROOT, no_library, pair  # noqa: F401  (no_library is a fixture)

ENDS = torch.zeros(2, dtype=torch.int32)
A, B = pair((32,), 256), pair((2, 64), 256)
CASES = {
    'N % 16': (pair((24,), 256), B, ENDS, {}),
    'O % 64': (A, pair((2, 32), 256), ENDS, {}),
    'K % 128': (pair((32,), 160), pair((2, 64), 160), ENDS, {}),
    'alignment 8': (A, B, ENDS, dict(expert_alignment=8)),
    'K differs': (A, pair((2, 64), 384), ENDS, {}),
    'ends dtype': (A, B, ENDS.long(), {}),
    'out dtype': (A, B, ENDS, dict(out_dtype=torch.float16)),
    'b not contiguous': (A, tuple(t.transpose(0, 1).contiguous().transpose(0, 1) for t in B), ENDS, {}),
    'not on the GPU': (A, B, ENDS, dict(expert_alignment=128)),
}


@pytest.mark.parametrize('case', CASES)
def test_argument_checks_raise_before_the_library(no_library, case):  # noqa: F811
    import deepep_amd
    a, b, ends, kw = CASES[case]
    with pytest.raises(RuntimeError, match='^Assertion failed: grouped_gemm_mx_decode '):
        deepep_amd.grouped_gemm_mx_decode(a, b, ends, **kw)


def test_no_tokens_need_no_library(no_library, monkeypatch):  # noqa: F811
    import deepep_amd
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    out = deepep_amd.grouped_gemm_mx_decode(pair((0,), 256, 'fp6'), B, ENDS, out_dtype=torch.float32)
    assert tuple(out.shape) == (0, 64) and out.dtype == torch.float32


def test_the_name_reaches_every_layer():
    import __graft_entry__ as entry
    import deep_ep
    import deepep_amd
    from deepep_amd import _lib
    from deepep_amd.kernels import GroupedGemmMxKernels
    name = 'grouped_gemm_mx_decode'
    assert name in deepep_amd.__all__ and getattr(deep_ep, name) is getattr(deepep_amd, name)
    assert name in vars(GroupedGemmMxKernels)
    header = open(os.path.join(ROOT, 'include', 'deepep_amd.h')).read()
    decl = re.search(r'\nint deepep_grouped_gemm_mx_decode\(([^;]*)\);', header)
    assert decl and len(decl.group(1).split(',')) == len(_lib.SIGNATURES['deepep_' + name][1]) == 19
    assert _lib.ABI_VERSION == 14                                # additive
    assert all(any(s.endswith(name + '.hip') for s in srcs) for srcs in (entry.HIP_SOURCES, _lib.SOURCES))
    assert 'deepep_grouped_gemm_mx_decode' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
