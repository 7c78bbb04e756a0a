"""swiglu_cast_to_mx without a GPU: the argument checks that raise before any kernel runs, and the public names."""
import pytest
import torch


def _h(N=128, I=128, dtype=torch.bfloat16):
    return torch.zeros((N, 2 * I), dtype=dtype)


@pytest.mark.parametrize('h,fmt,kw,word', [
    (_h(I=192), 'fp8', {}, 'I % 128'),
    (torch.zeros((128, 129), dtype=torch.bfloat16), 'fp8', {}, 'I % 128'),
    (_h(N=130), 'fp4', dict(with_transposed=True), 'multiple of 128'),
    (_h(dtype=torch.float16), 'fp6', {}, 'bfloat16'),
    (_h(), 'fp5', {}, 'fmt'),
    (_h(), 8, {}, 'fmt'),
    (_h(), 'fp8', dict(expert_ends=torch.zeros(2, dtype=torch.int64)), 'expert_ends'),
    (_h(), 'fp8', dict(expert_ends=torch.zeros(2, dtype=torch.int32), expert_alignment=64, with_transposed=True),
     'expert_alignment'),
    (_h(), 'fp8', {}, 'on the GPU'),
])
def test_bad_arguments_raise_before_any_kernel(h, fmt, kw, word):
    import deepep_amd
    with pytest.raises(RuntimeError, match='Assertion failed: swiglu_cast_to_mx .*' + word):
        deepep_amd.swiglu_cast_to_mx(h, fmt, **kw)


def test_the_public_names():
    import deep_ep
    import deepep_amd
    from deepep_amd import _lib, kernels
    assert deep_ep.swiglu_cast_to_mx is deepep_amd.swiglu_cast_to_mx
    assert 'swiglu_cast_to_mx' in deepep_amd.__all__
    assert 'deepep_swiglu_cast_mx' in _lib.SIGNATURES and issubclass(kernels.HipKernels, kernels.SwigluCastKernels)
    assert any(s.endswith('swiglu_cast.hip') for s in _lib.SOURCES) and 'swiglu_cast.hip' in _lib.SOURCE_FLAGS
