"""swiglu_backward_cast_to_mx without a GPU: the argument checks that raise before any kernel runs, and the public
names."""
import pytest
import torch


def _h(N=128, I=128, dtype=torch.bfloat16):
    return torch.zeros((N, 2 * I), dtype=dtype)


def _da(N=128, I=128, dtype=torch.bfloat16):
    return torch.zeros((N, I), dtype=dtype)


@pytest.mark.parametrize('h,dact,fmt,kw,word', [
    (_h(dtype=torch.float16), _da(), 'fp6', {}, 'bfloat16'),
    (_h(), _da(dtype=torch.float32), 'fp6', {}, 'bfloat16'),
    (_h(), _da(I=256), 'fp8', {}, r'\[N, I\]'),
    (_h(), _da(N=64), 'fp8', {}, r'\[N, I\]'),
    (_h(I=192), _da(I=192), 'fp8', {}, 'I % 128'),
    (_h(N=130), _da(N=130), 'fp4', dict(with_transposed=True), 'multiple of 128'),
    (_h(I=130)[:, 2:258], _da(), 'fp8', {}, 'row stride'),
    (_h(), _da(I=256)[:, ::2], 'fp8', {}, 'row stride'),
    (_h(), _da(), 'fp5', {}, 'fmt'),
    (_h(), _da(), 8, {}, 'fmt'),
    (_h(), _da(), 'fp8', dict(expert_ends=torch.zeros(2, dtype=torch.int64)), 'expert_ends'),
    (_h(), _da(), 'fp8', dict(expert_ends=torch.zeros(2, dtype=torch.int32), expert_alignment=64,
                              with_transposed=True), 'expert_alignment'),
    (_h(), _da(), 'fp8', {}, 'same GPU'),
])
def test_bad_arguments_raise_before_any_kernel(h, dact, fmt, kw, word):
    import deepep_amd
    with pytest.raises(RuntimeError, match='Assertion failed: swiglu_backward_cast_to_mx .*' + word):
        deepep_amd.swiglu_backward_cast_to_mx(h, dact, fmt, **kw)


def test_the_public_names():
    import __graft_entry__ as entry
    import deep_ep
    import deepep_amd
    from deepep_amd import _lib, kernels
    assert deep_ep.swiglu_backward_cast_to_mx is deepep_amd.swiglu_backward_cast_to_mx
    assert 'swiglu_backward_cast_to_mx' in deepep_amd.__all__
    assert 'deepep_swiglu_backward_cast_mx' in _lib.SIGNATURES
    assert hasattr(kernels.HipKernels, 'swiglu_backward_cast_mx')
    name = 'swiglu_backward_cast.hip'
    assert all(any(s.endswith(name) for s in srcs) for srcs in (_lib.SOURCES, entry.HIP_SOURCES))
    assert _lib.SOURCE_FLAGS[name] == _lib.SOURCE_FLAGS['swiglu_cast.hip']
