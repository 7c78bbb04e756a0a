"""route_topk without a GPU: the argument checks that raise before any kernel runs, and the public names."""
import pytest
import torch


def _x(T=4, E=64, dtype=torch.float32):
    return torch.zeros((T, E), dtype=dtype)


@pytest.mark.parametrize('logits,K,kw,word', [
    (_x(dtype=torch.float16), 4, {}, 'float32 or bfloat16'),
    (torch.zeros(64), 4, {}, '2-D'),
    (_x(E=4), 2, {}, 'E % 8'),
    (_x(E=1032), 2, {}, 'E <= 1024'),
    (_x(E=60), 2, {}, 'E % 8'),
    (_x(), 4, dict(score_func='tanh'), 'score_func'),
    (_x(), 4, dict(group_score='sum'), 'group_score'),
    (_x(), 4, dict(num_groups=3), 'E % num_groups'),
    (_x(E=1024), 4, dict(num_groups=128), 'num_groups <= 64'),
    (_x(), 4, dict(num_groups=8, num_topk_groups=9), 'num_topk_groups <= num_groups'),
    (_x(), 4, dict(num_groups=8, num_topk_groups=0), 'num_topk_groups'),
    (_x(), 4, dict(num_groups=64, num_topk_groups=8), 'at least 2 experts a group'),
    (_x(), 0, {}, 'num_topk <= 64'),
    (_x(E=128), 65, {}, 'num_topk <= 64'),
    (_x(), 17, dict(num_groups=8, num_topk_groups=2), 'num_topk_groups \\* E'),
    (torch.zeros((4, 128))[:, ::2], 4, {}, 'unit column stride'),
    (torch.zeros((4, 66))[:, :64], 4, {}, '16 bytes'),
    (_x(), 4, dict(bias=torch.zeros(64, dtype=torch.float64)), 'bias'),
    (_x(), 4, dict(bias=torch.zeros(32)), 'bias'),
    (_x(), 4, {}, 'on the GPU'),
])
def test_bad_arguments_raise_before_any_kernel(logits, K, kw, word):
    import deepep_amd
    with pytest.raises(RuntimeError, match='Assertion failed: route_topk .*' + word):
        deepep_amd.route_topk(logits, K, **kw)


def test_the_public_names():
    import __graft_entry__ as entry
    import deep_ep
    import deepep_amd
    from deepep_amd import _lib, kernels
    assert deep_ep.route_topk is deepep_amd.route_topk and 'route_topk' in deepep_amd.__all__
    assert 'deepep_route_topk' in _lib.SIGNATURES and issubclass(kernels.HipKernels, kernels.RouterKernels)
    assert 'route_topk' not in vars(kernels.HipKernels)
    assert all(any(s.endswith('router.hip') for s in srcs) for srcs in (_lib.SOURCES, entry.HIP_SOURCES))
