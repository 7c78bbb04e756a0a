"""The four writers of the MXFP4 path -- cast_fp4, cast_back_fp4, dispatch_pack_cast_fp4 and dispatch_copy_cast_fp4 --
under the guard (tests/guard.py): canary bands around every output their wrappers declare, at the shapes at which each
store pattern has a tail (one dword of exponent bytes, a part of a pass, passes and a part; row counts that end inside
a workgroup of four rows; the copy's chunk of 4096 columns and a part).

The declarations of the four wrappers are made here, for the duration of a test: they are methods of
deepep_amd.kernels.Fp4Kernels, the base class of HipKernels that only a dispatch(cast_to_fp4=True) and the package's
per_token_cast_*_fp4 reach, and tests/guard.py's table lists the wrappers HipKernels itself defines."""
import pytest
import torch

from tests import guard as guard_module
from tests.fp4_ref import FP4, fp4_back_ref, fp4_pair
from tests.guard import Guard

pytestmark = pytest.mark.gpu

FP4_OUTPUTS = {'cast_fp4': ('q', 'sf'), 'cast_back_fp4': ('out',),
               'dispatch_pack_cast_fp4': ('packed', 'error_flag'),
               'dispatch_copy_cast_fp4': ('recv_x_bytes', 'recv_sf_bytes', 'recv_w', 'error_flag')}


@pytest.fixture
def guard(monkeypatch):
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    for name, outs in FP4_OUTPUTS.items():
        monkeypatch.setitem(guard_module.OUTPUTS, name, outs)
    return Guard(HipKernels())


def _clean(guard, at_least):
    assert guard.guarded_calls >= at_least, f'{guard.guarded_calls} guarded calls'
    assert guard.verify() >= at_least


def test_the_declared_outputs_are_parameters_of_the_wrappers():
    import inspect
    from deepep_amd.kernels import Fp4Kernels, HipKernels
    for name, outs in FP4_OUTPUTS.items():
        assert name in vars(Fp4Kernels) and set(outs) <= set(inspect.signature(getattr(HipKernels, name)).parameters)
    public = sorted(n for n, v in vars(Fp4Kernels).items() if callable(v) and not n.startswith('_'))
    assert public == sorted(FP4_OUTPUTS)                        # every FP4 wrapper that writes is declared here


@pytest.mark.parametrize('rows', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 384, 2176, 7168])
def test_codec_kernels(guard, H, rows):
    from tests.test_fp4_gpu import _cast_input
    x_cpu = _cast_input(rows, H)
    x = x_cpu.cuda()
    wide = torch.zeros((rows, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x
    q_ref, sf_ref = fp4_pair(x_cpu)
    back_ref = fp4_back_ref(q_ref, sf_ref)
    for xin in (x, wide[:, :H]):
        q = torch.empty((rows, H // 2), dtype=torch.uint8, device='cuda')
        sf = torch.empty((rows, H // 32), dtype=torch.uint8, device='cuda')
        guard.cast_fp4(xin, q, sf)
        out = torch.empty((rows, H), dtype=torch.bfloat16, device='cuda')
        guard.cast_back_fp4(q, sf, out)
        assert torch.equal(q.cpu(), q_ref) and torch.equal(sf.cpu(), sf_ref)
        assert torch.equal(out.cpu().view(torch.int16), back_ref.view(torch.int16))
    _clean(guard, 4)


@pytest.mark.parametrize('T,H,K', [(33, 256, 4), (70, 1152, 2)])
def test_pack_into_a_local_buffer(guard, T, H, K):
    from tests.test_fp4_gpu import test_pack_cast_fp4_equals_pack_of_the_reference_pair as case
    case(guard, T, H, K, False)
    _clean(guard, 2)


@pytest.mark.parametrize('weights', [True, False])
@pytest.mark.parametrize('K,E', [(3, 8), (8, 16)])
def test_one_rank_dispatch_copies(guard, K, E, weights):
    """The reduced and the expanded casting copy (H = 5120: a chunk of codes and a part of the next)."""
    from tests.test_cast_keyword_gpu import _group1
    from tests.test_mx_gpu import _buffer, _mx_inputs
    from tests.ue8m0_ref import packed_differences
    T, H = 33, 5120
    buf = _buffer(_group1(), T, H, K, kernels=guard)
    x, idx, w = _mx_inputs(5 + K, T, H, K, E)
    w = w if weights else None
    for more in (dict(), dict(do_expand=True), dict(do_expand=True, expert_alignment=16, do_zero_padding=True)):
        got = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, **more, **FP4)
        want = buf.dispatch(fp4_pair(x), topk_idx=idx, topk_weights=w, num_experts=E, **more)
        assert not packed_differences(got, want), more
    assert guard.verify() > 0
    assert buf.kernels.names().count('dispatch_copy_cast_fp4') == 3
