"""The four writers of the MXFP6 path -- cast_fp6 (both store widths), cast_back_fp6, dispatch_pack_cast_fp6 and
dispatch_copy_cast_fp6 -- under the guard (tests/guard.py): canary bands around every output their wrappers declare, at
the shapes at which each store pattern has a tail (one quad; a row whose last lane pair ends the row; a pass and a
quad; passes and a part; row counts that end inside a workgroup of four rows; the copy's chunk of 4096 columns and a
part).

The declarations of the four wrappers are made here, for the duration of a test: they are methods of
deepep_amd.kernels.Fp6Kernels, the base class of HipKernels that only a dispatch(cast_to_fp6=True) and the package's
per_token_cast_*_fp6 reach, and tests/guard.py's table lists the wrappers HipKernels itself defines."""
import pytest
import torch

from tests import guard as guard_module
from tests.fp6_ref import FP6, fp6_back_ref, fp6_pair
from tests.guard import Guard

pytestmark = pytest.mark.gpu

FP6_OUTPUTS = {'cast_fp6': ('q', 'sf'), 'cast_back_fp6': ('out',),
               'dispatch_pack_cast_fp6': ('packed', 'error_flag'),
               'dispatch_copy_cast_fp6': ('recv_x_bytes', 'recv_sf_bytes', 'recv_w', 'error_flag')}


@pytest.fixture
def guard(monkeypatch):
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    for name, outs in FP6_OUTPUTS.items():
        monkeypatch.setitem(guard_module.OUTPUTS, name, outs)
    return Guard(HipKernels())


def _clean(guard, at_least):
    assert guard.guarded_calls >= at_least, f'{guard.guarded_calls} guarded calls'
    assert guard.verify() >= at_least


def test_the_declared_outputs_are_parameters_of_the_wrappers():
    import inspect
    from deepep_amd.kernels import Fp6Kernels, HipKernels
    for name, outs in FP6_OUTPUTS.items():
        assert name in vars(Fp6Kernels) and set(outs) <= set(inspect.signature(getattr(HipKernels, name)).parameters)
    public = sorted(n for n, v in vars(Fp6Kernels).items() if callable(v) and not n.startswith('_'))
    assert public == sorted(FP6_OUTPUTS)                        # every FP6 wrapper that writes is declared here


@pytest.mark.parametrize('rows', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 1152, 2176, 7168])   # 1152: 36 groups, the last lane pair ends the row
def test_codec_kernels(guard, H, rows):
    from tests.test_fp6_gpu import _cast_input
    x_cpu = _cast_input(rows, H)
    x = x_cpu.cuda()
    wide = torch.zeros((rows, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x
    q_ref, sf_ref = fp6_pair(x_cpu)
    back_ref = fp6_back_ref(q_ref, sf_ref)
    for xin in (x, wide[:, :H]):
        for store_bytes in (None, 8, 16):
            q = torch.empty((rows, 3 * H // 4), dtype=torch.uint8, device='cuda')
            sf = torch.empty((rows, H // 32), dtype=torch.uint8, device='cuda')
            guard.cast_fp6(xin, q, sf, store_bytes=store_bytes)
            assert torch.equal(q.cpu(), q_ref) and torch.equal(sf.cpu(), sf_ref), store_bytes
        out = torch.empty((rows, H), dtype=torch.bfloat16, device='cuda')
        guard.cast_back_fp6(q, sf, out)
        assert torch.equal(out.cpu().view(torch.int16), back_ref.view(torch.int16))
    _clean(guard, 8)


@pytest.mark.parametrize('T,H,K', [(33, 256, 4), (70, 1152, 2)])
def test_pack_into_a_local_buffer(guard, T, H, K):
    from tests.test_fp6_gpu import test_pack_cast_fp6_equals_pack_of_the_reference_pair as case
    case(guard, T, H, K, False)
    _clean(guard, 2)


@pytest.mark.parametrize('weights', [True, False])
@pytest.mark.parametrize('K,E', [(3, 8), (8, 16)])
def test_one_rank_dispatch_copies(guard, K, E, weights):
    """The reduced and the expanded casting copy (H = 5248: a chunk of codes and a part of the next whose last lane
    pair ends the row)."""
    from tests.test_cast_keyword_gpu import _group1
    from tests.test_mx_gpu import _buffer, _mx_inputs
    from tests.ue8m0_ref import packed_differences
    T, H = 33, 5248
    buf = _buffer(_group1(), T, H, K, kernels=guard)
    x, idx, w = _mx_inputs(5 + K, T, H, K, E)
    w = w if weights else None
    for more in (dict(), dict(do_expand=True), dict(do_expand=True, expert_alignment=16, do_zero_padding=True)):
        got = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, **more, **FP6)
        want = buf.dispatch(fp6_pair(x), topk_idx=idx, topk_weights=w, num_experts=E, **more)
        assert not packed_differences(got, want), more
    assert guard.verify() > 0
    assert buf.kernels.names().count('dispatch_copy_cast_fp6') == 3
