"""The transposed MXFP4 and MXFP6 casts under the guard (tests/guard.py): canary bands around q_t, sf_t, q and sf, at the
shapes at which the tiling has tails (a run of tiles that ends early along the token axis: dword scale-factor stores;
more column blocks than one; whole runs: 16-byte scale-factor stores), in both forms and with strided rows.

The declaration of the wrappers is made here, for the duration of a test: they are methods of
deepep_amd.kernels.TransposedFp4Fp6Kernels, the base class of HipKernels that only the package's
cast_to_mxfp4_transposed / cast_to_mxfp6_transposed reach, and tests/guard.py's table lists the wrappers HipKernels
itself defines."""
import pytest
import torch

from tests import guard as guard_module
from tests.guard import Guard
from tests.mxt46_ref import FORMATS
from tests.mxt_ref import mxt_input

pytestmark = pytest.mark.gpu

OUTPUTS = {fmt.wrapper: ('q_t', 'sf_t', 'q', 'sf') for fmt in FORMATS}


@pytest.fixture
def guard(monkeypatch):
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    for name, outs in OUTPUTS.items():
        monkeypatch.setitem(guard_module.OUTPUTS, name, outs)
    return Guard(HipKernels())


def test_the_declared_outputs_are_parameters_of_the_wrappers():
    import inspect
    from deepep_amd.kernels import HipKernels, TransposedFp4Fp6Kernels
    for name, outs in OUTPUTS.items():
        assert name in vars(TransposedFp4Fp6Kernels)
        assert set(outs) <= set(inspect.signature(getattr(HipKernels, name)).parameters)
    public = sorted(n for n, v in vars(TransposedFp4Fp6Kernels).items() if callable(v) and not n.startswith('_'))
    assert public == sorted(OUTPUTS)                            # every wrapper of the mixin that writes is declared


@pytest.mark.parametrize('N,H', [(128, 128), (384, 640), (640, 7168), (1024, 256)])
@pytest.mark.parametrize('fmt', FORMATS, ids=repr)
def test_both_forms_stay_inside_their_outputs(guard, fmt, N, H):
    x_cpu = mxt_input(N, H, N + H)
    want_t, want_row = fmt.transposed_pair(x_cpu), fmt.rowwise_pair(x_cpu)
    x = x_cpu.cuda()
    wide = torch.zeros((N, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x
    calls = 0
    for xin in (x, wide[:, :H]):
        for rowwise in (False, True):
            q_t = torch.empty((H, fmt.row_bytes(N)), dtype=torch.uint8, device='cuda')
            sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device='cuda')
            q = torch.empty((N, fmt.row_bytes(H)), dtype=torch.uint8, device='cuda') if rowwise else None
            sf = torch.empty((N, H // 32), dtype=torch.uint8, device='cuda') if rowwise else None
            getattr(guard, fmt.wrapper)(xin, q_t, sf_t, q, sf)
            calls += 1
            assert torch.equal(q_t.cpu(), want_t[0]) and torch.equal(sf_t.cpu(), want_t[1])
            if rowwise:
                assert torch.equal(q.cpu(), want_row[0]) and torch.equal(sf.cpu(), want_row[1])
    assert guard.guarded_calls == calls
    assert guard.verify() >= 2 * calls                          # q_t and sf_t of every call, q and sf of half of them
