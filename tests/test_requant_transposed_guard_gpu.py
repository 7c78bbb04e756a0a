"""The requantisation along the tokens under the guard (tests/guard.py): canary bands around q_t and sf_t, in all five
forms, at the shapes at which the tiling has tails (a run of tiles that ends early along the token axis: dword
scale-factor stores; more column blocks than one; whole runs: 16-byte scale-factor stores), with contiguous and with
strided code rows.

The declaration of the wrappers is made here, for the duration of a test: they are methods of
deepep_amd.kernels.RequantTransposedKernels, the base class of HipKernels that only the package's
requant_mxfp8_transposed / requant_mxfp4_transposed / requant_mxfp6_transposed reach, and tests/guard.py's table lists
the wrappers HipKernels itself defines."""
import pytest
import torch

from tests import guard as guard_module
from tests.guard import Guard
from tests.requant_t_ref import ALL, as_bytes, pair_and_ref

pytestmark = pytest.mark.gpu

OUTPUTS = {form.wrapper: ('q_t', 'sf_t') for form in ALL}


@pytest.fixture
def guard(monkeypatch):
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    for name, outs in OUTPUTS.items():
        monkeypatch.setitem(guard_module.OUTPUTS, name, outs)
    return Guard(HipKernels())


def test_the_declared_outputs_are_parameters_of_the_wrappers():
    import inspect
    from deepep_amd.kernels import HipKernels, RequantTransposedKernels
    for name, outs in OUTPUTS.items():
        assert name in vars(RequantTransposedKernels)
        assert set(outs) <= set(inspect.signature(getattr(HipKernels, name)).parameters)
    public = sorted(n for n, v in vars(RequantTransposedKernels).items() if callable(v) and not n.startswith('_'))
    assert public == sorted(OUTPUTS)                            # every wrapper of the mixin that writes is declared


@pytest.mark.parametrize('N,H', [(128, 128), (384, 640), (640, 7168), (1024, 256)])
@pytest.mark.parametrize('form', ALL, ids=repr)
def test_every_form_stays_inside_its_outputs(guard, form, N, H):
    if H % form.h_multiple:
        H = (H + 511) // 512 * 512                              # packed factors: 128 -> 512, 640 -> 1024, 256 -> 512
    if H == 7168:
        # the reference of the wide row: the same build's two-launch route (pinned to the CPU references by its own
        # tests); the pair cast by the package's own cast
        from tests.test_requant_transposed_gpu import _composition, _wide_pair
        q, sf = (t[:N] for t in _wide_pair(form))
        want = _composition(form, q, sf)
    else:
        (q, sf), want = pair_and_ref(form, N, H)
        q, sf = q.cuda(), sf.cuda()
    wide = torch.zeros((N, q.shape[1] + 64), dtype=torch.uint8, device='cuda').view(q.dtype)
    wide[:, :q.shape[1]] = q
    calls = 0
    for rows in (q, wide[:, :q.shape[1]]):
        q_t = torch.empty((H, form.row_bytes(N)), dtype=torch.uint8, device='cuda')
        if form.fmt is None:
            q_t = q_t.view(torch.float8_e4m3fn)
        sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device='cuda')
        getattr(guard, form.wrapper)(rows, sf, q_t, sf_t)
        calls += 1
        assert torch.equal(as_bytes(q_t), as_bytes(want[0])) and torch.equal(as_bytes(sf_t), as_bytes(want[1]))
    assert guard.guarded_calls == calls
    assert guard.verify() >= 2 * calls                          # q_t and sf_t of every call
