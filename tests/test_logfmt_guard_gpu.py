"""The three new writers of the LogFMT path -- cast_logfmt, cast_back_logfmt and logfmt_pack_rows -- and the LogFMT
epilogue under the guard (tests/guard.py): canary bands around every output their wrappers declare, at the shapes at
which each store pattern has a tail (one group, a part of a pass, two passes and a part; row counts that end inside a
workgroup of four rows).

The declarations of the three wrappers are made here, for the duration of a test: they are methods of
deepep_amd.kernels.LogfmtKernels, the base class of HipKernels that only a combine(use_logfmt=True) reaches, and
tests/guard.py's table lists the wrappers HipKernels itself defines."""
import pytest
import torch

from tests import guard as guard_module
from tests.guard import Guard

pytestmark = pytest.mark.gpu

MODE_EPILOGUE = 1
LOGFMT_OUTPUTS = {'cast_logfmt': ('planes', 'meta'), 'cast_back_logfmt': ('out',), 'logfmt_pack_rows': ('dst',)}


@pytest.fixture
def guard(monkeypatch):
    from deepep_amd.kernels import HipKernels
    assert torch.cuda.is_available()
    for name, outs in LOGFMT_OUTPUTS.items():
        monkeypatch.setitem(guard_module.OUTPUTS, name, outs)
    return Guard(HipKernels())


def _clean(guard, at_least):
    assert guard.guarded_calls >= at_least, f'{guard.guarded_calls} guarded calls'
    assert guard.verify() >= at_least


def test_the_declared_outputs_are_parameters_of_the_wrappers():
    import inspect
    from deepep_amd.kernels import HipKernels, LogfmtKernels
    for name, outs in LOGFMT_OUTPUTS.items():
        assert name in vars(LogfmtKernels) and set(outs) <= set(inspect.signature(getattr(HipKernels, name)).parameters)
    public = sorted(n for n, v in vars(LogfmtKernels).items() if callable(v) and not n.startswith('_'))
    assert public == sorted(LOGFMT_OUTPUTS)                     # every LogFMT wrapper that writes is declared here


@pytest.mark.parametrize('rows', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 384, 2176, 7168])
def test_codec_kernels(guard, H, rows):
    from tests.test_logfmt_gpu import _cast_input
    x = _cast_input(H)[0][:rows].cuda()
    wide = torch.zeros((rows, H + 64), dtype=torch.bfloat16, device='cuda')
    wide[:, :H] = x
    outs = []
    for xin in (x, wide[:, :H]):
        planes = torch.empty((rows, H * 5 // 4), dtype=torch.uint8, device='cuda')
        meta = torch.empty((rows, H // 128), dtype=torch.int32, device='cuda')
        guard.cast_logfmt(xin, planes, meta)
        out = torch.empty((rows, H), dtype=torch.bfloat16, device='cuda')
        guard.cast_back_logfmt(planes, meta, out)
        outs.append((planes, meta, out))
    _clean(guard, 4)
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:2], outs[1][:2]))
    assert torch.equal(outs[0][2].view(torch.int16), outs[1][2].view(torch.int16))


@pytest.mark.parametrize('single, K', [(False, 3), (True, 8), (None, 8)])
@pytest.mark.parametrize('H', [128, 384, 2176, 7168])
def test_pack_rows(guard, H, single, K):
    from deepep_amd.handle import logfmt_row_layout, packed_row_layout
    from tests.test_logfmt_gpu import _cast_input
    with_w = single is not None
    rb, w_off, _ = packed_row_layout(H, K, with_w, bool(single))
    lb, lw_off, _ = logfmt_row_layout(H, K, with_w, bool(single))
    for n in (1, 5, 129):
        src = torch.zeros((n, rb), dtype=torch.uint8, device='cuda')
        src[:, :H * 2] = _cast_input(H)[0][:n].cuda().view(torch.uint8).view(n, H * 2)
        dst = torch.zeros((n + 2, lb), dtype=torch.uint8, device='cuda')
        # the destination as the exchange hands it over: the whole allocation, of which the first n rows are written
        guard.logfmt_pack_rows(src.view(torch.bfloat16), n, H, dst[:n], src_tail_offset=w_off, dst_tail_offset=lw_off,
                               tail_bytes=lb - lw_off)
    _clean(guard, 3)


@pytest.mark.parametrize('H', [128, 384, 2176])
def test_logfmt_epilogue(guard, H):
    from tests.test_logfmt_gpu import _epilogue_both, _epilogue_table
    fails = []
    for width in (1, 3, 8, 9):
        table = _epilogue_table(width, H + width)
        for weighted, biases, weights in ((False, 0, False), (True, 2, True), (False, 1, True)):
            bad = _epilogue_both(guard, H, table, weighted, biases, weights, seed=width)
            if bad:
                fails.append((width, weighted, biases, weights, bad))
    assert not fails, fails
    _clean(guard, 8)
