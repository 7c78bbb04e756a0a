"""deepep_cast_back_fp8 (HipKernels.cast_back_fp8, deepep_amd.per_token_cast_back) on the GPU against the torch
code of per_token_cast_back (workloads.py; the reference's deep_ep/utils/math.py:42-56) run on the CPU -- bitwise:
an exact e4m3fn -> fp32 conversion, one fp32 multiply by the group's scale factor, one round-to-nearest-even to
bf16.  The two NaN bytes (0x7f, 0xff) are compared by isnan (payload unspecified)."""
import numpy as np
import pytest
import torch

from tests.test_fp8_cast_gpu import _same, cast_ref
from workloads import per_token_cast_back as torch_cast_back

pytestmark = pytest.mark.gpu


def back_ref(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """bf16 [M, H] of the pair, computed on the CPU."""
    return torch_cast_back(q.cpu().contiguous(), sf.cpu().contiguous())


def _fp8(codes: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)


def _random_pair(M, H, seed):
    """Random finite e4m3fn bytes and positive normal scale factors over 12 binades."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(M, H), dtype=np.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x3c
    sf = (rng.random((M, H // 128), dtype=np.float32) + 0.5) * np.exp2(rng.integers(-9, 3, size=(M, H // 128))).astype(np.float32)
    return _fp8(codes), torch.from_numpy(sf)


def _check(q_cpu, sf_cpu, q_gpu=None, sf_gpu=None):
    import deepep_amd
    out = deepep_amd.per_token_cast_back(q_cpu.cuda() if q_gpu is None else q_gpu,
                                         sf_cpu.cuda() if sf_gpu is None else sf_gpu)
    torch.cuda.synchronize()
    ref = back_ref(q_cpu, sf_cpu)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == ref.shape
    got = out.cpu()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan)
    bad = ((got.view(torch.int16) != ref.view(torch.int16)) & ~nan).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} values differ, first at {bad[0].tolist()}: ' \
                             f'{got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}'
    return ref


def test_cast_back_exhaustive():
    """All 256 bytes in every column position of a 128-column group, against each of five scale factors."""
    clamp = (torch.tensor(1e-4, dtype=torch.float32) / 448.0).item()
    scales = torch.tensor([clamp, 1.0 / 448.0, 1.0, 2.0 ** -10, 2.0 ** 3], dtype=torch.float32)
    r, c = np.arange(1280).reshape(1280, 1), np.arange(640).reshape(1, 640)
    q = _fp8((r + c) % 256)                                    # column c of row r holds byte (r + c) % 256
    # five blocks of 256 rows: inside a block a group keeps one scale factor while every column of it runs
    # through all 256 bytes; over the blocks every group meets every scale factor
    g = (r // 256 + np.arange(5).reshape(1, 5)) % 5
    sf = scales[torch.from_numpy(g)]
    ref = _check(q, sf)
    assert int(ref.isnan().sum()) == 5 * 2 * 640               # 0x7f and 0xff once per column and block
    assert ref[0, 0].item() == 0 and ref[0x7e, 256].item() == 448.0     # byte 0x7e at scale factor 1.0


@pytest.mark.parametrize('M', [1, 5, 129])
@pytest.mark.parametrize('H', [128, 384, 2176, 7168])
def test_cast_back_shapes(M, H):
    q, sf = _random_pair(M, H, M * 10007 + H)
    _check(q, sf)


@pytest.mark.parametrize('round_scale', [False, True])
def test_cast_back_of_the_cast_pair(round_scale):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((67, 384), generator=g) * 3).to(torch.bfloat16)
    x[3, 128:256] = 0                                          # a clamped group: the smallest scale factor
    q, sf = cast_ref(x, round_scale)
    ref = _check(q, sf)
    assert bool((ref[3, 128:256] == 0).all())


def test_cast_back_strided_rows_and_column_major_scales():
    M, H = 37, 384
    q, sf = _random_pair(M, H, 9)
    wide = torch.zeros((M, H + 16), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    wide.view(torch.uint8)[:, :H] = q.view(torch.uint8).cuda()
    view = wide[:, :H]
    assert view.stride(0) == H + 16 and not view.is_contiguous()
    _check(q, sf, q_gpu=view)
    # the column-major scale factors of use_tma_aligned_col_major_sf: read in place, no copy
    col = torch.empty_strided((M, H // 128), (1, 40), dtype=torch.float32, device='cuda')
    col.copy_(sf.cuda())
    assert col.stride() == (1, 40)
    _check(q, sf, sf_gpu=col)
    _check(q, sf, q_gpu=view, sf_gpu=col)


def test_cast_back_no_rows_and_wrapper_rejections():
    import deepep_amd
    from deepep_amd.kernels import HipKernels
    out = deepep_amd.per_token_cast_back(torch.empty((0, 256), dtype=torch.float8_e4m3fn, device='cuda'),
                                         torch.empty((0, 2), dtype=torch.float32, device='cuda'))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 256)
    kern = HipKernels()
    q = torch.zeros((4, 256), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)
    sf = torch.ones((4, 2), dtype=torch.float32, device='cuda')
    out = torch.full((4, 256), 7.0, dtype=torch.bfloat16, device='cuda')
    bad = [dict(q=q.view(torch.uint8)), dict(q=q.cpu()), dict(q=q[:, :192]), dict(q=q.t()),
           dict(sf=sf.to(torch.int32)), dict(sf=sf[:, :1]), dict(sf=sf.cpu()),
           dict(out=out.float()), dict(out=out[:, :128]), dict(out=out.t()),
           dict(q=torch.zeros((4, 264), dtype=torch.uint8, device='cuda').view(torch.float8_e4m3fn)[:, 8:])]   # rows 8 bytes off
    for kw in bad:
        args = dict(dict(q=q, sf=sf, out=out), **kw)
        with pytest.raises(RuntimeError):
            kern.cast_back_fp8(args['q'], args['sf'], args['out'])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    kern.cast_back_fp8(q, sf, out)
    torch.cuda.synchronize()
    assert _same(out, torch.zeros((4, 256), dtype=torch.bfloat16))
