"""deepep_amd: DeepEP's ElasticBuffer combine path, built for AMD Instinct MI355X (gfx950).

Drop-in surface of `deep_ep` for the combine reduction:
    ElasticBuffer, EPHandle, EventOverlap, EventHandle, topk_idx_t
(deep_ep/__init__.py:90-97 in the reference).  The combine kernels live in
libdeepep_amd.so (hand-written HIP, C-ABI in include/deepep_amd.h).
"""
from .buffer import ElasticBuffer, calculate_buffer_size, topk_idx_t
from .event import EventHandle, EventOverlap
from .handle import EPHandle


def per_token_cast_to_fp8(x, round_scale: bool = False):
    """The reference's per_token_cast_to_fp8 (deep_ep/utils/math.py:30-39) as one HIP kernel: bf16 x [T, H] on
    the GPU, H % 128 == 0 (rows may be strided) -> (float8_e4m3fn [T, H], float32 [T, H / 128]), the pair
    dispatch((x_fp8, sf), ...) takes -- bit for bit what the torch code gives on the CPU.  round_scale:
    power-of-two scale factors (calculate_fp8_scales(round_scale=true), csrc/kernels/legacy/utils.cuh:494-503).
    Runs on the current stream, no host synchronisation; NaN / Inf inputs are unspecified."""
    import torch
    from .kernels import HipKernels
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp8 takes a 2-D bfloat16 tensor with hidden % 128 == 0')
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    sf = torch.empty((x.shape[0], x.shape[1] // 128), dtype=torch.float32, device=x.device)
    HipKernels().cast_fp8(x, q, sf, round_scale)
    return q, sf


def per_token_cast_back(x_fp8, x_scales):
    """The reference's per_token_cast_back (deep_ep/utils/math.py:42-56) as one HIP kernel, for the pair an FP8
    dispatch returns: x_fp8 float8_e4m3fn [M, H] on the GPU, H % 128 == 0 (rows may be strided), x_scales
    float32 [M, H / 128] of any strides (the column-major tensor of use_tma_aligned_col_major_sf is read in
    place) -> contiguous bf16 [M, H], bit for bit what the torch code gives on the CPU: an exact e4m3fn -> fp32
    conversion, one fp32 multiply by the group's scale factor, one round-to-nearest-even to bf16.  Covers
    finite bytes and positive, finite, normal scale factors; the NaN bytes come out NaN.  Packed UE8M0
    (torch.int) scale factors are not supported and are rejected.  Runs on the current stream, no host
    synchronisation; M == 0 returns an empty tensor without a launch."""
    import torch
    if not (isinstance(x_fp8, torch.Tensor) and x_fp8.dim() == 2 and x_fp8.dtype == torch.float8_e4m3fn and
            x_fp8.shape[1] > 0 and x_fp8.shape[1] % 128 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_back takes a 2-D float8_e4m3fn tensor with hidden % 128 == 0')
    if not (isinstance(x_scales, torch.Tensor) and x_scales.dtype == torch.float32):
        raise RuntimeError('Assertion failed: per_token_cast_back takes float32 scale factors '
                           '(packed UE8M0 torch.int scale factors are not supported)')
    if not (x_scales.dim() == 2 and tuple(x_scales.shape) == (x_fp8.shape[0], x_fp8.shape[1] // 128) and
            x_scales.device == x_fp8.device):
        raise RuntimeError('Assertion failed: per_token_cast_back takes scale factors [M, H / 128] on the device of x_fp8')
    out = torch.empty(x_fp8.shape, dtype=torch.bfloat16, device=x_fp8.device)
    if x_fp8.shape[0] == 0:
        return out
    from .kernels import HipKernels
    HipKernels().cast_back_fp8(x_fp8, x_scales, out)
    return out


def get_physical_domain_size(group=None):
    """(RDMA ranks, xGMI ranks) of a single-node group."""
    import torch.distributed as dist
    n = dist.get_world_size(group)
    return 1, n


def get_logical_domain_size(group=None, allow_hybrid_mode: bool = True):
    """(scale-out ranks, scale-up ranks) of a single-node group."""
    import torch.distributed as dist
    n = dist.get_world_size(group)
    return 1, n


# The API level implemented: the reference's deep_ep.__version__ (deep_ep/__init__.py:97), so caller
# code that gates on it sees the library it was written against.  This build's own version is
# __build_version__; the library's source hash is deepep_amd._lib.source_build_id().
__version__ = '2.1.0'
__build_version__ = '0.6.0'
__all__ = ['ElasticBuffer', 'EPHandle', 'EventOverlap', 'EventHandle', 'topk_idx_t',
           'calculate_buffer_size', 'get_physical_domain_size', 'get_logical_domain_size', 'per_token_cast_to_fp8',
           'per_token_cast_back']
