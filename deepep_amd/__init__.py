"""deepep_amd: DeepEP's ElasticBuffer combine path, built for AMD Instinct MI355X (gfx950).

Drop-in surface of `deep_ep` for the combine reduction:
    ElasticBuffer, EPHandle, EventOverlap, EventHandle, topk_idx_t
(deep_ep/__init__.py:90-97 in the reference).  The combine kernels live in
libdeepep_amd.so (hand-written HIP, C-ABI in include/deepep_amd.h).
"""
from .buffer import ElasticBuffer, calculate_buffer_size, topk_idx_t
from .event import EventHandle, EventOverlap
from .handle import EPHandle


def per_token_cast_to_fp8(x, round_scale: bool = False, use_ue8m0: bool = False, *, group_size: int = 128):
    """The reference's per_token_cast_to_fp8 (deep_ep/utils/math.py:30-39) as one HIP kernel: bf16 x [T, H] on
    the GPU, H % 128 == 0 (rows may be strided) -> (float8_e4m3fn [T, H], float32 [T, H / 128]), the pair
    dispatch((x_fp8, sf), ...) takes -- bit for bit what the torch code gives on the CPU.  round_scale:
    power-of-two scale factors (calculate_fp8_scales(round_scale=true), csrc/kernels/legacy/utils.cuh:494-503).
    use_ue8m0 (needs round_scale, as the reference's low-latency dispatch does, csrc/kernels/legacy/
    internode_ll.cu:509-510, and H % 512 == 0): the scale factors come packed, int32 [T, H / 512] -- byte j
    (little-endian) of element p is the biased exponent of column group 4p + j's power-of-two factor, the
    reference's use_ue8m0 form (groups of 128 columns); the e4m3fn bytes are the round_scale bytes.
    group_size=32 (extension; needs round_scale and use_ue8m0, H % 128 == 0): MXFP8, the operand of CDNA4's
    block-scaled MFMA (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32 elements along K) -> (float8_e4m3fn
    [T, H], uint8 [T, H / 32]), byte g of a row the biased exponent of column group g, a free
    .view(torch.float8_e8m0fnu).  The rule is the round_scale rule over 32 columns -- the library's own
    power-of-two ceiling (e = exponent(v) + (mantissa(v) != 0), v = amax / 448), so no element saturates; it is not
    the OCP floor rule.  Either rule's output is a valid MX operand; only this one is bit-compatible with the
    per-128 path.  Any other group_size raises.
    Runs on the current stream, no host synchronisation; NaN / Inf inputs are unspecified."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp8 takes a 2-D bfloat16 tensor with hidden % 128 == 0')
    if group_size not in (32, 128):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp8 scales groups of 128 columns or, as MXFP8, of 32')
    if group_size == 32 and not (round_scale and use_ue8m0):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp8 group_size=32 (MXFP8) needs round_scale and '
                           'use_ue8m0')
    from .kernels import HipKernels, sf_format
    fmt = sf_format(ue8m0=use_ue8m0 and group_size != 32, mx=group_size == 32)
    if (fmt.needs_round_scale and not round_scale) or x.shape[1] % fmt.multiple != 0:
        raise RuntimeError(f'Assertion failed: per_token_cast_to_fp8 gives {fmt.name} scale factors with round_scale '
                           f'only, for hidden % {fmt.multiple} == 0')
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    sf = torch.empty((x.shape[0], fmt.elems(x.shape[1])), dtype=fmt.dtype, device=x.device)
    HipKernels().cast_fp8(x, q, sf, round_scale, **fmt.kw)
    return q, sf


def per_token_cast_back(x_fp8, x_scales):
    """The reference's per_token_cast_back (deep_ep/utils/math.py:42-56) as one HIP kernel, for the pair an FP8
    dispatch returns: x_fp8 float8_e4m3fn [M, H] on the GPU, H % 128 == 0 (rows may be strided), x_scales
    float32 [M, H / 128] of any strides (the column-major tensor of use_tma_aligned_col_major_sf is read in
    place) -> contiguous bf16 [M, H], bit for bit what the torch code gives on the CPU: an exact e4m3fn -> fp32
    conversion, one fp32 multiply by the group's scale factor, one round-to-nearest-even to bf16.  Covers
    finite bytes and positive, finite, normal scale factors; the NaN bytes come out NaN.  Packed UE8M0
    scale factors (the reference's torch.int form, deep_ep/utils/math.py:51-53): x_scales int32 [M, H / 512] of
    any strides, H % 512 == 0, byte j of element p the exponent byte of column group 4p + j; the factor is
    float_from_bits(byte << 23), so for the pairs per_token_cast_to_fp8(use_ue8m0=True) gives the result is the
    fp32 form's, bit for bit (byte 0 multiplies by +0.0).  MXFP8 scale factors (per_token_cast_to_fp8(...,
    group_size=32)): x_scales uint8 or float8_e8m0fnu [M, H / 32] of any strides, one exponent byte per 32 columns,
    the same arithmetic.  Runs on the current stream, no host synchronisation;
    M == 0 returns an empty tensor without a launch."""
    import torch
    if not (isinstance(x_fp8, torch.Tensor) and x_fp8.dim() == 2 and x_fp8.dtype == torch.float8_e4m3fn and
            x_fp8.shape[1] > 0 and x_fp8.shape[1] % 128 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_back takes a 2-D float8_e4m3fn tensor with hidden % 128 == 0')
    M, H = x_fp8.shape
    from .kernels import HipKernels, sf_format_of
    fmt = sf_format_of(x_scales.dtype) if isinstance(x_scales, torch.Tensor) else None
    if fmt is None:
        raise RuntimeError('Assertion failed: per_token_cast_back takes float32, packed UE8M0 (torch.int32) or MXFP8 '
                           '(torch.uint8 or torch.float8_e8m0fnu) scale factors')
    if not (H % fmt.multiple == 0 and x_scales.dim() == 2 and tuple(x_scales.shape) == (M, fmt.elems(H)) and
            x_scales.device == x_fp8.device):
        raise RuntimeError(f'Assertion failed: per_token_cast_back takes {fmt} on the device of x_fp8, '
                           f'hidden % {fmt.multiple} == 0')
    out = torch.empty(x_fp8.shape, dtype=torch.bfloat16, device=x_fp8.device)
    if x_fp8.shape[0] == 0:
        return out
    HipKernels().cast_back_fp8(x_fp8, x_scales, out)
    return out


def per_token_cast_to_fp4(x):
    """MXFP4, the FP4 operand of CDNA4's block-scaled MFMA (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32 elements
    along K), as one HIP kernel: bf16 x [T, H] on the GPU, H % 128 == 0 (rows may be strided) -> (uint8 [T, H / 2],
    uint8 [T, H / 32]), the pair dispatch((x_fp4, sf), ...) takes.  Byte j of a row holds the e2m1 code of column 2j in
    bits 3:0 and of column 2j + 1 in bits 7:4 (a free .view(torch.float4_e2m1fn_x2)); a code is s eem, magnitudes
    0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6.  The scale factors are MXFP8's tensor (a free .view(torch.float8_e8m0fnu)).
    Per group of 32 columns, the library's power-of-two ceiling rule with 6 in place of 448 (not the OCP floor rule):
    amax = max(max|x|, 1e-4); v = amax * fp32(1 / 6); e = exponent(v) + (mantissa(v) != 0); byte = e + 127;
    code = sign(x) | e2m1_rne(|x| * 2^-e), ties to the even code, the sign bit of x always kept -- no element
    saturates.  Runs on the current stream, no host synchronisation; NaN / Inf inputs are unspecified."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0 and
            x.shape[1] > 0):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp4 takes a 2-D bfloat16 tensor with hidden % 128 == 0')
    from .kernels import HipKernels
    T, H = x.shape
    q = torch.empty((T, H // 2), dtype=torch.uint8, device=x.device)
    sf = torch.empty((T, H // 32), dtype=torch.uint8, device=x.device)
    if T:
        HipKernels().cast_fp4(x, q, sf)
    return q, sf


def per_token_cast_back_fp4(x_fp4, x_scales):
    """The inverse of per_token_cast_to_fp4 as one HIP kernel, for the pair an MXFP4 dispatch returns: x_fp4 uint8 or
    float4_e2m1fn_x2 [M, H / 2] on the GPU, H % 128 == 0 (rows may be strided), x_scales uint8 or float8_e8m0fnu
    [M, H / 32] of any strides (column-major scale factors are read in place) -> contiguous bf16 [M, H] =
    bf16_rne(fp32(code) * float_from_bits(byte << 23)); byte 0 multiplies by +0.0 (signed zeros).  Runs on the
    current stream, no host synchronisation; M == 0 returns an empty tensor without a launch."""
    import torch
    from .kernels import FP4_ROW_DTYPES, MX_SF_DTYPES
    if not (isinstance(x_fp4, torch.Tensor) and x_fp4.dim() == 2 and x_fp4.dtype in FP4_ROW_DTYPES and
            x_fp4.shape[1] > 0 and x_fp4.shape[1] % 64 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_back_fp4 takes 2-D uint8 or float4_e2m1fn_x2 rows of '
                           'hidden / 2 bytes, hidden % 128 == 0')
    M, H = x_fp4.shape[0], x_fp4.shape[1] * 2
    if not (isinstance(x_scales, torch.Tensor) and x_scales.dtype in MX_SF_DTYPES and x_scales.dim() == 2 and
            tuple(x_scales.shape) == (M, H // 32) and x_scales.device == x_fp4.device):
        raise RuntimeError('Assertion failed: per_token_cast_back_fp4 takes uint8 or float8_e8m0fnu [M, hidden / 32] '
                           'scale factors on the device of x_fp4')
    out = torch.empty((M, H), dtype=torch.bfloat16, device=x_fp4.device)
    if M == 0:
        return out
    from .kernels import HipKernels
    HipKernels().cast_back_fp4(x_fp4, x_scales, out)
    return out


def per_token_cast_to_fp6(x):
    """MXFP6 (e2m3), the FP6 operand of CDNA4's block-scaled MFMA (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32
    elements along K; FP6 runs at the FP4 rate), as one HIP kernel: bf16 x [T, H] on the GPU, H % 128 == 0 (rows may
    be strided) -> (uint8 [T, 3 * H / 4], uint8 [T, H / 32]), the pair dispatch((x_fp6, sf), ...) takes.  A group of 32
    columns is 24 bytes, group g at bytes [24g, 24g + 24) of a row, read as a little-endian 192-bit string with column
    c in bits 6c + 5 : 6c (columns 4j .. 4j + 3 are the 24-bit word c0 | c1 << 6 | c2 << 12 | c3 << 18 in bytes
    3j .. 3j + 2): the order of v_cvt_scalef32_pk32_fp6_bf16.  A code is s ee mmm: magnitude mmm / 8 for ee == 0, else
    (1 + mmm / 8) * 2^(ee - 1), at most 7.5.  The scale factors are MXFP8's tensor (a free
    .view(torch.float8_e8m0fnu)).  Per group, the library's power-of-two ceiling rule with 7.5 in place of 448 (not
    the OCP floor rule): amax = max(max|x|, 1e-4); v = amax * fp32(1 / 7.5); e = exponent(v) + (mantissa(v) != 0);
    byte = e + 127; code = sign(x) | e2m3_rne(|x| * 2^-e), ties to the even code, the sign bit of x always kept -- no
    element saturates.  Runs on the current stream, no host synchronisation; NaN / Inf inputs are unspecified."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0 and
            x.shape[1] > 0):
        raise RuntimeError('Assertion failed: per_token_cast_to_fp6 takes a 2-D bfloat16 tensor with hidden % 128 == 0')
    from .kernels import HipKernels
    T, H = x.shape
    q = torch.empty((T, 3 * H // 4), dtype=torch.uint8, device=x.device)
    sf = torch.empty((T, H // 32), dtype=torch.uint8, device=x.device)
    if T:
        HipKernels().cast_fp6(x, q, sf)
    return q, sf


def per_token_cast_back_fp6(x_fp6, x_scales):
    """The inverse of per_token_cast_to_fp6 as one HIP kernel, for the pair an MXFP6 dispatch returns: x_fp6 uint8
    [M, 3 * H / 4] on the GPU, H % 128 == 0 (rows may be strided), x_scales uint8 or float8_e8m0fnu [M, H / 32] of any
    strides (column-major scale factors are read in place) -> contiguous bf16 [M, H] =
    bf16_rne(fp32(code) * float_from_bits(byte << 23)); byte 0 multiplies by +0.0 (signed zeros).  Runs on the
    current stream, no host synchronisation; M == 0 returns an empty tensor without a launch."""
    import torch
    from .kernels import MX_SF_DTYPES
    if not (isinstance(x_fp6, torch.Tensor) and x_fp6.dim() == 2 and x_fp6.dtype == torch.uint8 and
            x_fp6.shape[1] > 0 and x_fp6.shape[1] % 96 == 0):
        raise RuntimeError('Assertion failed: per_token_cast_back_fp6 takes 2-D uint8 rows of 3 * hidden / 4 bytes, '
                           'hidden % 128 == 0')
    M, H = x_fp6.shape[0], x_fp6.shape[1] // 3 * 4
    if not (isinstance(x_scales, torch.Tensor) and x_scales.dtype in MX_SF_DTYPES and x_scales.dim() == 2 and
            tuple(x_scales.shape) == (M, H // 32) and x_scales.device == x_fp6.device):
        raise RuntimeError('Assertion failed: per_token_cast_back_fp6 takes uint8 or float8_e8m0fnu [M, hidden / 32] '
                           'scale factors on the device of x_fp6')
    out = torch.empty((M, H), dtype=torch.bfloat16, device=x_fp6.device)
    if M == 0:
        return out
    from .kernels import HipKernels
    HipKernels().cast_back_fp6(x_fp6, x_scales, out)
    return out


def cast_to_mxfp8_transposed(x, *, with_rowwise: bool = False):
    """The transposed MXFP8 cast as one HIP kernel: the operand of CDNA4's block-scaled MFMA
    (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32 elements along K) for a GEMM that contracts over TOKENS -- an
    expert's weight gradient dW_e = dY_e^T . X_e, both of whose operands are the expanded rows a dispatch returns
    (expert_alignment=128 gives the row count this needs).  bf16 x [N, H] on the GPU, N % 128 == 0, H % 128 == 0,
    H > 0; rows may be strided (unit column stride, row stride a multiple of 8 elements) ->
        q_t  float8_e4m3fn [H, N], contiguous;  sf_t uint8 [H, N / 32], contiguous (a free .view(torch.float8_e8m0fnu))
    bit for bit per_token_cast_to_fp8(x.t().contiguous(), round_scale=True, use_ue8m0=True, group_size=32), without
    the bf16 [H, N] copy: per block g of 32 consecutive tokens and per column c, amax = max(max|x[32g:32g+32, c]|, 1e-4);
    v = amax * fp32(1 / 448); e = exponent(v) + (mantissa(v) != 0); sf_t[c, g] = e + 127;
    q_t[c, 32g + r] = e4m3fn_rne(fp32(x[32g + r, c]) * 2^-e).  No element saturates.  per_token_cast_back(q_t, sf_t) is
    the inverse (the bf16 of x.t()).  with_rowwise=True: the same launch also writes the row-wise pair, from the same
    single read of x, and the result is ((q, sf), (q_t, sf_t)) with (q, sf) bit for bit
    per_token_cast_to_fp8(x, round_scale=True, use_ue8m0=True, group_size=32).
    NaN / Inf inputs are unspecified, except that a block's output depends only on that block's 32 rows (uninitialised
    rows behind the valid ones of a worst-case handle cannot disturb the valid blocks).  Runs on the current stream, no
    host synchronisation, no workspace (it captures into a graph); N == 0 returns empty tensors without a launch.
    cast_to_mxfp4_transposed / cast_to_mxfp6_transposed are the same cast over the FP4 / FP6 element types."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16):
        raise RuntimeError('Assertion failed: cast_to_mxfp8_transposed takes a 2-D bfloat16 tensor')
    N, H = x.shape
    if not (H > 0 and H % 128 == 0):
        raise RuntimeError('Assertion failed: cast_to_mxfp8_transposed needs hidden % 128 == 0 and hidden > 0')
    if N % 128 != 0:
        raise RuntimeError('Assertion failed: cast_to_mxfp8_transposed needs a row count that is a multiple of 128 '
                           '(four groups of 32 tokens to a scale-factor dword; expert_alignment=128 gives it)')
    if N and not (x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= H):
        raise RuntimeError('Assertion failed: cast_to_mxfp8_transposed takes rows of unit column stride whose row '
                           'stride is a multiple of 8 elements')
    if not x.is_cuda:
        raise RuntimeError('Assertion failed: cast_to_mxfp8_transposed takes a tensor on the GPU')
    q_t = torch.empty((H, N), dtype=torch.float8_e4m3fn, device=x.device)
    sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device=x.device)
    q = torch.empty((N, H), dtype=torch.float8_e4m3fn, device=x.device) if with_rowwise else None
    sf = torch.empty((N, H // 32), dtype=torch.uint8, device=x.device) if with_rowwise else None
    if N:
        from .kernels import HipKernels
        HipKernels().cast_fp8_mx_transposed(x, q_t, sf_t, q, sf)
    return ((q, sf), (q_t, sf_t)) if with_rowwise else (q_t, sf_t)


def _cast_to_mx_transposed(name, wrapper, num, den, x, with_rowwise):
    """The argument checks, the outputs and the launch of cast_to_mxfp4_transposed / cast_to_mxfp6_transposed: 32
    elements are 32 * num / den bytes of codes."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16):
        raise RuntimeError(f'Assertion failed: {name} takes a 2-D bfloat16 tensor')
    N, H = x.shape
    if not (H > 0 and H % 128 == 0):
        raise RuntimeError(f'Assertion failed: {name} needs hidden % 128 == 0 and hidden > 0')
    if N % 128 != 0:
        raise RuntimeError(f'Assertion failed: {name} needs a row count that is a multiple of 128 '
                           '(four groups of 32 tokens to a scale-factor dword; expert_alignment=128 gives it)')
    if N and not (x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= H):
        raise RuntimeError(f'Assertion failed: {name} takes rows of unit column stride whose row '
                           'stride is a multiple of 8 elements')
    if not x.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes a tensor on the GPU')
    q_t = torch.empty((H, N * num // den), dtype=torch.uint8, device=x.device)
    sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device=x.device)
    q = torch.empty((N, H * num // den), dtype=torch.uint8, device=x.device) if with_rowwise else None
    sf = torch.empty((N, H // 32), dtype=torch.uint8, device=x.device) if with_rowwise else None
    if N:
        from .kernels import HipKernels
        getattr(HipKernels(), wrapper)(x, q_t, sf_t, q, sf)
    return ((q, sf), (q_t, sf_t)) if with_rowwise else (q_t, sf_t)


def cast_to_mxfp4_transposed(x, *, with_rowwise: bool = False):
    """The transposed MXFP4 cast as one HIP kernel: cast_to_mxfp8_transposed over e2m1 codes, the FP4 operand (twice
    the FP8 rate on CDNA4) of a block-scaled MFMA that contracts over TOKENS, the weight gradient.  bf16 x [N, H] on
    the GPU, N % 128 == 0, H % 128 == 0, H > 0; rows may be strided (unit column stride, row stride a multiple of 8
    elements) ->
        q_t  uint8 [H, N / 2], contiguous (a free .view(torch.float4_e2m1fn_x2));  sf_t uint8 [H, N / 32], contiguous
    bit for bit per_token_cast_to_fp4(x.t().contiguous()), without the bf16 [H, N] copy: byte j of row c holds the
    code of token 2j of column c in bits 3:0 and of token 2j + 1 in bits 7:4, and sf_t[c, g] is the exponent byte of
    tokens 32g .. 32g + 31 of column c under that function's ceiling rule with 6.  The codes, the tie rule and the sign
    rule (the sign of -0.0 and of a negative underflow is kept) are that function's.  per_token_cast_back_fp4(q_t, sf_t)
    is the inverse (the bf16 of the dequantised x.t()).  with_rowwise=True: the same launch also writes the row-wise
    pair, from the same single read of x, and the result is ((q, sf), (q_t, sf_t)) with (q, sf) bit for bit
    per_token_cast_to_fp4(x).
    NaN / Inf inputs are unspecified, except that a block's output depends only on that block's 32 rows (uninitialised
    rows behind the valid ones of a worst-case handle cannot disturb the valid blocks).  Runs on the current stream, no
    host synchronisation, no workspace (it captures into a graph); N == 0 returns empty tensors without a launch."""
    return _cast_to_mx_transposed('cast_to_mxfp4_transposed', 'cast_fp4_mx_transposed', 1, 2, x, with_rowwise)


def cast_to_mxfp6_transposed(x, *, with_rowwise: bool = False):
    """The transposed MXFP6 (e2m3) cast as one HIP kernel: cast_to_mxfp4_transposed over e2m3 codes, which the
    block-scaled MFMA runs at the FP4 rate with e4m3's three mantissa bits.  The same input ->
        q_t  uint8 [H, 3 * N / 4], contiguous;  sf_t uint8 [H, N / 32], contiguous
    bit for bit per_token_cast_to_fp6(x.t().contiguous()): block g of 32 tokens lies at bytes [24g, 24g + 24) of row
    c, a little-endian 192-bit string with token r in bits 6r + 5 : 6r (the order of v_cvt_scalef32_pk32_fp6_bf16), and
    sf_t[c, g] is its exponent byte under that function's ceiling rule with 7.5.  per_token_cast_back_fp6(q_t, sf_t) is
    the inverse.  with_rowwise=True returns ((q, sf), (q_t, sf_t)) with (q, sf) bit for bit per_token_cast_to_fp6(x).
    Everything else as cast_to_mxfp4_transposed."""
    return _cast_to_mx_transposed('cast_to_mxfp6_transposed', 'cast_fp6_mx_transposed', 3, 4, x, with_rowwise)


def _requant_transposed(name, wrapper, row_what, row_dtypes, num, den, q_t_dtype, sf_forms, x_q, x_scales):
    """The argument checks, the outputs and the launch of requant_mxfp8_transposed / requant_mxfp4_transposed /
    requant_mxfp6_transposed: 32 elements are 32 * num / den bytes of codes; sf_forms: the scale-factor formats taken."""
    import torch
    from .kernels import sf_format_of
    if not (isinstance(x_q, torch.Tensor) and x_q.dim() == 2 and x_q.dtype in row_dtypes):
        raise RuntimeError(f'Assertion failed: {name} takes 2-D {row_what} rows')
    N, H = x_q.shape[0], x_q.shape[1] * den // num
    if not (H > 0 and H % 128 == 0 and x_q.shape[1] * den % num == 0):
        raise RuntimeError(f'Assertion failed: {name} needs hidden % 128 == 0 and hidden > 0')
    if N % 128 != 0:
        raise RuntimeError(f'Assertion failed: {name} needs a row count that is a multiple of 128 '
                           '(four groups of 32 tokens to a scale-factor dword; expert_alignment=128 gives it)')
    fmt = sf_format_of(x_scales.dtype) if isinstance(x_scales, torch.Tensor) else None
    if fmt is None or fmt not in sf_forms:
        raise RuntimeError(f'Assertion failed: {name} takes ' + ' or '.join(str(f) for f in sf_forms))
    if not (H % fmt.multiple == 0 and x_scales.dim() == 2 and tuple(x_scales.shape) == (N, fmt.elems(H))):
        raise RuntimeError(f'Assertion failed: {name} takes {fmt}, hidden % {fmt.multiple} == 0')
    if x_scales.device != x_q.device:
        raise RuntimeError(f'Assertion failed: {name} takes the scale factors on the device of the rows')
    if not x_q.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes tensors on the GPU')
    if N and not (x_q.stride(1) == 1 and x_q.stride(0) % 16 == 0 and x_q.stride(0) >= x_q.shape[1]):
        raise RuntimeError(f'Assertion failed: {name} takes rows of unit column stride whose row stride is a multiple '
                           'of 16 bytes')
    q_t = torch.empty((H, N * num // den), dtype=q_t_dtype, device=x_q.device)
    sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device=x_q.device)
    if N:
        from .kernels import HipKernels
        getattr(HipKernels(), wrapper)(x_q, x_scales, q_t, sf_t)
    return q_t, sf_t


def requant_mxfp8_transposed(x_fp8, x_scales):
    """A dispatched FP8 pair requantised along the tokens, as one HIP kernel: the wgrad operand
    (cast_to_mxfp8_transposed) from what dispatch(cast_to_fp8=True) returns, without the bf16 [N, H] rows between.
    x_fp8 float8_e4m3fn [N, H] on the GPU, N % 128 == 0 (expert_alignment=128 gives it), H % 128 == 0, H > 0; rows may
    be strided (unit column stride, row stride a multiple of 16 bytes).  x_scales in any form per_token_cast_back takes,
    of any strides (the column-major tensor of use_tma_aligned_col_major_sf is read in place): float32 [N, H / 128],
    packed UE8M0 int32 [N, H / 512] (H % 512 == 0), or MXFP8's uint8 / float8_e8m0fnu [N, H / 32] ->
        q_t  float8_e4m3fn [H, N], contiguous;  sf_t uint8 [H, N / 32], contiguous (a free .view(torch.float8_e8m0fnu))
    bit for bit cast_to_mxfp8_transposed(per_token_cast_back(x_fp8, x_scales)).  No new format and no new arithmetic:
    every element is cast back as there (exact e4m3fn -> fp32, one fp32 multiply by its group's factor, one round to
    nearest even to bf16 -- the rounding is part of the contract) and the bf16 values go through the token-axis rule
    unchanged.  An exponent byte 0 is the factor +0.0, so the padding rows of a casting dispatch (do_zero_padding) become
    zero rows.  NaN bytes and NaN factors are unspecified, except that a block's output depends only on that block's 32
    rows.  Runs on the current stream, no host synchronisation, no workspace (it captures into a graph); N == 0 returns
    empty tensors without a launch.  requant_mxfp4_transposed / requant_mxfp6_transposed are the same over the FP4 /
    FP6 pairs."""
    import torch
    from .kernels import SF_FORMATS
    return _requant_transposed('requant_mxfp8_transposed', 'requant_fp8_mx_transposed', 'float8_e4m3fn',
                               (torch.float8_e4m3fn,), 1, 1, torch.float8_e4m3fn, SF_FORMATS, x_fp8, x_scales)


def requant_mxfp4_transposed(x_fp4, x_scales):
    """requant_mxfp8_transposed over an MXFP4 pair (dispatch(cast_to_fp4=True), per_token_cast_to_fp4): x_fp4 uint8 or
    float4_e2m1fn_x2 [N, H / 2], x_scales uint8 / float8_e8m0fnu [N, H / 32] of any strides ->
        q_t  uint8 [H, N / 2], contiguous (a free .view(torch.float4_e2m1fn_x2));  sf_t uint8 [H, N / 32], contiguous
    bit for bit cast_to_mxfp4_transposed(per_token_cast_back_fp4(x_fp4, x_scales)).  Everything else as
    requant_mxfp8_transposed."""
    import torch
    from .kernels import FP4_ROW_DTYPES, SF_MXFP8
    return _requant_transposed('requant_mxfp4_transposed', 'requant_fp4_mx_transposed', 'uint8 or float4_e2m1fn_x2',
                               FP4_ROW_DTYPES, 1, 2, torch.uint8, (SF_MXFP8,), x_fp4, x_scales)


def requant_mxfp6_transposed(x_fp6, x_scales):
    """requant_mxfp8_transposed over an MXFP6 pair (dispatch(cast_to_fp6=True), per_token_cast_to_fp6): x_fp6 uint8
    [N, 3 * H / 4], x_scales uint8 / float8_e8m0fnu [N, H / 32] of any strides ->
        q_t  uint8 [H, 3 * N / 4], contiguous;  sf_t uint8 [H, N / 32], contiguous
    bit for bit cast_to_mxfp6_transposed(per_token_cast_back_fp6(x_fp6, x_scales)).  Everything else as
    requant_mxfp8_transposed."""
    import torch
    from .kernels import SF_MXFP8
    return _requant_transposed('requant_mxfp6_transposed', 'requant_fp6_mx_transposed', 'uint8', (torch.uint8,), 3, 4,
                               torch.uint8, (SF_MXFP8,), x_fp6, x_scales)


def per_token_cast_to_logfmt(x):
    """LogFMT-10, the format combine(use_logfmt=True) moves between ranks, as one HIP kernel: bf16 x [T, H] on the
    GPU, H % 128 == 0 (rows may be strided) -> (planes uint8 [T, H + H / 4], meta int32 [T, H / 128]).  planes is
    [low plane: code & 0xff of every column | high plane: two bits per column, (sign << 1) | (code >> 8), column c
    in bits 2 * (c & 3) of byte c / 4]; meta holds amax_bits | amin_bits << 16 of each group of 128 columns.  The
    arithmetic is the reference's (csrc/kernels/legacy/internode_ll.cu:557-638) with three departures -- every
    group is encoded, degenerate and non-finite groups are exact, a decoded value is rounded to bf16 -- all in
    deepep_amd/csrc/logfmt_codec.h.  Runs on the current stream, no host synchronisation."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0 and
            x.shape[1] > 0):
        raise RuntimeError('Assertion failed: per_token_cast_to_logfmt takes a 2-D bfloat16 tensor with hidden % 128 == 0')
    if not x.is_cuda:
        raise RuntimeError('Assertion failed: per_token_cast_to_logfmt takes a tensor on the GPU')
    from .kernels import HipKernels
    T, H = x.shape
    planes = torch.empty((T, H + H // 4), dtype=torch.uint8, device=x.device)
    meta = torch.empty((T, H // 128), dtype=torch.int32, device=x.device)
    if T:
        HipKernels().cast_logfmt(x, planes, meta)
    return planes, meta


def per_token_cast_back_logfmt(planes, meta):
    """The inverse of per_token_cast_to_logfmt (csrc/kernels/legacy/internode_ll.cu:672-712) as one HIP kernel:
    planes uint8 [M, H + H / 4] and meta int32 [M, H / 128] on the GPU (rows may be strided) -> bf16 [M, H], every
    decoded value rounded to nearest even.  Runs on the current stream, no host synchronisation."""
    import torch
    if not (isinstance(planes, torch.Tensor) and isinstance(meta, torch.Tensor) and planes.dim() == 2 and
            meta.dim() == 2 and planes.dtype == torch.uint8 and meta.dtype == torch.int32):
        raise RuntimeError('Assertion failed: per_token_cast_back_logfmt takes 2-D uint8 planes and 2-D int32 meta')
    G = meta.shape[1]
    if not (G > 0 and planes.shape[1] == G * 160 and planes.shape[0] == meta.shape[0]):
        raise RuntimeError('Assertion failed: per_token_cast_back_logfmt takes planes [M, H + H / 4] and meta '
                           '[M, H / 128] of the same rows, hidden % 128 == 0')
    if not (planes.is_cuda and meta.device == planes.device):
        raise RuntimeError('Assertion failed: per_token_cast_back_logfmt takes planes and meta on one GPU')
    from .kernels import HipKernels
    out = torch.empty((planes.shape[0], G * 128), dtype=torch.bfloat16, device=planes.device)
    if planes.shape[0]:
        HipKernels().cast_back_logfmt(planes, meta, out)
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
__build_version__ = '0.8.0'
__all__ = ['ElasticBuffer', 'EPHandle', 'EventOverlap', 'EventHandle', 'topk_idx_t',
           'calculate_buffer_size', 'get_physical_domain_size', 'get_logical_domain_size', 'per_token_cast_to_fp8',
           'per_token_cast_back', 'per_token_cast_to_logfmt', 'per_token_cast_back_logfmt', 'per_token_cast_to_fp4',
           'per_token_cast_back_fp4', 'per_token_cast_to_fp6', 'per_token_cast_back_fp6',
           'cast_to_mxfp8_transposed', 'cast_to_mxfp4_transposed', 'cast_to_mxfp6_transposed',
           'requant_mxfp8_transposed', 'requant_mxfp4_transposed', 'requant_mxfp6_transposed']
