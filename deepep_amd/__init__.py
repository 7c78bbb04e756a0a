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


def _per_token_cast_to_mx(mx, x):
    """The argument checks, the outputs and the launch of per_token_cast_to_fp4 / per_token_cast_to_fp6."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 and x.shape[1] % 128 == 0 and
            x.shape[1] > 0):
        raise RuntimeError(f'Assertion failed: per_token_cast_to_{mx.name} takes a 2-D bfloat16 tensor with '
                           'hidden % 128 == 0')
    from .kernels import HipKernels
    T, H = x.shape
    q = torch.empty((T, mx.row_bytes(H)), dtype=mx.out_dtype, device=x.device)
    sf = torch.empty((T, H // 32), dtype=torch.uint8, device=x.device)
    if T:
        getattr(HipKernels(), f'cast_{mx.name}')(x, q, sf)
    return q, sf


def _per_token_cast_back_mx(mx, x_q, x_scales):
    """The same of per_token_cast_back_fp4 / per_token_cast_back_fp6."""
    import torch
    from .kernels import MX_SF_DTYPES
    name = f'per_token_cast_back_{mx.name}'
    if not (isinstance(x_q, torch.Tensor) and x_q.dim() == 2 and x_q.dtype in mx.row_dtypes and
            x_q.shape[1] > 0 and x_q.shape[1] % mx.row_bytes(128) == 0):
        raise RuntimeError(f'Assertion failed: {name} takes 2-D {mx.dtype_words(" or ")} rows of '
                           f'{mx.row_words("hidden")} bytes, hidden % 128 == 0')
    M, H = x_q.shape[0], mx.elems(x_q.shape[1])
    if not (isinstance(x_scales, torch.Tensor) and x_scales.dtype in MX_SF_DTYPES and x_scales.dim() == 2 and
            tuple(x_scales.shape) == (M, H // 32) and x_scales.device == x_q.device):
        raise RuntimeError(f'Assertion failed: {name} takes uint8 or float8_e8m0fnu [M, hidden / 32] '
                           f'scale factors on the device of x_{mx.name}')
    out = torch.empty((M, H), dtype=torch.bfloat16, device=x_q.device)
    if M == 0:
        return out
    from .kernels import HipKernels
    getattr(HipKernels(), f'cast_back_{mx.name}')(x_q, x_scales, out)
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
    from .kernels import MXFP4
    return _per_token_cast_to_mx(MXFP4, x)


def per_token_cast_back_fp4(x_fp4, x_scales):
    """The inverse of per_token_cast_to_fp4 as one HIP kernel, for the pair an MXFP4 dispatch returns: x_fp4 uint8 or
    float4_e2m1fn_x2 [M, H / 2] on the GPU, H % 128 == 0 (rows may be strided), x_scales uint8 or float8_e8m0fnu
    [M, H / 32] of any strides (column-major scale factors are read in place) -> contiguous bf16 [M, H] =
    bf16_rne(fp32(code) * float_from_bits(byte << 23)); byte 0 multiplies by +0.0 (signed zeros).  Runs on the
    current stream, no host synchronisation; M == 0 returns an empty tensor without a launch."""
    from .kernels import MXFP4
    return _per_token_cast_back_mx(MXFP4, x_fp4, x_scales)


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
    from .kernels import MXFP6
    return _per_token_cast_to_mx(MXFP6, x)


def per_token_cast_back_fp6(x_fp6, x_scales):
    """The inverse of per_token_cast_to_fp6 as one HIP kernel, for the pair an MXFP6 dispatch returns: x_fp6 uint8
    [M, 3 * H / 4] on the GPU, H % 128 == 0 (rows may be strided), x_scales uint8 or float8_e8m0fnu [M, H / 32] of any
    strides (column-major scale factors are read in place) -> contiguous bf16 [M, H] =
    bf16_rne(fp32(code) * float_from_bits(byte << 23)); byte 0 multiplies by +0.0 (signed zeros).  Runs on the
    current stream, no host synchronisation; M == 0 returns an empty tensor without a launch."""
    from .kernels import MXFP6
    return _per_token_cast_back_mx(MXFP6, x_fp6, x_scales)


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
    from .kernels import MXFP8
    return _cast_to_mx_transposed(MXFP8, x, with_rowwise)


def _cast_to_mx_transposed(mx, x, with_rowwise):
    """The argument checks, the outputs and the launch of cast_to_mxfp8_transposed / cast_to_mxfp4_transposed /
    cast_to_mxfp6_transposed."""
    import torch
    name = f'cast_to_mx{mx.name}_transposed'
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
    q_t = torch.empty((H, mx.row_bytes(N)), dtype=mx.out_dtype, device=x.device)
    sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device=x.device)
    q = torch.empty((N, mx.row_bytes(H)), dtype=mx.out_dtype, device=x.device) if with_rowwise else None
    sf = torch.empty((N, H // 32), dtype=torch.uint8, device=x.device) if with_rowwise else None
    if N:
        from .kernels import HipKernels
        getattr(HipKernels(), f'cast_{mx.name}_mx_transposed')(x, q_t, sf_t, q, sf)
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
    from .kernels import MXFP4
    return _cast_to_mx_transposed(MXFP4, x, with_rowwise)


def cast_to_mxfp6_transposed(x, *, with_rowwise: bool = False):
    """The transposed MXFP6 (e2m3) cast as one HIP kernel: cast_to_mxfp4_transposed over e2m3 codes, which the
    block-scaled MFMA runs at the FP4 rate with e4m3's three mantissa bits.  The same input ->
        q_t  uint8 [H, 3 * N / 4], contiguous;  sf_t uint8 [H, N / 32], contiguous
    bit for bit per_token_cast_to_fp6(x.t().contiguous()): block g of 32 tokens lies at bytes [24g, 24g + 24) of row
    c, a little-endian 192-bit string with token r in bits 6r + 5 : 6r (the order of v_cvt_scalef32_pk32_fp6_bf16), and
    sf_t[c, g] is its exponent byte under that function's ceiling rule with 7.5.  per_token_cast_back_fp6(q_t, sf_t) is
    the inverse.  with_rowwise=True returns ((q, sf), (q_t, sf_t)) with (q, sf) bit for bit per_token_cast_to_fp6(x).
    Everything else as cast_to_mxfp4_transposed."""
    from .kernels import MXFP6
    return _cast_to_mx_transposed(MXFP6, x, with_rowwise)


def _requant_transposed(mx, x_q, x_scales):
    """The argument checks, the outputs and the launch of requant_mxfp8_transposed / requant_mxfp4_transposed /
    requant_mxfp6_transposed.  FP8 rows come with scale factors in every FP8 form, the others with MXFP8's only."""
    import torch
    from .kernels import MXFP8, SF_FORMATS, SF_MXFP8, sf_format_of
    name = f'requant_mx{mx.name}_transposed'
    sf_forms = SF_FORMATS if mx is MXFP8 else (SF_MXFP8,)
    if not (isinstance(x_q, torch.Tensor) and x_q.dim() == 2 and x_q.dtype in mx.row_dtypes):
        raise RuntimeError(f'Assertion failed: {name} takes 2-D {mx.dtype_words(" or ")} rows')
    N, H = x_q.shape[0], mx.elems(x_q.shape[1])
    if not (H > 0 and H % 128 == 0):                      # (whole rows only: no other width gives a multiple of 128)
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
    q_t = torch.empty((H, mx.row_bytes(N)), dtype=mx.out_dtype, device=x_q.device)
    sf_t = torch.empty((H, N // 32), dtype=torch.uint8, device=x_q.device)
    if N:
        from .kernels import HipKernels
        getattr(HipKernels(), f'requant_{mx.name}_mx_transposed')(x_q, x_scales, q_t, sf_t)
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
    from .kernels import MXFP8
    return _requant_transposed(MXFP8, x_fp8, x_scales)


def requant_mxfp4_transposed(x_fp4, x_scales):
    """requant_mxfp8_transposed over an MXFP4 pair (dispatch(cast_to_fp4=True), per_token_cast_to_fp4): x_fp4 uint8 or
    float4_e2m1fn_x2 [N, H / 2], x_scales uint8 / float8_e8m0fnu [N, H / 32] of any strides ->
        q_t  uint8 [H, N / 2], contiguous (a free .view(torch.float4_e2m1fn_x2));  sf_t uint8 [H, N / 32], contiguous
    bit for bit cast_to_mxfp4_transposed(per_token_cast_back_fp4(x_fp4, x_scales)).  Everything else as
    requant_mxfp8_transposed."""
    from .kernels import MXFP4
    return _requant_transposed(MXFP4, x_fp4, x_scales)


def requant_mxfp6_transposed(x_fp6, x_scales):
    """requant_mxfp8_transposed over an MXFP6 pair (dispatch(cast_to_fp6=True), per_token_cast_to_fp6): x_fp6 uint8
    [N, 3 * H / 4], x_scales uint8 / float8_e8m0fnu [N, H / 32] of any strides ->
        q_t  uint8 [H, 3 * N / 4], contiguous;  sf_t uint8 [H, N / 32], contiguous
    bit for bit cast_to_mxfp6_transposed(per_token_cast_back_fp6(x_fp6, x_scales)).  Everything else as
    requant_mxfp8_transposed."""
    from .kernels import MXFP6
    return _requant_transposed(MXFP6, x_fp6, x_scales)


def swiglu_cast_to_mx(h, fmt, *, expert_ends=None, expert_alignment: int = 128, with_transposed: bool = False,
                      return_act: bool = False):
    """SwiGLU between the experts' two GEMMs, fused into the MX casts, as one HIP kernel: h = grouped_gemm_mx(x, w13,
    ...), bf16 [N, 2 * I] = [gate | up] on the GPU, becomes the operand of the second grouped_gemm_mx -- and, with
    with_transposed, of grouped_gemm_mx_wgrad -- in one read of h, without the bf16 [N, I] activation between.
    I % 128 == 0, I > 0; rows may be strided (unit column stride, row stride a multiple of 8 elements).  fmt is the
    format of the result: kernels.MXFP8, kernels.MXFP6 or kernels.MXFP4 (the one format table, kernels.MX_FORMATS), or
    such a format's name, 'fp8', 'fp6' or 'fp4'.  Two rules:
      1. act = bf16_rne(g / (1 + exp(-g)) * u), g = h[:, :I], u = h[:, I:], in fp32 with the hardware's exponential and
         reciprocal and one rounding: within 2^-7 |ref| + 2^-126 of the formula in double precision.
      2. every pair returned is bit for bit what the library's cast gives for act: (q, sf) is
         per_token_cast_to_fp8(act, round_scale=True, use_ue8m0=True, group_size=32) / per_token_cast_to_fp6(act) /
         per_token_cast_to_fp4(act), and (q_t, sf_t) is cast_to_mxfp8 / mxfp6 / mxfp4_transposed(act); no new scale
         rule, no new conversion, and the row-wise pair and act are the same bits with and without with_transposed.
    -> (q, sf); with_transposed=True (needs N % 128 == 0): ((q, sf), (q_t, sf_t)); return_act=True appends act, bf16
    [N, I] -- what a framework saves when it does not recompute.
    expert_ends: handle.psum_num_recv_tokens_per_expert as it is (int32 [E] on the GPU, never read on the host), with the
    handle's expert_alignment (positive; a multiple of 128 with with_transposed).  Rows at or past
    align_up(expert_ends[-1], expert_alignment) -- the tail of a worst-case-sized handle, which grouped_gemm_mx leaves
    unwritten -- are neither read nor written: the outputs' bytes of those rows (in q_t and sf_t, of those tokens in
    every row) are uninitialised.  The alignment padding inside the range is zero rows of h and comes out as the casts'
    zero rows.  Without with_transposed a streaming kernel takes any N; with it, the transposed casts' tile behind a
    SwiGLU load stage.  NaN / Inf inputs are unspecified.  Runs on the current stream, no host synchronisation, no
    workspace (it captures into a graph); N == 0 returns empty tensors without a launch."""
    import torch
    from .kernels import MX_FORMATS
    name = 'swiglu_cast_to_mx'
    mx = next((m for m in MX_FORMATS if fmt is m or fmt == m.name), None)
    if mx is None:
        raise RuntimeError(f'Assertion failed: {name} takes fmt as one of kernels.MX_FORMATS or its name ('
                           + ', '.join(repr(m.name) for m in MX_FORMATS) + ')')
    if not (isinstance(h, torch.Tensor) and h.dim() == 2 and h.dtype == torch.bfloat16):
        raise RuntimeError(f'Assertion failed: {name} takes a 2-D bfloat16 tensor')
    N, I = h.shape[0], h.shape[1] // 2
    if not (I > 0 and I % 128 == 0 and h.shape[1] == 2 * I):
        raise RuntimeError(f'Assertion failed: {name} takes [gate | up] rows of 2 * I columns, I % 128 == 0 and I > 0')
    if with_transposed and N % 128 != 0:
        raise RuntimeError(f'Assertion failed: {name} needs a row count that is a multiple of 128 with with_transposed '
                           '(four groups of 32 tokens to a scale-factor dword; expert_alignment=128 gives it)')
    if N and not (h.stride(1) == 1 and h.stride(0) % 8 == 0 and h.stride(0) >= 2 * I):
        raise RuntimeError(f'Assertion failed: {name} takes rows of unit column stride whose row stride is a multiple '
                           'of 8 elements')
    if expert_ends is not None:
        if not (isinstance(expert_ends, torch.Tensor) and expert_ends.dtype == torch.int32 and expert_ends.dim() == 1 and
                expert_ends.numel() >= 1 and expert_ends.is_contiguous() and expert_ends.device == h.device):
            raise RuntimeError(f'Assertion failed: {name} takes expert_ends as a contiguous int32 [E] tensor on the '
                               'device of h')
        if not (isinstance(expert_alignment, int) and expert_alignment > 0 and
                (not with_transposed or expert_alignment % 128 == 0)):
            raise RuntimeError(f'Assertion failed: {name} needs a positive expert_alignment, and '
                               'expert_alignment % 128 == 0 with with_transposed')
    if not h.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes a tensor on the GPU')
    q = torch.empty((N, mx.row_bytes(I)), dtype=mx.out_dtype, device=h.device)
    sf = torch.empty((N, I // 32), dtype=torch.uint8, device=h.device)
    q_t = torch.empty((I, mx.row_bytes(N)), dtype=mx.out_dtype, device=h.device) if with_transposed else None
    sf_t = torch.empty((I, N // 32), dtype=torch.uint8, device=h.device) if with_transposed else None
    act = torch.empty((N, I), dtype=torch.bfloat16, device=h.device) if return_act else None
    if N:
        from .kernels import HipKernels
        HipKernels().swiglu_cast_mx(mx, h, q, sf, q_t, sf_t, act, expert_ends, expert_alignment)
    out = ((q, sf), (q_t, sf_t)) if with_transposed else (q, sf)
    return (*out, act) if return_act else out


def swiglu_backward_cast_to_mx(h, dact, fmt, *, expert_ends=None, expert_alignment: int = 128,
                               with_transposed: bool = False, return_dh: bool = False):
    """The backward of swiglu_cast_to_mx's activation, fused into the MX casts of its result, as one HIP kernel: h bf16
    [N, 2 * I] = [gate | up], the tensor the forward consumed, and dact bf16 [N, I], the gradient of act = silu(gate)
    * up as the dgrad grouped_gemm_mx of the second weights writes it, become dh = [dgate | dup], [N, 2 * I], as the
    operand of the first GEMM's dgrad grouped_gemm_mx -- and, with with_transposed, of its grouped_gemm_mx_wgrad --
    without the bf16 dh between.  I % 128 == 0, I > 0; both on one GPU; rows of either may be strided (unit column
    stride, row stride a multiple of 8 elements, each its own).  fmt as in swiglu_cast_to_mx.  Two rules:
      1. with t = exp(-|g|), r = 1 / (1 + t), s = (g >= 0 ? r : t r) = sigmoid(g), c = (g >= 0 ? t r : r) =
         1 - sigmoid(g): dgate = bf16_rne(da * u * (s * (1 + g * c))), dup = bf16_rne(da * (g * s)), in fp32 with the
         hardware's exponential and reciprocal and one rounding: within 2^-7 |ref| + 2^-126 of
         da u sigmoid(g) (1 + g (1 - sigmoid(g))) and da g sigmoid(g) in double precision.
      2. every pair returned is bit for bit what the library's cast gives for dh, as in swiglu_cast_to_mx: (q, sf) the
         per_token_cast_to_fpX of dh, (q_t, sf_t) its cast_to_mxfpX_transposed; the row-wise pair and dh are the same
         bits with and without with_transposed.
    -> (q, sf), q [N, mx.row_bytes(2 * I)] and sf uint8 [N, I / 16]; with_transposed=True (needs N % 128 == 0):
    ((q, sf), (q_t, sf_t)), q_t [2 * I, mx.row_bytes(N)] and sf_t uint8 [2 * I, N / 32]; return_dh=True appends dh,
    bf16 [N, 2 * I].
    expert_ends and expert_alignment mean what they mean in swiglu_cast_to_mx: rows at or past
    align_up(expert_ends[-1], expert_alignment) are neither read, in h or in dact, nor written.  Without
    with_transposed a streaming kernel takes any N; with it, the transposed casts' tile behind a load stage that makes
    dgate and then dup of a tile.  NaN / Inf inputs are unspecified.  Runs on the current stream, no host
    synchronisation, no workspace (it captures into a graph); N == 0 returns empty tensors without a launch."""
    import torch
    from .kernels import MX_FORMATS
    name = 'swiglu_backward_cast_to_mx'
    mx = next((m for m in MX_FORMATS if fmt is m or fmt == m.name), None)
    if mx is None:
        raise RuntimeError(f'Assertion failed: {name} takes fmt as one of kernels.MX_FORMATS or its name ('
                           + ', '.join(repr(m.name) for m in MX_FORMATS) + ')')
    if not all(isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.bfloat16 for x in (h, dact)):
        raise RuntimeError(f'Assertion failed: {name} takes h and dact as 2-D bfloat16 tensors')
    N, I = h.shape[0], h.shape[1] // 2
    if not (I > 0 and I % 128 == 0 and h.shape[1] == 2 * I):
        raise RuntimeError(f'Assertion failed: {name} takes [gate | up] rows of 2 * I columns, I % 128 == 0 and I > 0')
    if tuple(dact.shape) != (N, I):
        raise RuntimeError(f'Assertion failed: {name} takes dact of shape [N, I], the gradient of the activation')
    if with_transposed and N % 128 != 0:
        raise RuntimeError(f'Assertion failed: {name} needs a row count that is a multiple of 128 with with_transposed '
                           '(four groups of 32 tokens to a scale-factor dword; expert_alignment=128 gives it)')
    if N and not all(x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.stride(0) >= x.shape[1] for x in (h, dact)):
        raise RuntimeError(f'Assertion failed: {name} takes rows of unit column stride whose row stride is a multiple '
                           'of 8 elements')
    if expert_ends is not None:
        if not (isinstance(expert_ends, torch.Tensor) and expert_ends.dtype == torch.int32 and expert_ends.dim() == 1 and
                expert_ends.numel() >= 1 and expert_ends.is_contiguous() and expert_ends.device == h.device):
            raise RuntimeError(f'Assertion failed: {name} takes expert_ends as a contiguous int32 [E] tensor on the '
                               'device of h')
        if not (isinstance(expert_alignment, int) and expert_alignment > 0 and
                (not with_transposed or expert_alignment % 128 == 0)):
            raise RuntimeError(f'Assertion failed: {name} needs a positive expert_alignment, and '
                               'expert_alignment % 128 == 0 with with_transposed')
    if not (h.is_cuda and dact.device == h.device):
        raise RuntimeError(f'Assertion failed: {name} takes h and dact on the same GPU')
    q = torch.empty((N, mx.row_bytes(2 * I)), dtype=mx.out_dtype, device=h.device)
    sf = torch.empty((N, I // 16), dtype=torch.uint8, device=h.device)
    q_t = torch.empty((2 * I, mx.row_bytes(N)), dtype=mx.out_dtype, device=h.device) if with_transposed else None
    sf_t = torch.empty((2 * I, N // 32), dtype=torch.uint8, device=h.device) if with_transposed else None
    dh = torch.empty((N, 2 * I), dtype=torch.bfloat16, device=h.device) if return_dh else None
    if N:
        from .kernels import HipKernels
        HipKernels().swiglu_backward_cast_mx(mx, h, dact, q, sf, q_t, sf_t, dh, expert_ends, expert_alignment)
    out = ((q, sf), (q_t, sf_t)) if with_transposed else (q, sf)
    return (*out, dh) if return_dh else out


def _mx_operand(name, what, pair, lead, allow_empty=False):
    """The format inference of grouped_gemm_mx / grouped_gemm_mx_wgrad: pair = (codes, sf) with `lead` leading
    dimensions -> (codes, sf, the format's number, the leading shape, the elements along the contraction).  The
    contraction length is 32 * sf.shape[-1]; the code dtype and a row's bytes then pick FP8, FP4 or FP6."""
    import torch
    from .kernels import MX_SF_DTYPES, MXFP4, MXFP6, MXFP8, mx_format_of
    if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(isinstance(t, torch.Tensor) for t in pair)):
        raise RuntimeError(f'Assertion failed: {name} takes {what} as a pair (codes, scale factors) of tensors')
    q, sf = pair
    if not (sf.dtype in MX_SF_DTYPES and sf.dim() == lead + 1 and q.dim() == lead + 1 and
            tuple(sf.shape[:-1]) == tuple(q.shape[:-1]) and sf.device == q.device):
        raise RuntimeError(f'Assertion failed: {name} takes {what} as codes with uint8 or float8_e8m0fnu scale factors '
                           f'[..., K / 32] of the same leading shape ({lead + 1}-D) on one device')
    C, row = 32 * sf.shape[-1], q.shape[-1]
    mx = mx_format_of(q.dtype, row, C)
    if mx is None:
        rows = [f'{m.dtype_words()} [{m.row_bytes(C)}]' for m in (MXFP8, MXFP4, MXFP6)]
        raise RuntimeError(f'Assertion failed: {name} cannot tell the format of {what}: with {sf.shape[-1]} scale '
                           f'factors a row is {rows[0]}, {rows[1]} or {rows[2]}, not {q.dtype} [{row}]')
    if C % 128 != 0 or (C == 0 and not allow_empty):
        raise RuntimeError(f'Assertion failed: {name} needs a contraction length of {what} that is a multiple of 128'
                           + ('' if allow_empty else ', and positive'))
    return q, sf, mx.number, tuple(q.shape[:-1]), C


def _mx_rows(name, what, q, sf):
    """2-D views' checks shared by both functions: unit column stride, rows a multiple of 16 bytes apart."""
    if q.numel() and not (q.stride(-1) == 1 and q.stride(0) % 16 == 0 and q.stride(0) >= q.shape[1] and
                          sf.stride(-1) == 1 and sf.stride(0) >= sf.shape[1]):
        raise RuntimeError(f'Assertion failed: {name} takes {what} as rows of unit column stride whose row stride is a '
                           'multiple of 16 bytes')


def _mx_experts(name, expert_ends, expert_alignment, device, rows=128):
    """rows: the rows of the kernel's tile, which expert_alignment must be a multiple of."""
    import torch
    if not (isinstance(expert_ends, torch.Tensor) and expert_ends.dtype == torch.int32 and expert_ends.dim() == 1 and
            1 <= expert_ends.numel() <= 1024 and expert_ends.is_contiguous()):
        raise RuntimeError(f'Assertion failed: {name} takes expert_ends as a contiguous int32 [E] tensor, 1 <= E <= 1024')
    if not (isinstance(expert_alignment, int) and expert_alignment > 0 and expert_alignment % rows == 0):
        raise RuntimeError(f'Assertion failed: {name} needs expert_alignment % {rows} == 0 (a {rows}-row tile then never '
                           'holds rows of two experts)')
    if expert_ends.device != device:
        raise RuntimeError(f'Assertion failed: {name} takes expert_ends on the device of the operands')


def _grouped_gemm_mx_fprop(name, rows, cols, launch, a, b, expert_ends, expert_alignment, out_dtype):
    """The argument checks, the output and the launch of grouped_gemm_mx / grouped_gemm_mx_decode: a tile of `rows`
    rows, O in multiples of `cols`; launch(kernels, a_format, b_format, ...) calls the kernel's wrapper."""
    import torch
    out_dtype = torch.bfloat16 if out_dtype is None else out_dtype
    aq, asf, afmt, (N,), K = _mx_operand(name, 'a', a, 1)
    bq, bsf, bfmt, (E, O), Kb = _mx_operand(name, 'b', b, 2)
    if K != Kb:
        raise RuntimeError(f'Assertion failed: {name} operands differ along the contraction ({K} and {Kb})')
    if N % rows != 0 or O == 0 or O % cols != 0:
        raise RuntimeError(f'Assertion failed: {name} needs N % {rows} == 0 and O % {cols} == 0, O > 0')
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f'Assertion failed: {name} writes torch.bfloat16 or torch.float32')
    _mx_experts(name, expert_ends, expert_alignment, aq.device, rows=rows)
    if expert_ends.numel() != E or bq.device != aq.device:
        raise RuntimeError(f'Assertion failed: {name} takes b as [E, O, ...] of the E experts of expert_ends, on the '
                           'device of a')
    if not (bq.is_contiguous() and bsf.is_contiguous()):
        raise RuntimeError(f'Assertion failed: {name} takes contiguous weights')
    _mx_rows(name, 'a', aq, asf)
    if not aq.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes tensors on the GPU')
    out = torch.empty((N, O), dtype=out_dtype, device=aq.device)
    if N:
        from .kernels import HipKernels
        launch(HipKernels(), afmt, bfmt, aq, asf, bq.view(E * O, -1), bsf.view(E * O, -1), expert_ends,
               expert_alignment, out)
    return out


def grouped_gemm_mx(a, b, expert_ends, *, expert_alignment: int = 128, out_dtype=None):
    """The experts' GEMM over a dispatch's expanded rows, as one HIP kernel on CDNA4's block-scaled MFMA
    (v_mfma_scale_f32_16x16x128_f8f6f4): fprop, and dgrad when b is the pair of the transposed weights.
    a = (codes, sf) over [N, K]: what dispatch(cast_to_fp8=True, fp8_group_size=32 | cast_to_fp4 | cast_to_fp6,
    do_expand=True, expert_alignment=128) returns, or per_token_cast_to_fp8(group_size=32) / _fp4 / _fp6 of such rows.
    b = (codes, sf) over [E, O, K]: those casts of W.view(E * O, K), viewed back as [E, O, ...]; contiguous.
    A pair is float8_e4m3fn [.., K] (FP8), uint8 or float4_e2m1fn_x2 [.., K / 2] (FP4) or uint8 [.., 3 * K / 4] (FP6)
    with uint8 or float8_e8m0fnu [.., K / 32]; the format is inferred from the scale factors' width, the code dtype and
    a row's bytes, independently for a and b (nine combinations, as the instruction takes them).
    expert_ends int32 [E] on the GPU: expert e owns rows [start_e, expert_ends[e]), start_0 = 0, start_e =
    align_up(expert_ends[e - 1], expert_alignment).  handle.psum_num_recv_tokens_per_expert of a do_expand dispatch is
    exactly this tensor (dispatch_scan writes start + count there for an expanded layout), so it is passed as it is,
    with the handle's expert_alignment.
    -> out [N, O] in out_dtype (torch.bfloat16, the default, or torch.float32): out[n] = A[n] . B[e(n)]^T over the
    dequantised values, accumulated in fp32, one round to nearest even for bf16.  Rows [expert_ends[e], start_{e + 1})
    (alignment padding) are written as zeros; rows at or past the last expert's aligned end -- the tail of a
    worst-case-sized handle -- are not written and not read.
    Needs N % 128 == 0, K % 128 == 0, O % 128 == 0, expert_alignment % 128 == 0; a's rows may be strided (a multiple
    of 16 bytes apart).  Unspecified: NaN codes, an exponent byte 0xff, and an exponent byte 0 under non-zero codes
    (the hardware reads byte 0 as 2^-127, the cast backs as +0.0; the casts never produce it for non-zero data, their
    amax floor of 1e-4 keeps the byte above 100).
    Runs on the current stream, no host synchronisation, no workspace (it captures into a graph); N == 0 returns an
    empty tensor without a launch."""
    return _grouped_gemm_mx_fprop('grouped_gemm_mx', 128, 128, lambda kern, *args: kern.grouped_gemm_mx(False, *args),
                                  a, b, expert_ends, expert_alignment, out_dtype)


def grouped_gemm_mx_decode(a, b, expert_ends, *, expert_alignment: int = 16, out_dtype=None):
    """grouped_gemm_mx for a decoding step -- 1 to 64 tokens an expert -- as a HIP kernel of its own on the same
    instruction, at 16-row granularity: the contract of grouped_gemm_mx, word for word (a = (codes, sf) over [N, K],
    b = (codes, sf) over [E, O, K], formats inferred independently, expert_ends =
    handle.psum_num_recv_tokens_per_expert as it is; alignment-padding rows [expert_ends[e], start_{e + 1}) written as
    zeros, rows at or past the last expert's aligned end neither read nor written; out [N, O] in torch.bfloat16 (the
    default) or torch.float32, accumulated in fp32, one round to nearest even for bf16), with other requirements:
    N % 16 == 0, K % 128 == 0, O % 64 == 0 (O > 0), expert_alignment % 16 == 0 -- what
    dispatch(..., do_expand=True, expert_alignment=16) lays out, and 128-aligned layouts too.
    Which one: grouped_gemm_mx owns 128 x 128 tiles and is built for prefill and training, hundreds of rows an expert;
    below about 64 rows an expert most of such a tile is padding, the time goes into streaming the weights once, and
    this function is the one to call: a workgroup owns 16 rows x 64 columns, its 4 waves split the contraction with
    several steps of loads in flight each, and their partial sums are added in a fixed order (no atomics: the result
    is a function of the inputs alone).  float32 results of the two functions may differ in the last bits, since the
    summation order differs; sums that are exact in fp32 are equal.
    Rows of a inside an expert's aligned range but past its end may hold anything (an output row depends on its own
    row of a only).  Unspecified inputs as in grouped_gemm_mx.  Runs on the current stream, no host synchronisation,
    no workspace (it captures into a graph); N == 0 returns an empty tensor without a launch."""
    return _grouped_gemm_mx_fprop('grouped_gemm_mx_decode', 16, 64, lambda kern, *args: kern.grouped_gemm_mx_decode(*args),
                                  a, b, expert_ends, expert_alignment, out_dtype)


def grouped_gemm_mx_wgrad(dy_t, x_t, expert_ends, *, expert_alignment: int = 128):
    """The experts' weight gradient over a dispatch's expanded rows, the same kernel contracting over TOKENS:
    dy_t = (codes, sf) over [O, N] and x_t = (codes, sf) over [H, N], the outputs of cast_to_mxfp8 / mxfp4 /
    mxfp6_transposed or requant_mxfp8 / mxfp4 / mxfp6_transposed (formats inferred as in grouped_gemm_mx, independent)
    -> float32 [E, O, H]: dW[e] = dY_t[:, seg_e] . X_t[:, seg_e]^T, seg_e = [start_e, align_up(expert_ends[e], 128)),
    with grouped_gemm_mx's expert_ends (handle.psum_num_recv_tokens_per_expert as it is).
    The padding tokens inside a segment, [expert_ends[e], align_up(expert_ends[e], 128)), are part of the contraction
    and must be zero codes: dispatch(do_zero_padding=True) followed by the requantisation gives that (zero rows become
    zero codes with the exponent byte of the 1e-4 floor).  A garbage exponent byte 0xff there is NaN times zero and
    poisons the whole expert; tokens between segments and past the last one are never read.  An expert without rows
    gets zeros.
    Needs O % 128 == 0, H % 128 == 0, N % 128 == 0, expert_alignment % 128 == 0.  Unspecified inputs as in
    grouped_gemm_mx.  Runs on the current stream, no host synchronisation, no workspace (it captures into a graph);
    N == 0 returns zeros without a launch."""
    import torch
    name = 'grouped_gemm_mx_wgrad'
    aq, asf, afmt, (O,), N = _mx_operand(name, 'dy_t', dy_t, 1, allow_empty=True)
    bq, bsf, bfmt, (H,), Nb = _mx_operand(name, 'x_t', x_t, 1, allow_empty=True)
    if N != Nb:
        raise RuntimeError(f'Assertion failed: {name} operands differ along the tokens ({N} and {Nb})')
    if O == 0 or O % 128 != 0 or H == 0 or H % 128 != 0:
        raise RuntimeError(f'Assertion failed: {name} needs O % 128 == 0 and H % 128 == 0, both positive')
    _mx_experts(name, expert_ends, expert_alignment, aq.device)
    if bq.device != aq.device:
        raise RuntimeError(f'Assertion failed: {name} takes both operands on one device')
    _mx_rows(name, 'dy_t', aq, asf)
    _mx_rows(name, 'x_t', bq, bsf)
    if not aq.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes tensors on the GPU')
    E = expert_ends.numel()
    if N == 0:
        return torch.zeros((E, O, H), dtype=torch.float32, device=aq.device)
    out = torch.empty((E, O, H), dtype=torch.float32, device=aq.device)
    from .kernels import HipKernels
    HipKernels().grouped_gemm_mx(True, afmt, bfmt, aq, asf, bq, bsf, expert_ends, expert_alignment, out)
    return out


def route_topk(logits, num_topk: int, *, score_func: str = 'sigmoid', bias=None, num_groups: int = 1,
               num_topk_groups: int = 1, group_score: str = 'top2_sum', norm_topk_prob: bool = True,
               routed_scaling_factor: float = 1.0, return_counts: bool = False):
    """The MoE gate's scoring and group-limited top-k (a DeepSeek-V3 style gate) as one HIP kernel: logits [T, E], the
    output of the gate's linear layer, float32 or bfloat16 on the GPU, become what ElasticBuffer.dispatch takes:
    -> (topk_idx [T, K] deep_ep.topk_idx_t, topk_weights [T, K] float32), with return_counts also counts int32 [E].
    Each logit is read once; there is no [T, E] temporary.  One token a row, all in fp32 on the device:
      1. s[e] = 1 / (1 + exp(-x[e])) for score_func='sigmoid'; for 'softmax' the softmax of the row over all E experts,
         the row maximum subtracted first.
      2. sel[e] = s[e] + bias[e]; bias is None or float32 [E], contiguous: the selection-only correction
         (e_score_correction_bias).
      3. With num_groups > 1 a group is E / num_groups consecutive experts, and its score the sum of its two largest
         sel (group_score='top2_sum') or its largest ('max'); the num_topk_groups groups with the largest scores stay,
         experts of the others cannot be chosen.
      4. The K = num_topk remaining experts with the largest sel are chosen, in descending sel.
      5. An exact tie, at either step, goes to the lower group or expert index: the result is a function of the inputs
         alone.
      6. w[k] = s[idx[k]] (not sel); with norm_topk_prob divided by the sum of the K chosen s; then multiplied by
         routed_scaling_factor.
      7. counts[e] is the number of (t, k) with topk_idx[t, k] == e, exact.
    No index is -1 or repeated in a row.  Logits may be infinite: s(-inf) = 0 under both score functions (an expert
    masked with -inf before a softmax gate), sigmoid(+inf) = 1.  Unspecified: NaN logits or bias, and for 'softmax' a
    row with a +inf logit or without a finite one (torch.softmax gives NaN there).
    8 <= E <= 1024 and E % 8 == 0; unit column stride, rows a multiple of 16 bytes apart; 1 <= num_groups <= 64 with
    E % num_groups == 0; 1 <= num_topk_groups <= num_groups; 'top2_sum' needs at least 2 experts a group;
    1 <= K <= 64 and K <= num_topk_groups * E / num_groups.
    Runs on the current stream, no host synchronisation, no workspace (it captures into a graph); every output is
    contiguous; T == 0 returns empty tensors, and zero counts, without a launch."""
    import torch
    from . import _lib
    name = 'route_topk'
    if not (isinstance(logits, torch.Tensor) and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)):
        raise RuntimeError(f'Assertion failed: {name} takes logits as a 2-D float32 or bfloat16 tensor')
    T, E = logits.shape
    if not (8 <= E <= 1024 and E % 8 == 0):
        raise RuntimeError(f'Assertion failed: {name} needs 8 <= E <= 1024 and E % 8 == 0')
    if score_func not in _lib.ROUTE_SCORE_FUNCS or group_score not in _lib.ROUTE_GROUP_SCORES:
        raise RuntimeError(f'Assertion failed: {name} takes score_func as one of {list(_lib.ROUTE_SCORE_FUNCS)} and '
                           f'group_score as one of {list(_lib.ROUTE_GROUP_SCORES)}')
    if not (isinstance(num_groups, int) and 1 <= num_groups <= 64 and E % num_groups == 0):
        raise RuntimeError(f'Assertion failed: {name} needs 1 <= num_groups <= 64 and E % num_groups == 0')
    if not (isinstance(num_topk_groups, int) and 1 <= num_topk_groups <= num_groups):
        raise RuntimeError(f'Assertion failed: {name} needs 1 <= num_topk_groups <= num_groups')
    if num_groups > 1 and group_score == 'top2_sum' and E // num_groups < 2:
        raise RuntimeError(f"Assertion failed: {name} needs at least 2 experts a group for group_score='top2_sum'")
    if not (isinstance(num_topk, int) and 1 <= num_topk <= 64 and num_topk <= num_topk_groups * (E // num_groups)):
        raise RuntimeError(f'Assertion failed: {name} needs 1 <= num_topk <= 64 and num_topk <= num_topk_groups * E / '
                           'num_groups')
    if T and not (logits.stride(1) == 1 and logits.stride(0) >= E and
                  logits.stride(0) * logits.element_size() % 16 == 0 and logits.data_ptr() % 16 == 0):
        raise RuntimeError(f'Assertion failed: {name} takes rows of unit column stride that start a multiple of 16 '
                           'bytes apart')
    if bias is not None and not (isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and
                                 tuple(bias.shape) == (E,) and bias.is_contiguous() and bias.device == logits.device):
        raise RuntimeError(f'Assertion failed: {name} takes bias as a contiguous float32 [E] tensor on the device of '
                           'the logits')
    if not logits.is_cuda:
        raise RuntimeError(f'Assertion failed: {name} takes a tensor on the GPU')
    topk_idx = torch.empty((T, num_topk), dtype=topk_idx_t, device=logits.device)
    topk_weights = torch.empty((T, num_topk), dtype=torch.float32, device=logits.device)
    counts = None
    if return_counts:
        counts = (torch.empty if T else torch.zeros)((E,), dtype=torch.int32, device=logits.device)
    if T:
        from .kernels import HipKernels
        HipKernels().route_topk(logits, topk_idx, topk_weights, score_func=score_func, bias=bias, num_groups=num_groups,
                                num_topk_groups=num_topk_groups, group_score=group_score,
                                norm_topk_prob=norm_topk_prob, routed_scaling_factor=routed_scaling_factor,
                                counts=counts)
    return (topk_idx, topk_weights, counts) if return_counts else (topk_idx, topk_weights)


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
           'requant_mxfp8_transposed', 'requant_mxfp4_transposed', 'requant_mxfp6_transposed',
           'grouped_gemm_mx', 'grouped_gemm_mx_wgrad', 'grouped_gemm_mx_decode', 'swiglu_cast_to_mx',
           'swiglu_backward_cast_to_mx', 'route_topk']
