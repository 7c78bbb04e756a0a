"""LogFMT-10, fixed length (deepep_amd/csrc/logfmt_codec.h): the stand-in in torch, the plane pack / unpack and the
CPU kernel provider that knows the LogFMT wrappers -- TEST INFRASTRUCTURE ONLY.

The stand-in follows the header's arithmetic in a chosen precision: torch.float32 (the kernels' precision; not bit for
bit theirs, whose log2 / exp2 / reciprocal are the hardware's approximations) or torch.float64 (the yardstick of the
GPU tests).  Everything that is integer arithmetic in the format -- the meta dwords, the degenerate and non-finite
groups, the bit layout -- is exact in both."""
import torch

from tests.fp8_combine_ref import Fp8CombineOracleKernels

GROUP = 128


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """int32 [..] of the 16 bits of a bf16 tensor."""
    assert x.dtype == torch.bfloat16
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xffff


def bits_bf16(bits: torch.Tensor) -> torch.Tensor:
    b = bits.to(torch.int32) & 0xffff
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.bfloat16)


def magnitudes(x: torch.Tensor) -> torch.Tensor:
    """m = bits & 0x7fff, a bf16 denormal as 0."""
    m = bf16_bits(x) & 0x7fff
    return torch.where(m < 0x80, torch.zeros_like(m), m)


def meta_ref(x: torch.Tensor) -> torch.Tensor:
    """int32 [T, H / 128]: amax_bits | amin_bits << 16, the integer maximum and minimum of m."""
    T, H = x.shape
    m = magnitudes(x).view(T, H // GROUP, GROUP)
    return m.amax(dim=2) | (m.amin(dim=2) << 16)


def _mag_float(m: torch.Tensor, dtype) -> torch.Tensor:
    return bits_bf16(m).to(dtype)


def group_params(meta: torch.Tensor, dtype):
    """(li, step, amax bits, exact, nan) per group, as both sides derive them from the meta dword."""
    amax, amin = meta & 0xffff, (meta >> 16) & 0xffff
    nan = amax >= 0x7f80
    exact = nan | (amax == amin)
    safe_max = torch.where(exact, torch.full_like(amax, 0x3f80), amax)       # avoid log2(0 / inf) in unused lanes
    la = torch.log2(_mag_float(safe_max, dtype))
    lmin = torch.log2(_mag_float(torch.where((amin == 0) | exact, torch.full_like(amin, 0x3f80), amin), dtype))
    li = torch.where(amin == 0, la - 32, torch.maximum(lmin, la - 32))
    li = torch.where(exact, la, li)
    step = (la - li) * (1.0 / 510.0) if dtype == torch.float32 else (la - li) / 510.0
    return li, step, amax, exact, nan


def encode_ref(x: torch.Tensor, dtype=torch.float32):
    """(codes int32 [T, H] in 0..511, sign int32 [T, H], meta int32 [T, H / 128]) of bf16 rows x."""
    T, H = x.shape
    assert H % GROUP == 0
    meta = meta_ref(x)
    li, step, _, exact, _ = (p.unsqueeze(2) for p in group_params(meta, dtype))
    m = magnitudes(x).view(T, H // GROUP, GROUP)
    a = _mag_float(torch.where(m == 0, torch.full_like(m, 0x3f80), m), dtype)
    safe_step = torch.where(exact, torch.ones_like(step), step)
    inv = 1.0 / safe_step
    mid = torch.log2(torch.exp2(safe_step) * 0.5 + 0.5)
    rounding = 2.0 - mid * inv
    t = ((torch.log2(a) - li) * inv + rounding).clamp(0.0, 511.0)
    code = torch.floor(t).to(torch.int32)
    code = torch.where(exact.expand_as(m), (m != 0).to(torch.int32), code)
    code = torch.where(m == 0, torch.zeros_like(code), code)
    sign = (bf16_bits(x) >> 15).view(T, H)
    return code.view(T, H), sign, meta


def decode_value(code: torch.Tensor, meta: torch.Tensor, dtype):
    """The decoded magnitudes [T, H] (in dtype, before the sign and the rounding to bf16) and the NaN mask."""
    T, H = code.shape
    li, step, amax, exact, nan = (p.unsqueeze(2) for p in group_params(meta, dtype))
    c = code.view(T, H // GROUP, GROUP)
    v = torch.exp2((c - 1).to(dtype) * step + li)
    v = torch.where(v < 2.0 ** -126, torch.zeros_like(v), v)
    v = torch.where(exact.expand_as(c), _mag_float(amax, dtype).expand_as(v), v)
    v = torch.where(c == 0, torch.zeros_like(v), v)
    return v.view(T, H), nan.expand_as(c).reshape(T, H)


def decode_ref(code: torch.Tensor, sign: torch.Tensor, meta: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """bf16 [T, H]: the decoded value, signed, rounded to nearest even; NaN (0x7fc0) for a non-finite group."""
    v, nan = decode_value(code, meta, dtype)
    out = bf16_bits(v.to(torch.float32).to(torch.bfloat16)) | (sign << 15)
    return bits_bf16(torch.where(nan, torch.full_like(out, 0x7fc0), out))


def pack_planes(code: torch.Tensor, sign: torch.Tensor) -> torch.Tensor:
    """uint8 [T, H + H / 4]: [low | high], column c in bits 2 * (c & 3) of high byte c / 4."""
    T, H = code.shape
    low = (code & 0xff).to(torch.uint8)
    two = ((sign << 1) | (code >> 8)).view(T, H // 4, 4)
    high = (two[:, :, 0] | two[:, :, 1] << 2 | two[:, :, 2] << 4 | two[:, :, 3] << 6).to(torch.uint8)
    return torch.cat([low, high], dim=1)


def unpack_planes(planes: torch.Tensor):
    """(codes, sign) int32 [T, H] of uint8 [T, H + H / 4]."""
    T, W = planes.shape
    H = W * 4 // 5
    low = planes[:, :H].to(torch.int32)
    high = planes[:, H:].to(torch.int32)
    two = torch.stack([(high >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(T, H)
    return low | (two & 1) << 8, two >> 1


def cast_ref(x: torch.Tensor, dtype=torch.float32):
    """(planes uint8 [T, H * 5 / 4], meta int32 [T, H / 128]) of bf16 rows, on the CPU."""
    code, sign, meta = encode_ref(x.cpu().contiguous(), dtype)
    return pack_planes(code, sign), meta


def cast_back_ref(planes: torch.Tensor, meta: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    if planes.shape[0] == 0:
        return torch.empty((0, planes.shape[1] * 4 // 5), dtype=torch.bfloat16)
    code, sign = unpack_planes(planes.cpu().contiguous())
    return decode_ref(code, sign, meta.cpu().contiguous(), dtype)


def logfmt_row_bytes(H: int) -> int:
    """The reference test's count (tests/legacy/test_low_latency.py:219): 10 bits an element, 4 bytes a group."""
    return H * 10 // 8 + H // 128 * 4


def calc_diff(x: torch.Tensor, y: torch.Tensor) -> float:
    """The reference's calc_diff (deep_ep/utils/testing)."""
    x, y = x.double() + 1, y.double() + 1
    denominator = (x * x + y * y).sum()
    return float(1 - 2 * (x * y).sum() / denominator)


class LogfmtOracleKernels(Fp8CombineOracleKernels):
    """The CPU provider with the LogFMT wrappers of deepep_amd.kernels.HipKernels (the fp32 stand-in); it asserts
    what the HIP wrappers require of their arguments."""
    name = 'oracle-logfmt'

    def cast_logfmt(self, x, planes, meta, stream=None):
        T, H = x.shape
        assert x.dtype == torch.bfloat16 and H % 128 == 0
        assert planes.dtype == torch.uint8 and planes.is_contiguous() and tuple(planes.shape) == (T, H * 5 // 4)
        assert meta.dtype == torch.int32 and meta.is_contiguous() and tuple(meta.shape) == (T, H // 128)
        p, m = cast_ref(x)
        planes.copy_(p)
        meta.copy_(m)

    def cast_back_logfmt(self, planes, meta, out, stream=None):
        M, H = out.shape
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and H % 128 == 0
        assert planes.dtype == torch.uint8 and tuple(planes.shape) == (M, H * 5 // 4)
        assert meta.dtype == torch.int32 and tuple(meta.shape) == (M, H // 128)
        out.copy_(cast_back_ref(planes, meta))

    def logfmt_pack_rows(self, src, num_rows, hidden, dst, src_tail_offset=0, dst_tail_offset=0, tail_bytes=0,
                         stream=None):
        assert src.dim() == 2 and dst.dim() == 2 and src.is_contiguous() and dst.is_contiguous()
        assert src.shape[0] >= num_rows and dst.shape[0] >= num_rows and hidden % 128 == 0
        s = src.view(torch.uint8).view(src.shape[0], -1)
        d = dst.view(torch.uint8).view(dst.shape[0], -1)
        coded = hidden * 5 // 4
        assert s.shape[1] % 16 == 0 and d.shape[1] % 16 == 0 and tail_bytes % 16 == 0
        if tail_bytes:
            assert src_tail_offset >= hidden * 2 and src_tail_offset + tail_bytes <= s.shape[1]
            assert dst_tail_offset >= coded + hidden // 32 and dst_tail_offset + tail_bytes <= d.shape[1]
        if num_rows == 0:
            return
        x = s[:num_rows, :hidden * 2].contiguous().view(torch.bfloat16)
        p, m = cast_ref(x)
        d[:num_rows, :coded] = p
        d[:num_rows, coded:coded + hidden // 32] = m.view(torch.uint8).view(num_rows, hidden // 32)
        if tail_bytes:
            d[:num_rows, dst_tail_offset:dst_tail_offset + tail_bytes] = \
                s[:num_rows, src_tail_offset:src_tail_offset + tail_bytes]

    def combine_reduce(self, mode, src, out, num_units, *args, src_logfmt_meta=None, **kw):
        if src_logfmt_meta is None:
            return super().combine_reduce(mode, src, out, num_units, *args, **kw)
        from deepep_amd.kernels import MODE_EPILOGUE
        H = out.shape[1]
        M = src.shape[0]
        assert mode == MODE_EPILOGUE and 'src_sf' not in kw
        assert src.dtype == torch.uint8 and src.dim() == 2 and src.shape[1] == H * 5 // 4 and H % 128 == 0
        assert M == 0 or (src.stride(1) == 1 and src.stride(0) % 16 == 0)
        assert src_logfmt_meta.dtype == torch.int32 and tuple(src_logfmt_meta.shape) == (M, H // 128)
        rows = cast_back_ref(src, src_logfmt_meta)
        return super().combine_reduce(mode, rows, out, num_units, *args, **kw)
