// logfmt_codec.h -- the device arithmetic of "LogFMT-10, fixed length", shared by the codec kernels (logfmt.hip) and
// the combine that reduces LogFMT rows without writing their bf16 form (combine_item_logfmt, combine.hip).  One
// definition, so the two cannot drift.
//
// The format is the reference's LogFMT-10 (csrc/kernels/legacy/internode_ll.cu:557-638 encode, :672-712 decode): per
// group of 128 columns a pair (amax, amin) of bf16 magnitudes and, per element, a sign and a 9-bit code on a
// logarithmic grid between them.  Three departures from the reference, all deliberate:
//   1. Every group is encoded.  The reference sends a group as bf16 when amax >= 1 or amin == amax
//      (internode_ll.cu:605); rows of varying length do not fit an all-to-all of equal-sized rows, and a logarithmic
//      grid is scale-invariant, so the fall-back buys no precision.
//   2. Degenerate and non-finite groups are exact.  With m = bits & 0x7fff (a magnitude below 2^-126, a bf16
//      denormal, counts as 0 everywhere: v_log_f32 does not take denormals), amax and amin are the *integer* maximum
//      and minimum of m over the group, which keeps the order and never drops a NaN.  amax >= 0x7f80 (Inf or NaN in
//      the group): every element decodes to NaN.  amax == amin (all-zero included): code = (m != 0), and a nonzero
//      code decodes to amax exactly.
//   3. A decoded value is rounded to bf16 (round to nearest even) before it enters a reduction -- the rule of the
//      FP8 source (fp8_dequant.h) -- so a combine over LogFMT rows is bit for bit the bf16 combine over the rows
//      deepep_cast_back_logfmt writes.
// Otherwise, in fp32, with a = the magnitude as a float:
//   la = log2(amax)     li = max(log2(amin), la - 32), la - 32 when amin == 0
//   step = (la - li) / 510     inv = 1 / step     rounding = 2 - log2((1 + exp2(step)) * 0.5) * inv
//   code = min(floor(max((log2(a) - li) * inv + rounding, 0)), 511), 0 for a == 0
//          (the reference's log2(a) * inv + rounding - li * inv with the difference taken first: it is exact for
//           neighbouring logarithms, where the two products cancel to a few bits in a narrow group)
//   decode: code 0 -> 0, else exp2((code - 1) * step + li), a result below 2^-126 is 0; then the sign
// log2 / exp2 are v_log_f32 / v_exp_f32, 1 / step is v_rcp_f32 and / 510 a multiply by 1.0f / 510; every multiply-add
// is an explicit fma, so the code does not depend on what the compiler contracts.  The decoder recomputes la, li and
// step from the stored pair (as logfmt_check_amaxmin does): the meta dword is all both sides share.
//
// Bit layout (this build's own, for 8 columns per lane): a row of H columns, H % 128 == 0, is three planes
//   low   H bytes        code & 0xff of every column
//   high  H / 4 bytes    two bits per column, (sign << 1) | (code >> 8), column c in bits 2 * (c & 3) of byte c / 4
//   meta  H / 128 dwords amax_bits | amin_bits << 16 per group
// so a lane's 8 columns are one 8-byte load from the low plane and one 2-byte load from the high plane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace deepep {

typedef uint32_t lf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lf_u32x2 __attribute__((ext_vector_type(2)));
typedef float lf_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 lf_bf16x2 __attribute__((ext_vector_type(2)));

// the magnitude bits of a bf16, a denormal as 0
__device__ __forceinline__ uint32_t lf_magnitude(uint32_t bits) {
    const uint32_t m = bits & 0x7fffu;
    return m < 0x0080u ? 0u : m;
}

// What both sides derive from a group's meta dword.
struct LfGroup {
    float li, step;
    uint32_t amax;       // bf16 bits
    bool exact;          // amax == amin or a non-finite group: code = (m != 0)
    bool nan;            // Inf or NaN in the group: decodes to NaN
};

__device__ __forceinline__ LfGroup lf_group(uint32_t meta) {
    LfGroup g;
    g.amax = meta & 0xffffu;
    const uint32_t amin = meta >> 16;
    const float la = __builtin_amdgcn_logf(__uint_as_float(g.amax << 16));
    const float floor_li = la - 32.0f;
    g.li = amin == 0u ? floor_li : fmaxf(__builtin_amdgcn_logf(__uint_as_float(amin << 16)), floor_li);
    g.step = (la - g.li) * (1.0f / 510.0f);
    g.nan = g.amax >= 0x7f80u;
    g.exact = g.nan || g.amax == amin;
    return g;
}

// The encoder's two per-group constants: code = floor(max(fma(log2(a) - li, inv, rounding), 0))
__device__ __forceinline__ void lf_encode_constants(const LfGroup& g, float& inv, float& rounding) {
    inv = __builtin_amdgcn_rcpf(g.step);
    const float mid = __builtin_amdgcn_logf(__builtin_fmaf(__builtin_amdgcn_exp2f(g.step), 0.5f, 0.5f));
    rounding = __builtin_fmaf(-mid, inv, 2.0f);
}

__device__ __forceinline__ uint32_t lf_encode1(uint32_t m, const LfGroup& g, float inv, float rounding) {
    if (g.exact) return m != 0u ? 1u : 0u;
    const float la = __builtin_amdgcn_logf(__uint_as_float(m << 16));
    const float t = fminf(fmaxf(__builtin_fmaf(la - g.li, inv, rounding), 0.0f), 511.0f);
    return m == 0u ? 0u : static_cast<uint32_t>(t);      // t >= 0: the conversion truncates = floor
}

// 8 consecutive bf16 (one 16-byte vector) of a group as 8 low bytes and 16 high-plane bits
__device__ __forceinline__ void lf_encode8(const lf_u32x4& raw, const LfGroup& g, lf_u32x2& low, uint32_t& high) {
    float inv, rounding;
    lf_encode_constants(g, inv, rounding);
    uint32_t lo[2] = {0u, 0u};
    high = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t bits = (raw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        const uint32_t code = lf_encode1(lf_magnitude(bits), g, inv, rounding);
        lo[j >> 2] |= (code & 0xffu) << (8 * (j & 3));
        high |= ((bits >> 15) << 1 | code >> 8) << (2 * j);
    }
    low = lf_u32x2{lo[0], lo[1]};
}

// column j's 9-bit code out of a lane's 8 low bytes and 16 high-plane bits
__device__ __forceinline__ uint32_t lf_code(uint32_t low0, uint32_t low1, uint32_t high, int j) {
    return (((j < 4 ? low0 : low1) >> (8 * (j & 3))) & 0xffu) | ((high >> (2 * j)) & 1u) << 8;
}

// 8 consecutive columns (8 low bytes, 16 high-plane bits) as 8 bf16: the decoded value, signed, rounded to nearest even.
// What only rare groups need -- amax for an exact group, the flush of a value below 2^-126, which takes li < -126 --
// sits behind a wave-uniform branch, so a wave without such a group pays for none of those selects.
__device__ __forceinline__ lf_u32x4 lf_decode8(uint32_t low0, uint32_t low1, uint32_t high, uint32_t meta) {
    const LfGroup g = lf_group(meta);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t code = lf_code(low0, low1, high, j);
        const float v = __builtin_amdgcn_exp2f(__builtin_fmaf(static_cast<float>(static_cast<int>(code) - 1), g.step, g.li));
        f[j] = code == 0u ? 0.0f : v;
    }
    const bool rare = g.exact || g.li < -126.0f;
    if (__builtin_amdgcn_ballot_w64(rare) != 0ull) {
        const float amax = __uint_as_float(g.amax << 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = g.exact ? amax : (f[j] < 0x1p-126f ? 0.0f : f[j]);
            f[j] = lf_code(low0, low1, high, j) == 0u ? 0.0f : r;
        }
    }
    lf_u32x4 out;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        // column j's sign is bit 2 * j + 1 of the high-plane bits: moved to bit 31
        const uint32_t s0 = (high << (30 - 4 * d)) & 0x80000000u, s1 = (high << (28 - 4 * d)) & 0x80000000u;
        const lf_f32x2 pair = {__uint_as_float(__float_as_uint(f[2 * d]) | s0),
                               __uint_as_float(__float_as_uint(f[2 * d + 1]) | s1)};
        out[d] = __builtin_bit_cast(uint32_t, __builtin_convertvector(pair, lf_bf16x2));
        if (g.nan) out[d] = 0x7fc07fc0u;
    }
    return out;
}

}  // namespace deepep
