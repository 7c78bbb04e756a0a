// fp4_cast_common.h -- what the e2m1 casting kernels of fp4_cast.hip (groups along hidden) and fp46_cast_t.hip (the
// transposed MXFP4 cast: groups along the token axis) share: the scale rule with 6, the e2m1 conversion and a lane's
// cast of a group of columns.  One definition, so the two axes cannot drift.
#pragma once

#include "cast_common.h"
#include "fp8_dequant.h"

namespace {

// the largest e2m1 magnitude, and the fp32 reciprocal the scale rule multiplies by
constexpr float kFp4Max = 6.0f, kFp4MaxRcp = 1.0f / kFp4Max;

// 8 consecutive elements (one 16-byte vector of bf16) as 8 codes in a dword, element j in bits 4j + 3 : 4j, by
// v_cvt_scalef32_pk_fp4_bf16: two bf16 of a dword divided by the power of two sf = 2^e and rounded to e2m1, written to
// byte j of the result.  The scaled magnitude is in [0, 6] (the ceiling rule keeps a group's amax in (3, 6]).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// (Each dword passes through an empty asm first: handed the elements of one 16-byte vector directly, the compiler
// selected the vector's first dword as the source of all four conversions.)
__device__ __forceinline__ uint32_t cvt8_fp4(const u32x4& raw, float sf) {
    uint32_t d[4] = {raw[0], raw[1], raw[2], raw[3]};
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(d[j]));
    out = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(out, __builtin_bit_cast(bf16x2, d[0]), sf, 0);
    out = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(out, __builtin_bit_cast(bf16x2, d[1]), sf, 1);
    out = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(out, __builtin_bit_cast(bf16x2, d[2]), sf, 2);
    out = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(out, __builtin_bit_cast(bf16x2, d[3]), sf, 3);
    return out;
}

// the group's exponent byte from its amax (at least 1e-4f): the ceiling rule, 112..253 for finite bf16
__device__ __forceinline__ uint32_t fp4_exp_byte(float amax) {
    const uint32_t bits = __float_as_uint(amax * kFp4MaxRcp);
    return ((bits >> 23) & 0xffu) + ((bits & 0x7fffffu) != 0);
}

// what a lane holds after the cast of its kVecs 16-byte loads
template <int kVecs>
struct Fp4Lane {
    typedef uint32_t q_t __attribute__((ext_vector_type(kVecs)));
    q_t q;              // this lane's 8 * kVecs codes, 4 * kVecs bytes
    uint32_t byte;      // the group's exponent byte (the same in every lane of the group)
};

// raw: the lane's kVecs 16-byte loads, 8 * kVecs consecutive bf16 (zeros in a lane past the row: it must still run
// the cross-lane steps); a group of 32 columns is 32 / (8 * kVecs) lanes: a quad of 8 columns, two of 16 columns, or
// the lane itself
template <int kVecs>
__device__ __forceinline__ Fp4Lane<kVecs> cast_group_fp4(const u32x4* raw) {
    static_assert(kVecs == 1 || kVecs == 2 || kVecs == 4, "a lane holds 8, 16 or 32 columns");
    u16x2 m = {0, 0};
#pragma unroll
    for (int j = 0; j < kVecs; ++j) m = amax8(m, raw[j]);
    float amax = amax_floor(m[0] > m[1] ? m[0] : m[1]);
    if constexpr (kVecs < 4) amax = group_max<4 / kVecs>(amax);
    Fp4Lane<kVecs> out;
    out.byte = fp4_exp_byte(amax);
    const float sf = deepep::ue8m0_factor(out.byte);                     // 2^e
#pragma unroll
    for (int j = 0; j < kVecs; ++j) out.q[j] = cvt8_fp4(raw[j], sf);
    return out;
}

}  // namespace
