// fp6_cast_common.h -- what the e2m3 casting kernels of fp6_cast.hip (groups along hidden) and fp46_cast_t.hip (the
// transposed MXFP6 cast: groups along the token axis) share: the scale rule with 7.5, the e2m3 conversion and a lane's
// cast of a group of columns.  One definition, so the two axes cannot drift.
#pragma once

#include "cast_common.h"
#include "fp8_dequant.h"

namespace {

typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));

constexpr int kGroupBytes = 24;                          // 32 codes of 6 bits

// the largest e2m3 magnitude, and the fp32 reciprocal the scale rule multiplies by
constexpr float kFp6Max = 7.5f, kFp6MaxRcp = 1.0f / kFp6Max;

// the group's exponent byte from its amax (at least 1e-4f): the ceiling rule, 111..253 for finite bf16
__device__ __forceinline__ uint32_t fp6_exp_byte(float amax) {
    const uint32_t bits = __float_as_uint(amax * kFp6MaxRcp);
    return ((bits >> 23) & 0xffu) + ((bits & 0x7fffffu) != 0);
}

// 32 bf16 in 16 dwords (element 2j in the low half of dword j) divided by the power of two sf = 2^e and rounded to
// e2m3 by v_cvt_scalef32_pk32_fp6_bf16: the 32 codes dense in 6 dwords, element r in bits 6r + 5 : 6r.  The scaled
// magnitude is in [0, 7.5] (the ceiling rule keeps a group's amax in (3.75, 7.5]).
__device__ __forceinline__ u32x6 cvt32_fp6(const u32x16& v, float sf) {
    return __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, v), sf);
}

// what a lane holds after the cast of its group
struct Fp6Lane {
    u32x6 q;            // the group's 32 codes, column c in bits 6c + 5 : 6c
    uint32_t byte;      // the group's exponent byte
};

// raw: the lane's kVecs 16-byte loads (zeros in a lane past the row: it must still run the cross-lane steps).  Four:
// 32 consecutive bf16 = one group.  One: 8 consecutive bf16, a quarter of the group its quad of lanes holds; the
// lane's 8 codes are the low 48 bits of q (the conversion's other sources are zeros, whose codes are zero).
template <int kVecs = 4>
__device__ __forceinline__ Fp6Lane cast_group_fp6(const u32x4* raw) {
    static_assert(kVecs == 1 || kVecs == 4, "a lane holds 8 or 32 columns");
    u16x2 m = {0, 0};
#pragma unroll
    for (int j = 0; j < kVecs; ++j) m = amax8(m, raw[j]);
    float amax = amax_floor(m[0] > m[1] ? m[0] : m[1]);
    if constexpr (kVecs == 1) amax = group_max<4>(amax);
    Fp6Lane out;
    out.byte = fp6_exp_byte(amax);
    const float sf = deepep::ue8m0_factor(out.byte);                     // 2^e
    u32x16 v = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * j + k] = raw[j][k];
    }
    out.q = cvt32_fp6(v, sf);
    return out;
}

}  // namespace
