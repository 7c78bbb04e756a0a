// fp6_dequant.h -- the device arithmetic of the MXFP6 cast back, shared by the kernel that writes the bf16 rows
// (cast_back_fp6_kernel, fp6_cast.hip) and the requantisation along the tokens that never writes them
// (requant_mx_t_kernel, requant_t.hip).  One definition, so the two cannot drift:
//   bf16 = bf16_rne(fp32(e2m3) * sf)        e2m3 -> fp32 is exact (v_cvt_scalef32_pk32_f32_fp6 with the scale 1.0f),
//                                           one fp32 multiply by the group's factor, one round-to-nearest-even
//   sf   = float_from_bits(byte << 23)      the group's UE8M0 exponent byte (ue8m0_factor; byte 0: +0.0f)
#pragma once

#include "fp8_dequant.h"

namespace deepep {

typedef uint32_t dq_u32x6 __attribute__((ext_vector_type(6)));
typedef float dq_f32x32 __attribute__((ext_vector_type(32)));

// a group's 24 bytes times its factor s, as 32 bf16 in four 16-byte vectors: v_cvt_scalef32_pk32_f32_fp6 with the
// scale 1.0f gives the 32 codes as fp32, exactly; then one fp32 multiply by s and one round-to-nearest-even each, as
// the FP8 cast back (the factor is applied here, not by the conversion: byte 0 is +0.0f and gives signed zeros)
__device__ __forceinline__ void dequant32_fp6(const dq_u32x6& raw, float s, dq_u32x4* out) {
    const dq_f32x32 v = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(raw, 1.0f);
    const dq_f32x2 ss = {s, s};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const dq_f32x2 p = {v[8 * j + 2 * k], v[8 * j + 2 * k + 1]};
            out[j][k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(p * ss, dq_bf16x2));
        }
    }
}

}  // namespace deepep
