// fp4_dequant.h -- the device arithmetic of the MXFP4 cast back, shared by the kernel that writes the bf16 rows
// (cast_back_fp4_kernel, fp4_cast.hip) and the requantisation along the tokens that never writes them
// (requant_mx_t_kernel, requant_t.hip).  One definition, so the two cannot drift:
//   bf16 = bf16_rne(fp32(e2m1) * sf)        e2m1 -> fp32 is exact (v_cvt_scalef32_pk_f32_fp4 with the scale 1.0f), one
//                                           fp32 multiply by the group's factor, one round-to-nearest-even
//   sf   = float_from_bits(byte << 23)      the group's UE8M0 exponent byte (ue8m0_factor; byte 0: +0.0f)
#pragma once

#include "fp8_dequant.h"

namespace deepep {

// 8 codes (one dword) times the group's factor s, as 8 bf16: v_cvt_scalef32_pk_f32_fp4 with the scale 1.0f gives the
// two codes of byte j as fp32, exactly; then one fp32 multiply by s and one round-to-nearest-even each, as the FP8
// cast back (the factor is applied here, not by the conversion: byte 0 is +0.0f and gives signed zeros)
__device__ __forceinline__ dq_u32x4 dequant8_fp4(uint32_t raw, float s) {
    const dq_f32x2 ss = {s, s};
    const dq_f32x2 v[4] = {__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 0),
                           __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 1),
                           __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 2),
                           __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw, 1.0f, 3)};
    dq_u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        r[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v[j] * ss, dq_bf16x2));
    return r;
}

}  // namespace deepep
