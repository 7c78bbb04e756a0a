// fp8_dequant.h -- the device arithmetic of the FP8 cast back, shared by the kernel that writes the bf16 rows
// (cast_back_fp8_kernel, fp8_cast.hip) and the combine that reduces FP8 expert rows without writing them
// (combine_rows_kernel with an FP8 source, combine.hip).  One definition, so the two cannot drift:
//   bf16 = bf16_rne(fp32(e4m3fn) * sf)      e4m3fn -> fp32 is exact (v_cvt_pk_f32_fp8), one fp32 multiply by the
//                                           group's scale factor, one round-to-nearest-even (v_cvt_pk_bf16_f32)
//   sf   = float_from_bits(byte << 23)      for a packed UE8M0 exponent byte (byte 0: +0.0f)
// Reference: per_token_cast_back, deep_ep/utils/math.py:42-56.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace deepep {

typedef uint32_t dq_u32x4 __attribute__((ext_vector_type(4)));
typedef float dq_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 dq_bf16x2 __attribute__((ext_vector_type(2)));

// the scale factor 2^(byte - 127) of a UE8M0 exponent byte
__device__ __forceinline__ float ue8m0_factor(uint32_t byte) { return __uint_as_float(byte << 23); }

// 4 consecutive e4m3fn bytes (one dword) times ss = {s, s}, as 4 bf16 in two dwords
__device__ __forceinline__ void dequant4(uint32_t raw, const dq_f32x2& ss, uint32_t& lo, uint32_t& hi) {
    const dq_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw), false);
    const dq_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(raw), true);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(a * ss, dq_bf16x2));
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(b * ss, dq_bf16x2));
}

// 8 consecutive e4m3fn bytes times the group's scale factor s, as 8 bf16
__device__ __forceinline__ dq_u32x4 dequant8(uint32_t raw0, uint32_t raw1, float s) {
    const dq_f32x2 ss = {s, s};
    uint32_t r[4];
    dequant4(raw0, ss, r[0], r[1]);
    dequant4(raw1, ss, r[2], r[3]);
    return dq_u32x4{r[0], r[1], r[2], r[3]};
}

// 16 consecutive e4m3fn bytes times the group's scale factor s, as 16 bf16: columns 0-7 in lo, 8-15 in hi
__device__ __forceinline__ void dequant16(const dq_u32x4& raw, float s, dq_u32x4& lo, dq_u32x4& hi) {
    lo = dequant8(raw[0], raw[1], s);
    hi = dequant8(raw[2], raw[3], s);
}

}  // namespace deepep
