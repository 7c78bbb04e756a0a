// grouped_gemm_mx_common.h -- what the experts' GEMMs of grouped_gemm_mx.hip (128 x 128 tiles) and
// grouped_gemm_mx_decode.hip (16 x 64 tiles) share: an MX operand (codes and exponent bytes), its load into the
// registers of v_mfma_scale_f32_16x16x128_f8f6f4 (the layouts: the comment at the top of grouped_gemm_mx.hip and
// DESIGN.md section 3), the store of four results, the launchers' checks of an operand and the dispatch over the
// formats.  One definition, so the two schedules cannot drift.  The schedules themselves and the expert lookups (64-bit
// there, 32-bit with a clamp for negative ends in the decode kernel) stay in their files.
#pragma once

#include <type_traits>

#include "cast_common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxExperts = 1024;

// the bytes of 32 codes; the format's number is the instruction's own (cbsz / blgp)
__host__ __device__ constexpr int block_bytes(int fmt) {
    return fmt == DEEPEP_MX_FP8 ? 32 : fmt == DEEPEP_MX_FP6 ? 24 : 16;
}

// where the codes of lane group kb start inside a step's bytes of a row
__host__ __device__ constexpr int lane_bytes(int fmt, int kb) { return fmt == DEEPEP_MX_FP6 ? 24 * kb : 16 * kb; }

// a lane's 32 codes as the instruction's operand; p: the step's bytes of the row + lane_bytes (FP8, FP4: 16-byte
// aligned; FP6: 8-byte aligned)
template <int kFmt>
__device__ __forceinline__ i32x8 load_codes(const uint8_t* p) {
    if constexpr (kFmt == DEEPEP_MX_FP8) {
        const u32x4 lo = *reinterpret_cast<const u32x4*>(p), hi = *reinterpret_cast<const u32x4*>(p + 64);
        return i32x8{int(lo[0]), int(lo[1]), int(lo[2]), int(lo[3]), int(hi[0]), int(hi[1]), int(hi[2]), int(hi[3])};
    } else if constexpr (kFmt == DEEPEP_MX_FP6) {
        const u32x2 v0 = *reinterpret_cast<const u32x2*>(p), v1 = *reinterpret_cast<const u32x2*>(p + 8),
                    v2 = *reinterpret_cast<const u32x2*>(p + 16);
        return i32x8{int(v0[0]), int(v0[1]), int(v1[0]), int(v1[1]), int(v2[0]), int(v2[1]), 0, 0};
    } else {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
        return i32x8{int(v[0]), int(v[1]), int(v[2]), int(v[3]), 0, 0, 0, 0};
    }
}

struct Operand {
    const uint8_t* __restrict__ q;                         // codes, rows q_stride bytes apart
    const uint8_t* __restrict__ sf;                        // exponent bytes, rows sf_stride bytes apart
    int64_t q_stride, sf_stride;
};

// a lane's four consecutive results: 16 bytes of fp32, or 8 of bf16 (one round to nearest even)
template <bool kF32>
__device__ __forceinline__ void store4(uint8_t* dst, const f32x4& v) {
    if constexpr (kF32) {
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v[0], v[1]}, bf16x2));
        const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v[2], v[3]}, bf16x2));
        *reinterpret_cast<u32x2*>(dst) = u32x2{lo, hi};
    }
}

bool is_format(int f) { return f == DEEPEP_MX_FP8 || f == DEEPEP_MX_FP6 || f == DEEPEP_MX_FP4; }

// what an operand of `k` elements along the contraction must satisfy
const char* operand_fault(const void* q, int64_t q_stride, const uint8_t* sf, int64_t sf_stride, int format, int64_t k) {
    if (q == nullptr || sf == nullptr || !a16(q)) return "null or misaligned pointers (16-byte aligned codes)";
    if (q_stride < k / 32 * block_bytes(format) || q_stride % 16 != 0)
        return "row stride below a row's bytes or not 16-byte aligned";
    if (sf_stride < k / 32) return "scale-factor row stride below a row's bytes";
    if (q_stride > (1 << 24) || sf_stride > (1 << 24)) return "row stride above 2^24";
    return nullptr;
}

// f(the format as an integral constant), for a format is_format accepts
template <typename F>
void with_format(int format, F f) {
    if (format == DEEPEP_MX_FP8) f(std::integral_constant<int, DEEPEP_MX_FP8>{});
    else if (format == DEEPEP_MX_FP6) f(std::integral_constant<int, DEEPEP_MX_FP6>{});
    else f(std::integral_constant<int, DEEPEP_MX_FP4>{});
}

// launch(a, b, f32) with the operands' formats and the output's type as integral constants: the caller names its
// kernel<decltype(a)::value, decltype(b)::value, decltype(f32)::value> there, one of the 3 x 3 x 2
template <typename Launch>
void for_formats(int a_format, int b_format, bool f32, Launch launch) {
    with_format(a_format, [&](auto a) {
        with_format(b_format, [&](auto b) {
            if (f32) launch(a, b, std::true_type{});
            else launch(a, b, std::false_type{});
        });
    });
}

}  // namespace
