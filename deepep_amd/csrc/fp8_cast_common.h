// fp8_cast_common.h -- what the e4m3fn casting kernels of fp8_cast.hip (groups along hidden) and fp8_cast_t.hip (the
// transposed MXFP8 cast: groups along the token axis) share: the scale rule, the e4m3fn conversion, a lane's cast of a
// group of columns and the scale-factor formats.  One definition, so the two axes cannot drift.
#pragma once

#include "cast_common.h"
#include "fp8_dequant.h"

namespace {

// ---------------------------------------------------------------- the cast (per token, per group of columns)
// The per-token cast in front of an FP8 dispatch (reference: per_token_cast_to_fp8, deep_ep/utils/math.py:30-39;
// fused into the send kernel by the legacy low-latency path, csrc/kernels/legacy/internode_ll.cu:220-245 with
// calculate_fp8_scales, csrc/kernels/legacy/utils.cuh:494-503).  A lane holds 8 or 16 consecutive bf16 (one or two
// 16-byte loads), the lanes of a group of columns (128; MXFP8: 32) find its amax by a butterfly, and the lane's
// OCP e4m3fn bytes leave in one store.  Bitwise contract, per group:
//   round_scale == 0: amax = max(max|x|, 1e-4f); sf = amax / 448.0f; q = e4m3fn_rne(fp32(x) * ((1.0f / amax) * 448.0f))
//                     (torch evaluates the reference's `448.0 / amax` as reciprocal(amax) * 448: two roundings)
//   round_scale != 0: v = amax * fp32(1 / 448); e = exponent(v) + (mantissa(v) != 0); sf = 2^e;
//                     q = e4m3fn_rne(fp32(x) * 2^-e)
// -- true fp32 divisions, one fp32 multiply and one round-to-nearest-even conversion per element.  Inputs are
// finite bf16 (NaN / Inf: unspecified).

// what a lane holds after the cast of its kVecs 16-byte loads
template <int kVecs>
struct Fp8Lane {
    typedef uint32_t q_t __attribute__((ext_vector_type(2 * kVecs)));
    q_t q;          // this lane's 8 * kVecs e4m3fn bytes
    float sf;       // the group's scale factor (the same in every lane of the group)
};

// the group's two factors from its amax (the contract above): q = e4m3fn_rne(x * scale), sf is what is stored
__device__ __forceinline__ void group_scales(float amax, int round_scale, float& scale, float& sf) {
    if (round_scale) {
        const uint32_t bits = __float_as_uint(amax * (1.0f / 448.0f));
        const int e = static_cast<int>((bits >> 23) & 0xffu) - 127 + ((bits & 0x7fffffu) != 0);
        sf = __uint_as_float(static_cast<uint32_t>(e + 127) << 23);
        scale = __uint_as_float(static_cast<uint32_t>(127 - e) << 23);
    } else {
        sf = amax / 448.0f;
        scale = (1.0f / amax) * 448.0f;                  // not 448.0f / amax: see above
    }
}

// 8 scaled values as 8 e4m3fn bytes (one round-to-nearest-even conversion each)
// (the products as pairs: one packed fp32 multiply for two values, each the same IEEE product)
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32x2 cvt8(const float* f, float scale) {
    const f32x2 s = {scale, scale};
    const f32x2 p0 = f32x2{f[0], f[1]} * s, p1 = f32x2{f[2], f[3]} * s;
    const f32x2 p2 = f32x2{f[4], f[5]} * s, p3 = f32x2{f[6], f[7]} * s;
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(p0[0], p0[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(p1[0], p1[1], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(p2[0], p2[1], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(p3[0], p3[1], hi, true);
    return u32x2{static_cast<uint32_t>(lo), static_cast<uint32_t>(hi)};
}

// raw: the lane's kVecs 16-byte loads, 8 * kVecs consecutive bf16 (zeros in a lane past the row: it must still run
// the butterfly); kGroupCols: the columns that share a scale factor
template <int kVecs, int kGroupCols>
__device__ __forceinline__ Fp8Lane<kVecs> cast_group_fp8(const u32x4* raw, int round_scale) {
    float f[8 * kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) unpack8(raw[j], f + 8 * j);
    float amax = 1e-4f;
#pragma unroll
    for (int j = 0; j < 8 * kVecs; ++j) amax = fmaxf(amax, fabsf(f[j]));
    amax = group_max<kGroupCols / (8 * kVecs)>(amax);
    float scale;
    Fp8Lane<kVecs> out;
    group_scales(amax, round_scale, scale, out.sf);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const u32x2 h = cvt8(f + 8 * j, scale);
        out.q[2 * j] = h[0];
        out.q[2 * j + 1] = h[1];
    }
    return out;
}

// the value held by the first lane of every 8 lanes (the other lanes hold zero bits), in all 8
template <typename T>
__device__ __forceinline__ T share8(T v) {
    const int q = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), kDppQuadFirst, 0xf, 0xf, true);
    const int m = __builtin_amdgcn_mov_dpp(q, kDppHalfMirror, 0xf, 0xf, true);
    return __builtin_bit_cast(T, q | m);                       // lanes 0-3: value | 0, lanes 4-7: 0 | value
}

// ---------------------------------------------------------------- the scale-factor formats
// One specialisation per format, and nothing about a format anywhere else in the casting files.  A format supplies:
//   elem          the type behind a scale-factor pointer (rows of hidden / kElemCols elements, contiguous)
//   kGroupCols    the columns that share a scale factor
//   kElemCols     the columns one stored element covers; hidden is a positive multiple of it
//   word<C>       the cast's store, for lanes of C = 8 or 16 columns: the element of the lane's kElemCols columns from
//                 the lane's group factor (every lane of the wave active); who stores it where: SfTile below
//   the cast back (a lane holds 16 columns, vector u of its row; in: u is inside the row):
//   stride_unit   what the strides that the cast back is given count
//   back_dwords   a wave-uniform choice between two ways to load, from the strides
//   back_load, back_factor   what the lane loads for vector u; its group's factor from what its 8 lanes loaded
enum class Sf { kFp32, kExp128, kExp32 };

template <Sf kSf> struct SfFormat;
template <Sf kSf> using sf_elem_t = typename SfFormat<kSf>::elem;

// float32 [rows][hidden / 128]: the factor itself; the cast back's first lane of a group loads it, share8 hands it on
template <> struct SfFormat<Sf::kFp32> {
    using elem = float;
    static constexpr int kGroupCols = 128, kElemCols = 128;
    using stride_unit = float;
    template <int kLaneCols>
    static __device__ __forceinline__ float word(float sf, int) { return sf; }
    static __device__ __forceinline__ bool back_dwords(int64_t, int64_t) { return false; }
    static __device__ __forceinline__ float back_load(const float* sfs, int u, bool in, int lane, int64_t col_stride,
                                                      bool) {
        if (!(in && (lane & 7) == 0)) return 0.0f;
        return sfs[(u >> 3) * col_stride];
    }
    static __device__ __forceinline__ float back_factor(float loaded, int, bool) { return share8(loaded); }
};

// Packed UE8M0, int32 [rows][hidden / 512] (hidden % 512 == 0, round_scale): the exponent bytes of four groups of
// 128 columns to an element -- the form the reference's low-latency dispatch produces with use_ue8m0
// (csrc/kernels/legacy/internode_ll.cu:439-459, extract_required_scale_format at legacy/utils.cuh:505-512) and its
// per_token_cast_back takes (deep_ep/utils/math.py:51-53).  The e4m3fn bytes are the round_scale bytes.
// The cast: a pass of 64 lanes x 8 columns is one element, 64 lanes x 16 columns two (hidden % 512 == 0: the lanes of
// an element are all inside the row or all outside).  The cast back: the group's first lane loads the one byte of its
// group (group g: byte g & 3 of element g >> 2) and forms 2^e as byte << 23 (byte 0: +0.0f).
template <> struct SfFormat<Sf::kExp128> {
    using elem = uint32_t;
    static constexpr int kGroupCols = 128, kElemCols = 512;
    using stride_unit = uint32_t;
    template <int kLaneCols>
    static __device__ __forceinline__ uint32_t word(float sf, int lane) {
        const uint32_t byte = ue8m0_byte(sf);
        const uint32_t lo = ue8m0_gather4(byte, 0, 128 / kLaneCols);
        if constexpr (kLaneCols == 8) {
            return lo;
        } else {
            const uint32_t hi = ue8m0_gather4(byte, 32, 128 / kLaneCols);       // (both gathers by the whole wave)
            return lane < 32 ? lo : hi;
        }
    }
    static __device__ __forceinline__ bool back_dwords(int64_t, int64_t) { return false; }
    static __device__ __forceinline__ float back_load(const uint32_t* sfs, int u, bool in, int lane,
                                                      int64_t col_stride, bool) {
        if (!(in && (lane & 7) == 0)) return 0.0f;
        const int g = u >> 3;
        return deepep::ue8m0_factor(reinterpret_cast<const uint8_t*>(sfs + (g >> 2) * col_stride)[g & 3]);
    }
    static __device__ __forceinline__ float back_factor(float loaded, int, bool) { return share8(loaded); }
};

// MXFP8, uint8 [rows][hidden / 32] (hidden % 128 == 0, round_scale): the round_scale rule over groups of 32 columns,
// the group of v_mfma_scale_f32_*_f8f6f4, byte g the biased exponent of column group g.  A row is hidden / 128 whole
// dwords, and the cast stores dwords (never a byte store into a peer window): 128 columns to an element.
// The cast back is given byte strides; 8 lanes share one dword of four 2-lane groups.  Column stride 1 and rows 4
// bytes apart (back_dwords): the first lane of every 8 loads the dword, share8 hands it on and each lane takes byte
// (lane & 7) >> 1; any other strides: every lane loads its own group's byte.
template <> struct SfFormat<Sf::kExp32> {
    using elem = uint32_t;
    static constexpr int kGroupCols = 32, kElemCols = 128;
    using stride_unit = uint8_t;
    template <int kLaneCols>
    static __device__ __forceinline__ uint32_t word(float sf, int lane) {
        return ue8m0_or4<kGroupCols / kLaneCols>(ue8m0_byte(sf), lane);
    }
    static __device__ __forceinline__ bool back_dwords(int64_t row_stride, int64_t col_stride) {
        return col_stride == 1 && (row_stride & 3) == 0;
    }
    static __device__ __forceinline__ uint32_t back_load(const uint32_t* sfs, int u, bool in, int lane,
                                                         int64_t col_stride, bool dwords) {
        uint32_t w = 0;
        if (in) {
            if (!dwords) w = reinterpret_cast<const uint8_t*>(sfs)[(u >> 1) * col_stride];
            else if ((lane & 7) == 0) w = sfs[u >> 3];
        }
        return w;
    }
    static __device__ __forceinline__ float back_factor(uint32_t loaded, int lane, bool dwords) {
        return deepep::ue8m0_factor(dwords ? (share8(loaded) >> (((lane & 7) >> 1) * 8)) & 0xffu : loaded);
    }
};

// Who stores a format's elements where lane `lane` holds columns [v * kLaneCols, (v + 1) * kLaneCols) of its row and
// the wave's 64 lanes hold consecutive vectors v: the first of the kLanes lanes of an element, at index v / kLanes.
template <Sf kSf, int kLaneCols>
struct SfTile {
    using F = SfFormat<kSf>;
    static constexpr int kLanes = F::kElemCols / kLaneCols;
    static_assert(kLanes == 8 || kLanes == 16 || kLanes == 32 || kLanes == 64, "whole elements within a wave");
    static __device__ __forceinline__ bool owns(int lane) { return (lane & (kLanes - 1)) == 0; }
    static __device__ __forceinline__ int index(int v, int lane) {
        // (a whole wave per element: lane 0 stores, at the wave-uniform index of its own vector; v == v0 + lane)
        if constexpr (kLanes == 64) return (v - lane) >> 6;
        else return v >> __builtin_ctz(kLanes);
    }
    static __device__ __forceinline__ auto word(float sf, int lane) { return F::template word<kLaneCols>(sf, lane); }
};

}  // namespace
