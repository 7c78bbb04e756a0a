// mx_cast_t_common.h -- what the kernels that quantise along the TOKEN axis share: the transposed casts of
// fp8_cast_t.hip (the tile's two constants only) and fp46_cast_t.hip, and the requantisation of requant_t.hip.  The
// tile's shape, the FP4 / FP6 element types as the tile sees them, and the pairing of two tokens of a column.  The
// kernel bodies stay in their files (requant_t.hip restates the casts' tile behind its load stages, to the
// instruction), as does swiglu_cast.hip; the tile's steps around its conversions are at the end of this file.
#pragma once

#include "fp6_cast_common.h"

namespace {

constexpr int kTile = 128;                                // tokens and columns of a tile
constexpr int kWaveTiles = 4;                             // tiles per wave: 512 tokens = 16 bytes of sf_t per column

enum class Mx { kFp4, kFp6 };

// Per element type: the bytes of one (column, block of 32 tokens) and the unit the LDS image is written in.
template <Mx kFmt> struct MxFormat;
template <> struct MxFormat<Mx::kFp4> {
    static constexpr int kBlockBytes = 16;                // 32 codes of 4 bits: one 16-byte unit
    using unit = u32x4;
};
template <> struct MxFormat<Mx::kFp6> {
    static constexpr int kBlockBytes = kGroupBytes;       // 32 codes of 6 bits: three 8-byte units
    using unit = u32x2;
};

// tokens (n, n + 1) of one column as the two bf16 of a dword, the lower token in the lower half -- the order both
// conversions take their sources in: a, b are the dwords of the two tokens that hold the column.  One v_perm_b32 (its
// selector bytes 0-3 name the bytes of the second operand, 4-7 those of the first): (a & 0xffff) | b << 16, or
// a >> 16 | (b & 0xffff0000) for the dword's high column.
__device__ __forceinline__ uint32_t pair_tokens(uint32_t a, uint32_t b, bool high) {
    return __builtin_amdgcn_perm(b, a, high ? 0x07060302u : 0x05040100u);
}

// ---------------------------------------------------------------- the tile around its conversions
// What the kernels that restate the casts' tile behind a load stage of their own (requant_t.hip, swiglu_cast.hip)
// share, after raw[i] holds the lane's 8 bf16 of token i.

// the work item of a workgroup: workgroups w = x (mod 8) share an XCD (observed, for speed only) and take consecutive
// items, column blocks fastest
__device__ __forceinline__ int64_t tile_item() {
    const int64_t per_xcd = gridDim.x / 8;
    return (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
}

// the packed 16-bit magnitudes' maximum over the lane's 32 tokens, per pair of columns
__device__ __forceinline__ void token_amax(const u32x4* raw, u16x2* m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = u16x2{0, 0};
#pragma unroll
    for (int i = 0; i < 32; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[j] = __builtin_elementwise_max(m[j], __builtin_bit_cast(u16x2, raw[i][j] & 0x7fff7fffu));
    }
}

// the tile's exponent dwords (lane l: columns 2l and 2l + 1) into the run's
__device__ __forceinline__ void keep_sf(u32x4* acc, const uint32_t* sf_image, int t, int lane) {
    const u32x2 s = reinterpret_cast<const u32x2*>(sf_image)[lane];
#pragma unroll
    for (int k = 0; k < kWaveTiles; ++k) {
        acc[0][k] = t == k ? s[0] : acc[0][k];
        acc[1][k] = t == k ? s[1] : acc[1][k];
    }
}

// a column's exponent dwords of the run: one 16-byte store per column (sf16: num_rows % 512 == 0 and a 16-byte aligned
// sf_t) or dwords (the tail)
__device__ __forceinline__ void store_sf(const u32x4* acc, uint8_t* __restrict__ sf_t, int64_t num_rows, int c0,
                                         int64_t n_base, int ntile, int sf16, int lane) {
    const int64_t sf_t_pitch = num_rows / 32;              // bytes per row of sf_t (a multiple of 4)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        uint8_t* dst = sf_t + (c0 + 2 * lane + p) * sf_t_pitch + n_base / 32;
        if (sf16 && ntile == kWaveTiles) {
            *reinterpret_cast<u32x4*>(dst) = acc[p];
        } else {
#pragma unroll
            for (int k = 0; k < kWaveTiles; ++k)
                if (k < ntile) reinterpret_cast<uint32_t*>(dst)[k] = acc[p][k];
        }
    }
}

}  // namespace
