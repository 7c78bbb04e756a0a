// mx_cast_t_common.h -- what the kernels that quantise along the TOKEN axis share: the transposed casts of
// fp8_cast_t.hip (the tile's two constants only) and fp46_cast_t.hip, and the requantisation of requant_t.hip.  The
// tile's shape, the FP4 / FP6 element types as the tile sees them, and the pairing of two tokens of a column.  The
// kernel bodies stay in their files (requant_t.hip restates the casts' tile behind its load stages, to the
// instruction).
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

}  // namespace
