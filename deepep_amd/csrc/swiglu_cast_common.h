// swiglu_cast_common.h -- what the activation's forward (swiglu_cast.hip) and backward (swiglu_backward_cast.hip) share
// around their own arithmetic: the rows that are live, and the row-wise cast of the 8 bf16 a lane holds.  The
// activation and its derivative stay in their files, each with its one definition.
#pragma once

#include "fp4_cast_common.h"
#include "fp6_cast_common.h"
#include "fp8_cast_common.h"
#include "mx_cast_t_common.h"

namespace {

// the rows that are read and written (wave-uniform: one scalar load)
__device__ __forceinline__ int64_t live_rows(int64_t num_rows, const int32_t* __restrict__ expert_ends, int num_experts,
                                             int expert_alignment) {
    if (expert_ends == nullptr) return num_rows;
    const int32_t last = expert_ends[num_experts - 1];
    if (last <= 0) return 0;
    const uint32_t a = static_cast<uint32_t>(expert_alignment);
    const int64_t end = static_cast<int64_t>((static_cast<uint32_t>(last) + a - 1u) / a) * a;     // (below 2^32)
    return end < num_rows ? end : num_rows;
}

// ---------------------------------------------------------------- rule 2, along hidden: a row's 8 columns
// In both kernels lane cl of 16 holds columns [8 cl, 8 cl + 8) of a block of 128 columns of one row: a quad is a group
// of 32 columns (the quad steps of group_max), 16 lanes the dword of the block's four exponent bytes, which lane 0
// stores -- the row-wise half of the transposed casts, to the instruction.  A block's codes are 4 * kBlockBytes bytes
// of the row; a lane's piece of them:
//   FP8  8 bytes at 8 cl                FP4  4 bytes at 4 cl
//   FP6  the lane's 8 codes are 48 bits; the quad's four are the group's 24 bytes, which its first three lanes store 8
//        bytes each, at 24 (cl >> 2) + 8 (cl & 3), after one quad DPP read of the next lane's
template <int kFormat> constexpr int kBlockBytes = kFormat == DEEPEP_MX_FP8 ? 32 : kFormat == DEEPEP_MX_FP6 ? 24 : 16;

template <int kFormat>
__device__ __forceinline__ uint32_t piece_off(int cl) {
    if constexpr (kFormat == DEEPEP_MX_FP8) return 8u * cl;
    else if constexpr (kFormat == DEEPEP_MX_FP4) return 4u * cl;
    else return kGroupBytes * (cl >> 2) + 8u * (cl & 3);
}

template <int kFormat>
__device__ __forceinline__ bool piece_stored(int cl) { return kFormat != DEEPEP_MX_FP6 || (cl & 3) < 3; }

// row: the lane's 8 bf16 -> its piece of the codes (FP4: the first dword) and the block's exponent dword.  Every lane
// of the 16 must be active.
template <int kFormat>
__device__ __forceinline__ void cast_row(const u32x4& row, int lane, u32x2& piece, uint32_t& w) {
    if constexpr (kFormat == DEEPEP_MX_FP8) {
        const Fp8Lane<1> r = cast_group_fp8<1, 32>(&row, 1);
        piece = r.q;
        w = SfTile<Sf::kExp32, 8>::word(r.sf, lane);
    } else if constexpr (kFormat == DEEPEP_MX_FP4) {
        const Fp4Lane<1> r = cast_group_fp4<1>(&row);
        piece = u32x2{r.q[0], 0u};
        w = ue8m0_or4<4>(r.byte, lane);
    } else {
        const Fp6Lane r = cast_group_fp6<1>(&row);
        w = ue8m0_or4<4>(r.byte, lane);
        // the lane's 48 bits: lo and the low half of hi; the next lane of the quad's (quad permute [1, 2, 3, 3]); piece
        // j of the group's three 8-byte pieces from lanes j and j + 1
        constexpr int kDppQuadNext = 0xF9;
        const uint32_t lo = r.q[0], hi = r.q[1];
        const uint32_t nlo = static_cast<uint32_t>(
            __builtin_amdgcn_mov_dpp(static_cast<int>(lo), kDppQuadNext, 0xf, 0xf, true));
        const uint32_t nhi = static_cast<uint32_t>(
            __builtin_amdgcn_mov_dpp(static_cast<int>(hi), kDppQuadNext, 0xf, 0xf, true));
        const int j = lane & 3;
        const uint32_t mix = hi | (nlo << 16);             // own bytes 4-5, the next lane's 0-1
        piece = j == 0 ? u32x2{lo, mix} : j == 1 ? u32x2{(lo >> 16) | (hi << 16), nlo}
                                                 : u32x2{mix, (nlo >> 16) | (nhi << 16)};
    }
}

}  // namespace
