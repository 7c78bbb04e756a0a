// cast_common.h -- what the casting kernels of fp8_cast.hip (e4m3fn rows), fp4_cast.hip (e2m1 rows) and fp6_cast.hip
// (e2m3 rows) share: the stores into a destination row that may lie in a peer window, the packing half of the fused
// pack (destination rows, bounds, fault record, the row's tail -- a restatement of pack_kernel of dispatch.hip, which
// stays as it is; the row layout is the same [x | sf | topk_idx | weights | src]), the cross-lane steps of a group's
// amax, the UE8M0 exponent bytes and the launchers' helpers.  One definition, so the element formats cannot drift.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdio.h>

#include "../../include/deepep_amd.h"
#include "fault.h"

extern "C" __attribute__((visibility("hidden"))) int deepep_amd_set_error(int code, const char* msg);

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool kPeer, typename V>
__device__ __forceinline__ void put(V* p, V v) {
    if constexpr (kPeer) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else *p = v;
}

template <bool kPeer>
__device__ __forceinline__ void put8(uint8_t* row, int off, const u32x2& v, int row_bytes) {
    if constexpr (kPeer) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, row_bytes, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, 17);           // sc0 sc1: system scope
    } else {
        *reinterpret_cast<u32x2*>(row + off) = v;
    }
}

// Lane r's byte address of the destination row of token t for rank r (0: not routed to r).
// (a row index outside the destination buffer -- offsets or slots that disagree with its size -- is
// never stored: bit 4 and the error record instead of a write past a window)
template <bool kPeer>
__device__ __forceinline__ uint64_t pack_dest_row(int t, int lane, const int32_t* __restrict__ dst_slot,
                                                  const int32_t* __restrict__ send_offsets, int R,
                                                  uint8_t* __restrict__ packed, const uint64_t* __restrict__ dest_bases,
                                                  int64_t row_bytes, int64_t dest_rows, int32_t* __restrict__ error_flag) {
    uint64_t my_row = 0;
    if (lane < R) {
        const int32_t s = dst_slot[static_cast<int64_t>(t) * R + lane];
        if (s >= 0) {
            const uint64_t base = kPeer ? dest_bases[lane] : reinterpret_cast<uint64_t>(packed);
            const int64_t row = static_cast<int64_t>(send_offsets[lane]) + s;
            if (row >= 0 && row < dest_rows)
                my_row = base + static_cast<uint64_t>(row) * row_bytes;
            else
                deepep::record_fault(error_flag, DEEPEP_FLAG_BAD_ADDRESS, DEEPEP_FAULT_PACK_ROW, t, lane,
                                     base + static_cast<uint64_t>(row) * row_bytes, dest_rows);
        }
    }
    return my_row;
}

// the row address lane r holds (pack_dest_row), as a wave-uniform pointer
__device__ __forceinline__ uint8_t* pack_row_of(uint64_t my_row, int r) {
    const uint64_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_row & 0xffffffffu), r));
    const uint64_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(my_row >> 32), r));
    return reinterpret_cast<uint8_t*>((hi << 32) | lo);
}

// the row's tail: [topk_idx | weights | src_global_idx] into every destination row of dmask
template <bool kPeer>
__device__ __forceinline__ void pack_tail(int t, int lane, uint64_t my_row, uint64_t dmask,
                                          const int64_t* __restrict__ topk_idx, const float* __restrict__ topk_weights,
                                          int K, int32_t src_base, int idx_off, int w_off, int src_off) {
    int64_t e = 0;
    float w = 0.0f;
    if (lane < K) {
        e = topk_idx[static_cast<int64_t>(t) * K + lane];
        w = topk_weights != nullptr ? topk_weights[static_cast<int64_t>(t) * K + lane] : 0.0f;
    }
    for (uint64_t m = dmask; m; m &= m - 1) {
        uint8_t* row = pack_row_of(my_row, __builtin_ctzll(m));
        if (lane < K) {
            put<kPeer>(reinterpret_cast<int64_t*>(row + idx_off) + lane, e);
            put<kPeer>(reinterpret_cast<float*>(row + w_off) + lane, w);
        }
        if (lane == 0) put<kPeer>(reinterpret_cast<int32_t*>(row + src_off), static_cast<int32_t>(src_base + t));
    }
}

// 8 bf16 of one 16-byte load as fp32
__device__ __forceinline__ void unpack8(const u32x4& raw, float* f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(raw[j] << 16);
        f[2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u);
    }
}

// the largest magnitude of the 8 bf16 of a 16-byte load and of m, as packed 16-bit magnitudes (a bf16 magnitude
// orders as its bits): the in-lane amax of the FP4 and FP6 casts
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 amax8(u16x2 m, const u32x4& raw) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2, raw[j] & 0x7fff7fffu));
    return m;
}

// a group's amax from its largest packed magnitude (a bf16 magnitude is the high half of the fp32 of the same
// value), never below 1e-4f
__device__ __forceinline__ float amax_floor(uint16_t m) {
    return fmaxf(__uint_as_float(static_cast<uint32_t>(m) << 16), 1e-4f);
}

// lane ^ 1 and lane ^ 2 of a quad (quad permutes [1,0,3,2] and [2,3,0,1]); the other quad of 8 lanes and the other
// half of a 16-lane row (mirrors: the order inside does not matter where every lane of a quad holds the same value);
// the first lane of every quad (quad permute [0,0,0,0])
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppRowMirror = 0x140, kDppQuadFirst = 0x00;

template <int kCtrl>
__device__ __forceinline__ float dpp_max(float v) {
    return fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), kCtrl, 0xf, 0xf, true)));
}

template <int kCtrl>
__device__ __forceinline__ uint32_t dpp_or(uint32_t v) {
    return v | static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), kCtrl, 0xf, 0xf, true));
}

// The maximum over the kLanes consecutive lanes of a group, in all of them (a maximum: the same value in any order).
// 16 lanes: the four-step butterfly; fewer: DPP lane swaps, no LDS round trip -- lanes ^1 and ^2, then the other quad
// of the 8 lanes (every lane of a quad holds the quad's maximum by then).
template <int kLanes>
__device__ __forceinline__ float group_max(float v) {
    static_assert(kLanes == 2 || kLanes == 4 || kLanes == 8 || kLanes == 16, "a group is 2, 4, 8 or 16 lanes");
    if constexpr (kLanes == 16) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    } else {
        v = dpp_max<kDppXor1>(v);
        if constexpr (kLanes >= 4) v = dpp_max<kDppXor2>(v);
        if constexpr (kLanes >= 8) v = dpp_max<kDppHalfMirror>(v);
    }
    return v;
}

// ---------------------------------------------------------------- UE8M0 exponent bytes
// A power-of-two scale factor 2^e (round_scale) travels as its biased exponent byte (bits(sf) >> 23) & 0xff; the
// kernels store four bytes as one dword, byte j (little-endian) of dword p the column group 4p + j.
__device__ __forceinline__ uint32_t ue8m0_byte(float sf) { return (__float_as_uint(sf) >> 23) & 0xffu; }

// the dword of the exponent bytes held by lanes l0, l0 + step, l0 + 2 * step, l0 + 3 * step (wave-uniform; every
// lane of the wave must be active and hold its group's byte)
__device__ __forceinline__ uint32_t ue8m0_gather4(uint32_t byte, int l0, int step) {
    const int b = static_cast<int>(byte);
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(b, l0)) |
           static_cast<uint32_t>(__builtin_amdgcn_readlane(b, l0 + step)) << 8 |
           static_cast<uint32_t>(__builtin_amdgcn_readlane(b, l0 + 2 * step)) << 16 |
           static_cast<uint32_t>(__builtin_amdgcn_readlane(b, l0 + 3 * step)) << 24;
}

// The dword of four consecutive groups of kGroupLanes lanes each (1: of a quad; 2: of 8 lanes; 4: of a 16-lane row),
// in all their lanes: every lane puts its group's byte in place, two DPP steps OR the four groups together.
template <int kGroupLanes>
__device__ __forceinline__ uint32_t ue8m0_or4(uint32_t byte, int lane) {
    static_assert(kGroupLanes == 1 || kGroupLanes == 2 || kGroupLanes == 4, "four groups within a 16-lane row");
    const uint32_t placed = byte << (((lane / kGroupLanes) & 3) * 8);
    if constexpr (kGroupLanes == 4) return dpp_or<kDppRowMirror>(dpp_or<kDppHalfMirror>(placed));
    else if constexpr (kGroupLanes == 2) return dpp_or<kDppHalfMirror>(dpp_or<kDppXor2>(placed));
    else return dpp_or<kDppXor2>(dpp_or<kDppXor1>(placed));
}

// ---------------------------------------------------------------- the launchers' helpers
int launch_status(const char* what) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s launch failed: %s", what, hipGetErrorString(err));
        return deepep_amd_set_error(DEEPEP_ERR_HIP, buf);
    }
    return DEEPEP_OK;
}

bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The entries' checks and launches are written once for every format; `what` names the entry in the error text.
int invalid(const char* what, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, msg);
    return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG, buf);
}

}  // namespace
