// combine.hip -- the combine reduction for MI355X (gfx950, CDNA4), exported through
// the C-ABI declared in include/deepep_amd.h.
//
// What is computed (semantics of the reference, /root/reference paths):
//   DEEPEP_MODE_LOCAL    combine_impl's local reduce       deep_ep/include/deep_ep/impls/combine.cuh:114-213
//   DEEPEP_MODE_EPILOGUE combine_reduce_epilogue_impl      deep_ep/include/deep_ep/impls/combine_reduce_epilogue.cuh:62-125
//   arithmetic core      combine_reduce                    deep_ep/include/deep_ep/impls/combine_utils.cuh:55-170
//   weighted variant     legacy low-latency combine        csrc/kernels/legacy/internode_ll.cu:1072-1135
//
// How (MI355X-first, not a translation of the TMA/warp design):
//   * the work is split into items = (output row, column chunk of 64 lanes x vpt x 16 B); one wave64
//     owns one item and a workgroup of 4 or 8 waves owns that many consecutive items, so the grid is
//     tens of thousands of workgroups with no tail imbalance;
//   * the item's row of the slot table (and, weighted, the gating weights) is staged once per
//     workgroup in LDS, one entry per lane; the valid slots are visited in ascending order through
//     the wave's ballot mask (= the reference's compacted slot order);
//   * each lane keeps 2-8 rows x vpt x 16 B of non-temporal global_load_dwordx4 in flight (every
//     expanded row is read exactly once), accumulates bf16 -> fp32 in registers in the reference's
//     order, rounds once with v_cvt_pk_bf16_f32 (RNE) and writes vpt x 16 B with a write-through
//     buffer store;
//   * an FP8 source (kFp8: the caller's x as e4m3fn rows and per-128-column scale factors) is cast back in
//     registers with the arithmetic of the cast-back kernel (fp8_dequant.h): each dequantised value is rounded
//     to bf16 and enters the same accumulation.  A lane loads 8 bytes = 8 columns per vector (the bf16 geometry:
//     one 16-byte store per vector, whole 128-byte lines per store instruction); the 16-byte load with two
//     stores per lane is kept as kLoad = 16 and lost (launch_shape_fp8).  The bf16 copy of the expert rows is
//     never written or read.
//   No MFMA: this is an HBM-bound gather + elementwise add (roofline and measurements in DESIGN.md).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>

#include "../../include/deepep_amd.h"
#include "fault.h"
#include "fp8_dequant.h"
#include "logfmt_codec.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxWidth = 32;          // top-k <= 32, as the reference (combine_reduce_epilogue.cuh:64)

thread_local char g_last_error[512] = "";

int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}

__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// Round-to-nearest-even pack of two floats (v_cvt_pk_bf16_f32), = __float22bfloat162_rn.
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    const bf16x2 r = __builtin_convertvector((f32x2){a, b}, bf16x2);
    return __builtin_bit_cast(uint32_t, r);
}

template <bool kNT>
__device__ __forceinline__ u32x4 load16(const u32x4* p) {
    if constexpr (kNT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

struct Params {
    const uint16_t* src;
    int64_t num_src_rows;
    int64_t src_stride;          // elements
    const int32_t* table;
    int64_t table_stride;
    int table_width;
    const float* row_weights;
    const uint16_t* bias0;
    const uint16_t* bias1;
    uint16_t* out;
    int64_t out_stride;          // elements
    int num_units;
    int hidden;
    const int32_t* wtable;
    int64_t wtable_stride;
    const float* wsrc;
    float* out_weights;
    int num_weights;
    int weights_pad;             // floats written per unit's weight row (>= num_weights; zeros past them)
    int64_t out_weights_stride;  // floats between consecutive units' weight rows
    int units_per_block;
    int32_t* error_flag;
    const uint64_t* out_rows;    // scatter (phase A over xGMI): byte address of unit u's output row, or NULL
    int64_t weights_offset;      // scatter: byte offset of the weights inside the output row
    const uint64_t* win_bases;   // scatter: the windows every out_rows[u] must lie in (lane l < win_count: window l)
    int win_count;
    uint64_t win_limit;          // scatter: largest offset of a row start inside a window (extent - row bytes)
    const void* sf;              // FP8 source: the scale factors of src's rows (fp32, or int32 of four UE8M0 bytes)
    int64_t sf_row_stride;       // FP8 source: elements between consecutive rows' scale factors
    int64_t sf_col_stride;       // FP8 source: elements between consecutive scale factors of a row
    int sf_packed;               // FP8 source: sf is the packed UE8M0 form
};

// Scatter (phase A into the owners' windows): the byte address of unit u's row, or 0 when the unit must
// not be stored -- a row plan_expert rejected (0, bit 1) or one not wholly inside any window (bit 4 and
// the error record: a wild store through a bad address is never issued).  Wave-uniform.
__device__ __forceinline__ uint64_t checked_row(const Params& p, int64_t u, int lane, bool report) {
    const uint64_t a = p.out_rows[u];
    if (a == 1ull) return 0ull;                          // a padding position of a padded plan: no unit
    if (a == 0ull) {
        if (report && lane == 0 && p.error_flag != nullptr) atomicOr(p.error_flag, DEEPEP_FLAG_BAD_SLOT);
        return 0ull;
    }
    const uint64_t base = lane < p.win_count ? p.win_bases[lane] : 0ull;
    const bool inside = lane < p.win_count && (a & 15ull) == 0ull && a >= base && a - base <= p.win_limit;
    if (__ballot(inside) != 0ull) return a;
    if (report && lane == 0)
        deepep::record_fault(p.error_flag, DEEPEP_FLAG_BAD_ADDRESS, DEEPEP_FAULT_SCATTER_ROW, u, -1, a,
                             static_cast<int64_t>(p.win_limit >> 4));
    return 0ull;
}

// acc[8*v + e] += element e of the 16-byte vector (8 bf16)
__device__ __forceinline__ void acc_add(float* acc, const u32x4& v) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        acc[2 * d] += bf16_lo(v[d]);
        acc[2 * d + 1] += bf16_hi(v[d]);
    }
}

__device__ __forceinline__ void acc_fma(float* acc, const u32x4& v, float w) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        acc[2 * d] = __builtin_fmaf(bf16_lo(v[d]), w, acc[2 * d]);
        acc[2 * d + 1] = __builtin_fmaf(bf16_hi(v[d]), w, acc[2 * d + 1]);
    }
}

__device__ __forceinline__ u32x4 acc_pack(const float* acc) {
    u32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        r[d] = pack_bf16x2(acc[2 * d], acc[2 * d + 1]);
    return r;
}

// Output stores: buffer_store_dwordx4 with a per-row descriptor (the hardware range check drops the
// lanes past the row end).  Three cache policies ship, one per kind of output:
//   sc1     (write-through, line not kept in L2): the fused and epilogue reduces, whose output is
//           written in token order -- best or tied in every cache state measured;
//   sc1 nt  (write-through streaming): phase A's send rows, written once and read back only by the
//           exchange -- within 2 % of the best policy in every cache state at EP = 2 / 4 / 8;
//   sc0 sc1 (system scope): phase A into a peer's symmetric window over xGMI, visible to the owning
//           GPU once the kernel has completed, whatever MTYPE the importing process maps it with.
// (plain, nt and a per-unit sc1 / sc1 nt mix lost or were cache-state dependent; their measurements
// are in CHANGELOG.md, the code in git history.)
constexpr int kAuxSC1 = 16, kAuxSys = 17, kAuxSC1NT = 18;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* row, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(row), 0, bytes, 0x00020000);
}

// The pass-through weight of lane k of unit u: wsrc[wtable[u][k]] (or wsrc[u * num_weights + k]), 0
// for masked lanes and for lanes past num_weights (the zeros of a padded tail line).  When the slot
// table doubles as the weight table (the expanded layouts) the lane's slot is already in hand -- and
// so is its weight when the reduction is weighted by the same array -- so no dependent gather
// delays the wave's row loads.
template <bool kWeighted>
__device__ __forceinline__ float pass_through_weight(const Params& p, int64_t u, int lane, int32_t my_slot, float my_w) {
    if (lane >= p.num_weights) return 0.0f;
    if (p.table != nullptr && p.wtable == p.table && p.wtable_stride == p.table_stride && lane < p.table_width) {
        if (kWeighted && p.wsrc == p.row_weights) return my_w;
        return my_slot >= 0 ? p.wsrc[my_slot] : 0.0f;
    }
    const int64_t i = p.wtable == nullptr ? u * p.num_weights + lane
                                          : static_cast<int64_t>(p.wtable[u * p.wtable_stride + lane]);
    return i >= 0 ? p.wsrc[i] : 0.0f;
}

// Store it: into the unit's weight row, or the row tail of a peer's window (system scope, as the
// row stores).  weights_pad > num_weights writes a packed row's whole 128-byte tail line.
__device__ __forceinline__ void store_weight(const Params& p, int64_t u, uint16_t* out_row, int lane, float v) {
    if (p.out_rows != nullptr) {
        float* const ow = reinterpret_cast<float*>(reinterpret_cast<char*>(out_row) + p.weights_offset);
        __hip_atomic_store(ow + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        p.out_weights[u * p.out_weights_stride + lane] = v;
    }
}

// FP8 source: row `slot` (a validated slot of the staged table, never a raw table entry) of the e4m3fn rows,
// and its scale factor for the 128-column group g.  Packed or not only changes which dword is loaded and how
// it becomes a factor.
__device__ __forceinline__ const u32x4* fp8_row(const Params& p, int32_t slot) {
    return reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(p.src) + static_cast<int64_t>(slot) * p.src_stride);
}

// One source vector (kLoad e4m3fn bytes, the low dwords of raw) cast back with its group's factor: kLoad / 8
// 16-byte vectors of bf16.
template <int kLoad>
__device__ __forceinline__ void fp8_bf16(const u32x4& raw, float s, u32x4* b) {
    if constexpr (kLoad == 16) deepep::dequant16(raw, s, b[0], b[1]);
    else b[0] = deepep::dequant8(raw[0], raw[1], s);
}

__device__ __forceinline__ float load_sf(const Params& p, int32_t slot, int g) {
    const uint32_t* row = static_cast<const uint32_t*>(p.sf) + static_cast<int64_t>(slot) * p.sf_row_stride;
    // a wave-uniform branch, which the compiler lifts out of the row loop; the same load with the index and the value
    // chosen by selects was slower in every shape (config 2, fused: 159 against 107 us)
    if (p.sf_packed) {
        const uint32_t word = row[(g >> 2) * p.sf_col_stride];
        return deepep::ue8m0_factor((word >> ((g & 3) * 8)) & 0xffu);
    }
    return __uint_as_float(row[g * p.sf_col_stride]);
}

// One wave per item = (unit u, column chunk c): the chunk is 64 lanes x kVPT x 16 B of every
// source row of u.  The unit's slot table row (and its gating weights) arrive in my_slot / my_w, one
// entry per lane; the valid slots are then visited in ascending order through the ballot mask,
// which is exactly the compacted order of compute_topk_slots (combine_utils.cuh:41-53).
template <int kMode, bool kWeighted, int kVPT, bool kFull, int kStoreAux, int kGroup>
__device__ __forceinline__ void combine_item(const Params& p, int64_t it, int nchunks, int nvec, int lane,
                                             int32_t my_slot, float my_w) {
    constexpr int kChunkVecs = 64 * kVPT;
    const int64_t u = it / nchunks;
    const int c = static_cast<int>(it - u * nchunks);
    // A barrier of this window timed out (bit 2 of the error flag, set by deepep_sym_barrier /
    // _wait): the rows in flight are not trustworthy, so no store reaches a peer and the output is
    // poisoned with NaN instead of holding a silently wrong sum.
    const bool aborted = p.error_flag != nullptr && (__hip_atomic_load(p.error_flag, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT) & 2);
    if (aborted && p.out_rows != nullptr) return;
    if (aborted) my_slot = -1;
    const uint64_t valid = __ballot(my_slot >= 0);
    const int n = __popcll(valid);

    // ---- top-k weight pass-through (combine.cuh:215-226, combine_reduce_epilogue.cuh:127-141),
    //      written once per unit by the wave owning chunk 0: gathered here, stored after the row
    uint16_t* const out_row = p.out_rows != nullptr ? reinterpret_cast<uint16_t*>(checked_row(p, u, lane, c == 0))
                                                     : p.out + u * p.out_stride;
    if (out_row == nullptr) return;                      // rejected / outside every window: flagged above
    const bool wlane = c == 0 && p.num_weights > 0 && lane < p.weights_pad;
    const float wv = wlane ? pass_through_weight<kWeighted>(p, u, lane, my_slot, my_w) : 0.0f;

    int vidx[kVPT];
    bool vok[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        vidx[v] = c * kChunkVecs + v * 64 + lane;
        vok[v] = kFull || vidx[v] < nvec;
    }
    const bool has_bias0 = p.bias0 != nullptr, has_bias1 = p.bias1 != nullptr;
    const bool has_bias = has_bias0 || has_bias1;

    // Initial value: -0.0f where the reference adds two sources in bf16 without an fp32 zero in
    // front (the hadd bypass, combine_utils.cuh:79-110: -0 + a == a exactly), +0.0f where it
    // starts from `float2 reduced = {}` (combine_utils.cuh:114).
    bool copy_row = false;
    float init;
    if constexpr (kMode == DEEPEP_MODE_LOCAL || kMode == DEEPEP_MODE_FUSED) {
        copy_row = !kWeighted && n == 1;                      // no_local_reduce (combine.cuh:134-156)
        init = (!kWeighted && n == 2) ? -0.0f : 0.0f;
    } else {
        // epilogue: bypass only without bias; weighted (single reduction, legacy semantics): from +0
        init = (!kWeighted && !has_bias && n == 2) ? -0.0f : 0.0f;
    }
    float acc[kVPT][8];
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[v][e] = init;
    if constexpr (kMode == DEEPEP_MODE_EPILOGUE) {
        // bias0 then bias1 before the partials (combine_utils.cuh:113-127)
#pragma unroll
        for (int v = 0; v < kVPT; ++v) {
            if (has_bias0 && vok[v]) acc_add(acc[v], *(reinterpret_cast<const u32x4*>(p.bias0 + u * p.hidden) + vidx[v]));
            if (has_bias1 && vok[v]) acc_add(acc[v], *(reinterpret_cast<const u32x4*>(p.bias1 + u * p.hidden) + vidx[v]));
        }
    }

    // The valid lanes, lowest first, kGroup at a time: every row of a group is loaded before any is
    // accumulated (kGroup rows x kVPT x 16 B in flight per lane), and the accumulation order is the
    // ascending lane order of compute_topk_slots whatever the group size.  `rem` is wave-uniform.
    u32x4 result[kVPT];
    uint64_t rem = valid;
    while (rem != 0ull) {
        int lane_of[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            lane_of[j] = rem != 0ull ? static_cast<int>(__builtin_ctzll(rem)) : -1;
            rem &= rem - 1ull;                              // (no-op once empty)
        }
        u32x4 vals[kGroup][kVPT];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (lane_of[j] >= 0) {
                const int32_t sj = __builtin_amdgcn_readlane(my_slot, lane_of[j]);
                const u32x4* row = reinterpret_cast<const u32x4*>(p.src + static_cast<int64_t>(sj) * p.src_stride);
#pragma unroll
                for (int v = 0; v < kVPT; ++v)
                    vals[j][v] = vok[v] ? load16<true>(row + vidx[v]) : (u32x4){0u, 0u, 0u, 0u};
            }
        }
        if (copy_row) {
#pragma unroll
            for (int v = 0; v < kVPT; ++v) result[v] = vals[0][v];        // n == 1: lane_of[0] is it
        } else {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                if (lane_of[j] >= 0) {
                    if constexpr (kWeighted) {
                        const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), lane_of[j]));
#pragma unroll
                        for (int v = 0; v < kVPT; ++v) acc_fma(acc[v], vals[j][v], w);
                    } else {
#pragma unroll
                        for (int v = 0; v < kVPT; ++v) acc_add(acc[v], vals[j][v]);
                    }
                }
            }
        }
    }
    if (!copy_row) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v) result[v] = acc_pack(acc[v]);
    }

    if constexpr (kMode == DEEPEP_MODE_FUSED) {
        // Phase B over the single per-rank partial (EP = 1): epilogue with one slot.
        // No bias: hadd bypass with a zero second operand -> +0 + partial.
        // Bias: fp32 +0 + bias0 + bias1 + partial, one rounding (combine_utils.cuh:111-165).
        const bool present = n > 0;
#pragma unroll
        for (int v = 0; v < kVPT; ++v) {
            float a[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = 0.0f;
            if (has_bias0 && vok[v]) acc_add(a, *(reinterpret_cast<const u32x4*>(p.bias0 + u * p.hidden) + vidx[v]));
            if (has_bias1 && vok[v]) acc_add(a, *(reinterpret_cast<const u32x4*>(p.bias1 + u * p.hidden) + vidx[v]));
            if (present) acc_add(a, result[v]);
            result[v] = acc_pack(a);
        }
    }

    if (aborted) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v) result[v] = (u32x4){0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};
    }
    const __amdgpu_buffer_rsrc_t orow = row_rsrc(out_row, p.hidden * 2);
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
        __builtin_amdgcn_raw_buffer_store_b128(result[v], orow, vidx[v] * 16, 0, kStoreAux);
    if (wlane) store_weight(p, u, out_row, lane, wv);
}

// combine_item for an FP8 source: the same item, order and rounding; a source vector is one kLoad-byte load of kLoad
// columns, cast back to bf16 (fp8_bf16) before it enters the sum, and kLoad / 8 16-byte output vectors per lane.  It
// is a function of its own, and combine_item above is kept as it was, so that the bf16 source's device code does not
// change by an instruction; whatever changes the reduction changes both.
template <int kMode, bool kWeighted, int kVPT, bool kFull, int kStoreAux, int kGroup, int kLoad>
__device__ __forceinline__ void combine_item_fp8(const Params& p, int64_t it, int nchunks, int nvec, int lane,
                                                 int32_t my_slot, float my_w) {
    static_assert(kLoad == 8 || kLoad == 16, "an FP8 source vector is one 8- or 16-byte load");
    constexpr int kChunkVecs = 64 * kVPT;
    constexpr int kOut = kLoad / 8;                      // 16-byte bf16 vectors per source vector
    constexpr int kGroupShift = kLoad == 16 ? 3 : 4;     // source vectors per 128-column group, log2
    const int64_t u = it / nchunks;
    const int c = static_cast<int>(it - u * nchunks);
    // A barrier of this window timed out (bit 2 of the error flag, set by deepep_sym_barrier /
    // _wait): the rows in flight are not trustworthy, so no store reaches a peer and the output is
    // poisoned with NaN instead of holding a silently wrong sum.
    const bool aborted = p.error_flag != nullptr && (__hip_atomic_load(p.error_flag, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT) & 2);
    if (aborted && p.out_rows != nullptr) return;
    if (aborted) my_slot = -1;
    const uint64_t valid = __ballot(my_slot >= 0);
    const int n = __popcll(valid);

    // ---- top-k weight pass-through (combine.cuh:215-226, combine_reduce_epilogue.cuh:127-141),
    //      written once per unit by the wave owning chunk 0: gathered here, stored after the row
    uint16_t* const out_row = p.out_rows != nullptr ? reinterpret_cast<uint16_t*>(checked_row(p, u, lane, c == 0))
                                                     : p.out + u * p.out_stride;
    if (out_row == nullptr) return;                      // rejected / outside every window: flagged above
    const bool wlane = c == 0 && p.num_weights > 0 && lane < p.weights_pad;
    const float wv = wlane ? pass_through_weight<kWeighted>(p, u, lane, my_slot, my_w) : 0.0f;

    int vidx[kVPT];
    bool vok[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        vidx[v] = c * kChunkVecs + v * 64 + lane;
        vok[v] = kFull || vidx[v] < nvec;
    }
    const bool has_bias0 = p.bias0 != nullptr, has_bias1 = p.bias1 != nullptr;
    const bool has_bias = has_bias0 || has_bias1;

    // Initial value: -0.0f where the reference adds two sources in bf16 without an fp32 zero in
    // front (the hadd bypass, combine_utils.cuh:79-110: -0 + a == a exactly), +0.0f where it
    // starts from `float2 reduced = {}` (combine_utils.cuh:114).
    bool copy_row = false;
    float init;
    if constexpr (kMode == DEEPEP_MODE_LOCAL || kMode == DEEPEP_MODE_FUSED) {
        copy_row = !kWeighted && n == 1;                      // no_local_reduce (combine.cuh:134-156)
        init = (!kWeighted && n == 2) ? -0.0f : 0.0f;
    } else {
        // epilogue: bypass only without bias; weighted (single reduction, legacy semantics): from +0
        init = (!kWeighted && !has_bias && n == 2) ? -0.0f : 0.0f;
    }
    float acc[kVPT][8 * kOut];
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
#pragma unroll
        for (int e = 0; e < 8 * kOut; ++e) acc[v][e] = init;
    if constexpr (kMode == DEEPEP_MODE_EPILOGUE) {
        // bias0 then bias1 before the partials (combine_utils.cuh:113-127)
#pragma unroll
        for (int v = 0; v < kVPT; ++v) {
#pragma unroll
            for (int o = 0; o < kOut; ++o) {
                const int ov = vidx[v] * kOut + o;
                if (has_bias0 && vok[v]) acc_add(acc[v] + 8 * o, *(reinterpret_cast<const u32x4*>(p.bias0 + u * p.hidden) + ov));
                if (has_bias1 && vok[v]) acc_add(acc[v] + 8 * o, *(reinterpret_cast<const u32x4*>(p.bias1 + u * p.hidden) + ov));
            }
        }
    }

    // The valid lanes, lowest first, kGroup at a time: every row of a group is loaded before any is
    // accumulated (kGroup rows x kVPT x 16 B in flight per lane), and the accumulation order is the
    // ascending lane order of compute_topk_slots whatever the group size.  `rem` is wave-uniform.
    u32x4 result[kVPT][kOut];
    uint64_t rem = valid;
    while (rem != 0ull) {
        int lane_of[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            lane_of[j] = rem != 0ull ? static_cast<int>(__builtin_ctzll(rem)) : -1;
            rem &= rem - 1ull;                              // (no-op once empty)
        }
        u32x4 vals[kGroup][kVPT];
        float sfs[kGroup][kVPT];                            // the factor of each vector's 128-column group
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (lane_of[j] >= 0) {
                const int32_t sj = __builtin_amdgcn_readlane(my_slot, lane_of[j]);
                const u32x4* row = fp8_row(p, sj);
#pragma unroll
                for (int v = 0; v < kVPT; ++v) {
                    vals[j][v] = (u32x4){0u, 0u, 0u, 0u};
                    if constexpr (kLoad == 16) {
                        if (vok[v]) vals[j][v] = load16<true>(row + vidx[v]);
                    } else if (vok[v]) {
                        const u32x2 half = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(row) + vidx[v]);
                        vals[j][v][0] = half[0];
                        vals[j][v][1] = half[1];
                    }
                    sfs[j][v] = vok[v] ? load_sf(p, sj, vidx[v] >> kGroupShift) : 0.0f;
                }
            }
        }
        if (copy_row) {
#pragma unroll
            for (int v = 0; v < kVPT; ++v)                   // n == 1: lane_of[0] is it; the dequantised bf16 row
                fp8_bf16<kLoad>(vals[0][v], sfs[0][v], result[v]);
        } else {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                if (lane_of[j] >= 0) {
                    float w = 0.0f;
                    if constexpr (kWeighted) w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), lane_of[j]));
#pragma unroll
                    for (int v = 0; v < kVPT; ++v) {
                        u32x4 b[kOut];
                        fp8_bf16<kLoad>(vals[j][v], sfs[j][v], b);
#pragma unroll
                        for (int o = 0; o < kOut; ++o) {
                            if constexpr (kWeighted) acc_fma(acc[v] + 8 * o, b[o], w);
                            else acc_add(acc[v] + 8 * o, b[o]);
                        }
                    }
                }
            }
        }
    }
    if (!copy_row) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v)
#pragma unroll
            for (int o = 0; o < kOut; ++o) result[v][o] = acc_pack(acc[v] + 8 * o);
    }

    if constexpr (kMode == DEEPEP_MODE_FUSED) {
        // Phase B over the single per-rank partial (EP = 1): epilogue with one slot.
        // No bias: hadd bypass with a zero second operand -> +0 + partial.
        // Bias: fp32 +0 + bias0 + bias1 + partial, one rounding (combine_utils.cuh:111-165).
        const bool present = n > 0;
#pragma unroll
        for (int v = 0; v < kVPT; ++v) {
#pragma unroll
            for (int o = 0; o < kOut; ++o) {
                const int ov = vidx[v] * kOut + o;
                float a[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = 0.0f;
                if (has_bias0 && vok[v]) acc_add(a, *(reinterpret_cast<const u32x4*>(p.bias0 + u * p.hidden) + ov));
                if (has_bias1 && vok[v]) acc_add(a, *(reinterpret_cast<const u32x4*>(p.bias1 + u * p.hidden) + ov));
                if (present) acc_add(a, result[v][o]);
                result[v][o] = acc_pack(a);
            }
        }
    }

    if (aborted) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v)
#pragma unroll
            for (int o = 0; o < kOut; ++o) result[v][o] = (u32x4){0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};
    }
    const __amdgpu_buffer_rsrc_t orow = row_rsrc(out_row, p.hidden * 2);
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
#pragma unroll
        for (int o = 0; o < kOut; ++o)
            __builtin_amdgcn_raw_buffer_store_b128(result[v][o], orow, (vidx[v] * kOut + o) * 16, 0, kStoreAux);
    if (wlane) store_weight(p, u, out_row, lane, wv);
}

// combine_item for a LogFMT source (MODE_EPILOGUE only: phase B of an EP > 1 combine whose rows crossed the links as
// LogFMT-10, logfmt_codec.h): combine_item_fp8 at 8-byte loads with the decode in place of dequant8.  p.src is the
// rows' low plane (p.src_stride counts bytes), the high plane follows it at byte p.hidden, and p.sf holds the groups'
// meta dwords (p.sf_row_stride dwords a row); a source vector is 8 columns -- one 8-byte load, one 2-byte load and the
// group's dword, each through the validated slot -- decoded to 8 bf16 before it enters the sum.  The same staging,
// ballot order, starts, bias order, NaN poison, weight pass-through and store policy; a function of its own, so
// that the two above do not change by an instruction.
template <bool kWeighted, int kVPT, int kStoreAux, int kGroup>
__device__ __forceinline__ void combine_item_logfmt(const Params& p, int64_t it, int nchunks, int nvec, int lane,
                                                    int32_t my_slot, float my_w) {
    constexpr int kChunkVecs = 64 * kVPT;
    const int64_t u = it / nchunks;
    const int c = static_cast<int>(it - u * nchunks);
    const bool aborted = p.error_flag != nullptr && (__hip_atomic_load(p.error_flag, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT) & 2);
    if (aborted) my_slot = -1;
    const uint64_t valid = __ballot(my_slot >= 0);
    const int n = __popcll(valid);

    uint16_t* const out_row = p.out + u * p.out_stride;
    const bool wlane = c == 0 && p.num_weights > 0 && lane < p.weights_pad;
    const float wv = wlane ? pass_through_weight<kWeighted>(p, u, lane, my_slot, my_w) : 0.0f;

    int vidx[kVPT];
    bool vok[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        vidx[v] = c * kChunkVecs + v * 64 + lane;
        vok[v] = vidx[v] < nvec;
    }
    const bool has_bias0 = p.bias0 != nullptr, has_bias1 = p.bias1 != nullptr;
    const bool has_bias = has_bias0 || has_bias1;
    // epilogue: the hadd bypass (-0.0f) only without bias; weighted (single reduction, legacy semantics): from +0
    const float init = (!kWeighted && !has_bias && n == 2) ? -0.0f : 0.0f;
    float acc[kVPT][8];
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[v][e] = init;
    // bias0 then bias1 before the partials (combine_utils.cuh:113-127)
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        if (has_bias0 && vok[v]) acc_add(acc[v], *(reinterpret_cast<const u32x4*>(p.bias0 + u * p.hidden) + vidx[v]));
        if (has_bias1 && vok[v]) acc_add(acc[v], *(reinterpret_cast<const u32x4*>(p.bias1 + u * p.hidden) + vidx[v]));
    }

    uint64_t rem = valid;
    while (rem != 0ull) {
        int lane_of[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            lane_of[j] = rem != 0ull ? static_cast<int>(__builtin_ctzll(rem)) : -1;
            rem &= rem - 1ull;                              // (no-op once empty)
        }
        u32x2 low[kGroup][kVPT];
        uint32_t high[kGroup][kVPT], meta[kGroup][kVPT];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (lane_of[j] >= 0) {
                const int32_t sj = __builtin_amdgcn_readlane(my_slot, lane_of[j]);
                const uint8_t* row = reinterpret_cast<const uint8_t*>(p.src) + static_cast<int64_t>(sj) * p.src_stride;
                const uint32_t* mrow = static_cast<const uint32_t*>(p.sf) + static_cast<int64_t>(sj) * p.sf_row_stride;
#pragma unroll
                for (int v = 0; v < kVPT; ++v) {
                    low[j][v] = (u32x2){0u, 0u};
                    high[j][v] = 0u;
                    meta[j][v] = 0u;
                    if (vok[v]) {
                        low[j][v] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(row) + vidx[v]);
                        high[j][v] = reinterpret_cast<const uint16_t*>(row + p.hidden)[vidx[v]];
                        meta[j][v] = mrow[vidx[v] >> 4];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (lane_of[j] >= 0) {
                float w = 0.0f;
                if constexpr (kWeighted) w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), lane_of[j]));
#pragma unroll
                for (int v = 0; v < kVPT; ++v) {
                    const u32x4 b = deepep::lf_decode8(low[j][v][0], low[j][v][1], high[j][v], meta[j][v]);
                    if constexpr (kWeighted) acc_fma(acc[v], b, w);
                    else acc_add(acc[v], b);
                }
            }
        }
    }
    u32x4 result[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) result[v] = acc_pack(acc[v]);
    if (aborted) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v) result[v] = (u32x4){0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};
    }
    const __amdgpu_buffer_rsrc_t orow = row_rsrc(out_row, p.hidden * 2);
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
        __builtin_amdgcn_raw_buffer_store_b128(result[v], orow, vidx[v] * 16, 0, kStoreAux);
    if (wlane) store_weight(p, u, out_row, lane, wv);
}

// A workgroup of kWaves waves takes kWaves consecutive items; the slot-table rows of the units those
// items belong to (and their gating weights) are staged once per workgroup in LDS, one entry per lane.
// One workgroup per kWaves items: 28,672 workgroups at config 2, no tail imbalance.
template <int kMode, bool kWeighted, int kVPT, bool kFull, int kStoreAux, int kWaves, int kGroup, int kFp8>
__global__ void __launch_bounds__(64 * kWaves)
combine_rows_kernel(const Params p) {
    constexpr int kChunkVecs = 64 * kVPT;
    __shared__ int32_t s_slot[kWaves][kMaxWidth];
    __shared__ float s_w[kWaves][kMaxWidth];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nvec = p.hidden >> (kFp8 == 16 ? 4 : 3);       // vectors per source row (kFp8: the bytes of an FP8 one, or 0)
    const int nchunks = (nvec + kChunkVecs - 1) / kChunkVecs;
    const int64_t items = static_cast<int64_t>(p.num_units) * nchunks;
    const int width = p.table == nullptr ? 1 : p.table_width;
    const int64_t it0 = static_cast<int64_t>(blockIdx.x) * kWaves;
    const int64_t it = it0 + wave;
    const int64_t u_first = it0 / nchunks;
    const int nu = static_cast<int>(min(it0 + kWaves - 1, items - 1) / nchunks - u_first) + 1;
    if (tid < nu * width) {                                  // nu * width <= kWaves * 32 threads
        const int ul = tid / width, j = tid - ul * width;
        const int64_t u = u_first + ul;
        int32_t s = p.table == nullptr ? static_cast<int32_t>(u) : p.table[u * p.table_stride + j];
        if (s >= p.num_src_rows) {                           // never dereference a bad slot
            if (p.error_flag != nullptr) atomicOr(p.error_flag, DEEPEP_FLAG_BAD_SLOT);
            s = -1;
        }
        s_slot[ul][j] = s;
        if constexpr (kWeighted) s_w[ul][j] = s >= 0 ? p.row_weights[s] : 0.0f;
    }
    __syncthreads();
    if (it >= items) return;
    int32_t my_slot = -1;
    float my_w = 0.0f;
    if (lane < width) {
        const int ul = static_cast<int>(it / nchunks - u_first);
        my_slot = s_slot[ul][lane];
        if constexpr (kWeighted) my_w = s_w[ul][lane];
    }
    if constexpr (kFp8 != 0) combine_item_fp8<kMode, kWeighted, kVPT, kFull, kStoreAux, kGroup, kFp8>(p, it, nchunks, nvec, lane, my_slot, my_w);
    else combine_item<kMode, kWeighted, kVPT, kFull, kStoreAux, kGroup>(p, it, nchunks, nvec, lane, my_slot, my_w);
}

// combine_rows_kernel for a LogFMT source: the same staging, then combine_item_logfmt (the epilogue, 8 waves).
template <bool kWeighted, int kVPT, int kStoreAux, int kGroup>
__global__ void __launch_bounds__(64 * 8)
combine_rows_logfmt_kernel(const Params p) {
    constexpr int kWaves = 8;
    constexpr int kChunkVecs = 64 * kVPT;
    __shared__ int32_t s_slot[kWaves][kMaxWidth];
    __shared__ float s_w[kWaves][kMaxWidth];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nvec = p.hidden >> 3;
    const int nchunks = (nvec + kChunkVecs - 1) / kChunkVecs;
    const int64_t items = static_cast<int64_t>(p.num_units) * nchunks;
    const int width = p.table == nullptr ? 1 : p.table_width;
    const int64_t it0 = static_cast<int64_t>(blockIdx.x) * kWaves;
    const int64_t it = it0 + wave;
    const int64_t u_first = it0 / nchunks;
    const int nu = static_cast<int>(min(it0 + kWaves - 1, items - 1) / nchunks - u_first) + 1;
    if (tid < nu * width) {                                  // nu * width <= kWaves * 32 threads
        const int ul = tid / width, j = tid - ul * width;
        const int64_t u = u_first + ul;
        int32_t s = p.table == nullptr ? static_cast<int32_t>(u) : p.table[u * p.table_stride + j];
        if (s >= p.num_src_rows) {                           // never dereference a bad slot
            if (p.error_flag != nullptr) atomicOr(p.error_flag, DEEPEP_FLAG_BAD_SLOT);
            s = -1;
        }
        s_slot[ul][j] = s;
        if constexpr (kWeighted) s_w[ul][j] = s >= 0 ? p.row_weights[s] : 0.0f;
    }
    __syncthreads();
    if (it >= items) return;
    int32_t my_slot = -1;
    float my_w = 0.0f;
    if (lane < width) {
        const int ul = static_cast<int>(it / nchunks - u_first);
        my_slot = s_slot[ul][lane];
        if constexpr (kWeighted) my_w = s_w[ul][lane];
    }
    combine_item_logfmt<kWeighted, kVPT, kStoreAux, kGroup>(p, it, nchunks, nvec, lane, my_slot, my_w);
}

// combine_item<MODE_LOCAL> as the scatter runs it (phase A into the owners' windows), with a LogFMT wire row in place
// of the bf16 row (combine(use_logfmt=True) over xGMI; the reference encodes in its sending kernel straight into the
// peer's buffer, internode_ll.cu:557-638 in :992-1100).  The same item, staging, ballot order, window check, starts
// and single rounding (acc_pack); the rounded bf16 bits are then encoded in registers, so the wire row is bit for bit
// deepep_cast_logfmt of the row the bf16 scatter would have stored.  hidden % 128 == 0 and a chunk is 512 x kVPT
// columns, so the 16 lanes of a quarter wave hold one whole 128-column group per vector -- inside the row or outside
// it -- and its amax / amin are encode_row's four-step butterfly (logfmt.hip); lanes past the row end hold zeros and
// take part.  Every exit before the butterfly is wave-uniform.  The wire row [low | high | meta | pad | weight tail]:
// 8 bytes a lane into the low plane, 2 into the high plane, the group's dword by its first lane, all system-scope
// buffer stores through a descriptor of the coded bytes; the padding behind the meta is not written.  A function of
// its own, so that the three above do not change by an instruction.
template <bool kWeighted, int kVPT, int kGroup>
__device__ __forceinline__ void combine_item_scatter_logfmt(const Params& p, int64_t it, int nchunks, int nvec, int lane,
                                                            int32_t my_slot, float my_w) {
    constexpr int kChunkVecs = 64 * kVPT;
    const int64_t u = it / nchunks;
    const int c = static_cast<int>(it - u * nchunks);
    // A barrier of this window timed out (bit 2 of the error flag): no store reaches a peer.  Through the ballot, so
    // that the wave leaves as one even if the flag is set between two lanes' loads.
    const bool aborted = __ballot(p.error_flag != nullptr && (__hip_atomic_load(p.error_flag, __ATOMIC_RELAXED,
                                                                                __HIP_MEMORY_SCOPE_AGENT) & 2)) != 0ull;
    if (aborted) return;
    const uint64_t valid = __ballot(my_slot >= 0);
    const int n = __popcll(valid);

    uint8_t* const out_row = reinterpret_cast<uint8_t*>(checked_row(p, u, lane, c == 0));
    if (out_row == nullptr) return;                      // rejected / outside every window: flagged above
    const bool wlane = c == 0 && p.num_weights > 0 && lane < p.weights_pad;
    const float wv = wlane ? pass_through_weight<kWeighted>(p, u, lane, my_slot, my_w) : 0.0f;

    int vidx[kVPT];
    bool vok[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        vidx[v] = c * kChunkVecs + v * 64 + lane;
        vok[v] = vidx[v] < nvec;
    }
    // MODE_LOCAL: the copy of a single row (no_local_reduce, combine.cuh:134-156), -0.0f in front of two rows (the
    // hadd bypass, combine_utils.cuh:79-110), else from +0
    const bool copy_row = !kWeighted && n == 1;
    const float init = (!kWeighted && n == 2) ? -0.0f : 0.0f;
    float acc[kVPT][8];
#pragma unroll
    for (int v = 0; v < kVPT; ++v)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[v][e] = init;

    u32x4 result[kVPT];
#pragma unroll
    for (int v = 0; v < kVPT; ++v) result[v] = (u32x4){0u, 0u, 0u, 0u};
    uint64_t rem = valid;
    while (rem != 0ull) {
        int lane_of[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            lane_of[j] = rem != 0ull ? static_cast<int>(__builtin_ctzll(rem)) : -1;
            rem &= rem - 1ull;                              // (no-op once empty)
        }
        u32x4 vals[kGroup][kVPT];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (lane_of[j] >= 0) {
                const int32_t sj = __builtin_amdgcn_readlane(my_slot, lane_of[j]);
                const u32x4* row = reinterpret_cast<const u32x4*>(p.src + static_cast<int64_t>(sj) * p.src_stride);
#pragma unroll
                for (int v = 0; v < kVPT; ++v)
                    vals[j][v] = vok[v] ? load16<true>(row + vidx[v]) : (u32x4){0u, 0u, 0u, 0u};
            }
        }
        if (copy_row) {
#pragma unroll
            for (int v = 0; v < kVPT; ++v) result[v] = vals[0][v];        // n == 1: lane_of[0] is it
        } else {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                if (lane_of[j] >= 0) {
                    if constexpr (kWeighted) {
                        const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), lane_of[j]));
#pragma unroll
                        for (int v = 0; v < kVPT; ++v) acc_fma(acc[v], vals[j][v], w);
                    } else {
#pragma unroll
                        for (int v = 0; v < kVPT; ++v) acc_add(acc[v], vals[j][v]);
                    }
                }
            }
        }
    }
    if (!copy_row) {
#pragma unroll
        for (int v = 0; v < kVPT; ++v) result[v] = acc_pack(acc[v]);
    }

    // ---- the encode of the rounded row (logfmt.hip's encode_row over registers) and the wire row's stores
    const int coded = p.hidden + p.hidden / 4 + p.hidden / 32;
    const __amdgpu_buffer_rsrc_t orow = row_rsrc(out_row, coded);
#pragma unroll
    for (int v = 0; v < kVPT; ++v) {
        const u32x4 raw = vok[v] ? result[v] : (u32x4){0u, 0u, 0u, 0u};      // past the row end: zeros
        uint32_t amax = 0u, amin = 0x7fffu;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t m = deepep::lf_magnitude((raw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
            amax = max(amax, m);
            amin = min(amin, m);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), off, 64)));
            amin = min(amin, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amin), off, 64)));
        }
        const uint32_t word = amax | amin << 16;
        deepep::lf_u32x2 lo;
        uint32_t hi;
        deepep::lf_encode8(raw, deepep::lf_group(word), lo, hi);
        // the descriptor spans all three planes, so the row end is tested here: a lane past it would land in the
        // high plane
        if (vok[v]) {
            __builtin_amdgcn_raw_buffer_store_b64(lo, orow, vidx[v] * 8, 0, kAuxSys);
            __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(hi), orow, p.hidden + vidx[v] * 2, 0, kAuxSys);
            if ((lane & 15) == 0)
                __builtin_amdgcn_raw_buffer_store_b32(word, orow, p.hidden * 5 / 4 + (vidx[v] >> 4) * 4, 0, kAuxSys);
        }
    }
    if (wlane) store_weight(p, u, reinterpret_cast<uint16_t*>(out_row), lane, wv);
}

// combine_rows_kernel's staging in the scatter's 4-wave workgroups, then combine_item_scatter_logfmt.
template <bool kWeighted, int kVPT, int kGroup>
__global__ void __launch_bounds__(64 * 4)
combine_scatter_logfmt_kernel(const Params p) {
    constexpr int kWaves = 4;
    constexpr int kChunkVecs = 64 * kVPT;
    __shared__ int32_t s_slot[kWaves][kMaxWidth];
    __shared__ float s_w[kWaves][kMaxWidth];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int nvec = p.hidden >> 3;
    const int nchunks = (nvec + kChunkVecs - 1) / kChunkVecs;
    const int64_t items = static_cast<int64_t>(p.num_units) * nchunks;
    const int width = p.table == nullptr ? 1 : p.table_width;
    const int64_t it0 = static_cast<int64_t>(blockIdx.x) * kWaves;
    const int64_t it = it0 + wave;
    const int64_t u_first = it0 / nchunks;
    const int nu = static_cast<int>(min(it0 + kWaves - 1, items - 1) / nchunks - u_first) + 1;
    if (tid < nu * width) {                                  // nu * width <= kWaves * 32 threads
        const int ul = tid / width, j = tid - ul * width;
        const int64_t u = u_first + ul;
        int32_t s = p.table == nullptr ? static_cast<int32_t>(u) : p.table[u * p.table_stride + j];
        if (s >= p.num_src_rows) {                           // never dereference a bad slot
            if (p.error_flag != nullptr) atomicOr(p.error_flag, DEEPEP_FLAG_BAD_SLOT);
            s = -1;
        }
        s_slot[ul][j] = s;
        if constexpr (kWeighted) s_w[ul][j] = s >= 0 ? p.row_weights[s] : 0.0f;
    }
    __syncthreads();
    if (it >= items) return;
    int32_t my_slot = -1;
    float my_w = 0.0f;
    if (lane < width) {
        const int ul = static_cast<int>(it / nchunks - u_first);
        my_slot = s_slot[ul][lane];
        if constexpr (kWeighted) my_w = s_w[ul][lane];
    }
    combine_item_scatter_logfmt<kWeighted, kVPT, kGroup>(p, it, nchunks, nvec, lane, my_slot, my_w);
}

// CU-budget streams created by deepep_stream_create_cu_budget (symmetric.hip) and their CU counts: a
// launch on one keeps its full grid (the CU mask alone holds it to the budget) with at most 4 rows in
// flight per lane -- 64 VGPRs, 8 waves per SIMD, more bytes in flight per budgeted CU than 8 rows at 5
// waves (config 2: 128 CUs 208 vs 235 us, 32 CUs 603 vs 661 us, profiles/archive/r02n_kcu2.jsonl).
std::mutex g_budget_mutex;
std::map<hipStream_t, int> g_budget_cus;

int budget_cus_of(hipStream_t s) {
    if (s == nullptr) return 0;
    std::lock_guard<std::mutex> lock(g_budget_mutex);
    const auto it = g_budget_cus.find(s);
    return it == g_budget_cus.end() ? 0 : it->second;
}

// The one tuning knob left (diagnostics; deepep_set_launch_config): vectors per lane (bits 0-3) and rows
// in flight (bits 4-7), 0 = automatic.  One atomic word, read once per launch, so a launch never sees
// half of another thread's update.
std::atomic<uint32_t> g_launch_config{0};

struct Shape {
    int vpt, waves, group;
};

template <int kMode, bool kWeighted, int kVPT, bool kFull, int kAux, int kWaves, int kFp8 = 0>
void launch_group(const Params& p, int group, hipStream_t stream) {
    const int nvec = p.hidden / (kFp8 == 16 ? 16 : 8);
    const int64_t items = static_cast<int64_t>(p.num_units) * ((nvec + 64 * kVPT - 1) / (64 * kVPT));
    const dim3 grid(static_cast<unsigned>((items + kWaves - 1) / kWaves)), block(64 * kWaves);
    if (group == 2)
        hipLaunchKernelGGL((combine_rows_kernel<kMode, kWeighted, kVPT, kFull, kAux, kWaves, 2, kFp8>), grid, block, 0, stream, p);
    else if (group == 4)
        hipLaunchKernelGGL((combine_rows_kernel<kMode, kWeighted, kVPT, kFull, kAux, kWaves, 4, kFp8>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((combine_rows_kernel<kMode, kWeighted, kVPT, kFull, kAux, kWaves, 8, kFp8>), grid, block, 0, stream, p);
}

// The FP8 source's instantiations: what launch_combine can select plus what the diagnostics knob sweeps, and
// no more (each one is built and shipped).  There is no whole-chunk (kFull) variant -- the row-end test is one
// compare per vector of a kernel that waits on HBM -- and the workgroup size follows units_per_block only
// where it is swept (the fused reduce and phase A into local rows); the epilogue keeps 8 waves and the
// scatter into peer windows 4.  72 kernels against the bf16 source's 192.
// kLoad: 8-byte loads everywhere.  With 16-byte loads a lane stores two adjacent 16-byte vectors, so one store
// instruction covers every other 16 bytes of its lines: under phase A's streaming write-through policy that cost
// 635 us against 245 us at EP = 8's phase-A shape, and 131 us against 107 us in the fused reduce of config 2
// (CHANGELOG.md has both sweeps).
template <int kMode, bool kWeighted, int kAux>
void launch_shape_fp8(const Params& p, const Shape& sh, hipStream_t stream) {
    constexpr bool kSwept = kMode == DEEPEP_MODE_FUSED || (kMode == DEEPEP_MODE_LOCAL && kAux != kAuxSys);
    constexpr int kFixed = kMode == DEEPEP_MODE_LOCAL ? 4 : 8;
    constexpr int kOther = kSwept ? 12 - kFixed : kFixed;
    constexpr int kLoad = 8;                             // the FP8 bytes a lane loads per vector
#define DEEPEP_WAVES(VPT)                                                                                    \
    (sh.waves == kFixed ? launch_group<kMode, kWeighted, VPT, false, kAux, kFixed, kLoad>(p, sh.group, stream) \
                        : launch_group<kMode, kWeighted, VPT, false, kAux, kOther, kLoad>(p, sh.group, stream))
    if (sh.vpt == 1) DEEPEP_WAVES(1);
    else DEEPEP_WAVES(2);
#undef DEEPEP_WAVES
}

template <int kMode, bool kWeighted, int kAux>
void launch_shape(const Params& p, const Shape& sh, hipStream_t stream) {
    if (p.sf != nullptr) return launch_shape_fp8<kMode, kWeighted, kAux>(p, sh, stream);
    const int nvec = p.hidden / 8;
#define DEEPEP_WAVES(VPT, FULL)                                                            \
    (sh.waves == 4 ? launch_group<kMode, kWeighted, VPT, FULL, kAux, 4>(p, sh.group, stream) \
                   : launch_group<kMode, kWeighted, VPT, FULL, kAux, 8>(p, sh.group, stream))
    if (sh.vpt == 1) {
        if (nvec % 64 == 0) DEEPEP_WAVES(1, true);
        else DEEPEP_WAVES(1, false);
    } else {
        if (nvec % 128 == 0) DEEPEP_WAVES(2, true);
        else DEEPEP_WAVES(2, false);
    }
#undef DEEPEP_WAVES
}

// The LogFMT source's instantiations: the epilogue shapes the FP8 source ships (8 waves, 1 or 2 vectors per lane,
// 2 / 4 / 8 rows in flight), weighted and not: 12 kernels.
template <bool kWeighted, int kVPT>
void launch_group_logfmt(const Params& p, int group, hipStream_t stream) {
    const int nvec = p.hidden / 8;
    const int64_t items = static_cast<int64_t>(p.num_units) * ((nvec + 64 * kVPT - 1) / (64 * kVPT));
    const dim3 grid(static_cast<unsigned>((items + 7) / 8)), block(64 * 8);
    if (group == 2)
        hipLaunchKernelGGL((combine_rows_logfmt_kernel<kWeighted, kVPT, kAuxSC1, 2>), grid, block, 0, stream, p);
    else if (group == 4)
        hipLaunchKernelGGL((combine_rows_logfmt_kernel<kWeighted, kVPT, kAuxSC1, 4>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((combine_rows_logfmt_kernel<kWeighted, kVPT, kAuxSC1, 8>), grid, block, 0, stream, p);
}

template <bool kWeighted>
void launch_shape_logfmt(const Params& p, const Shape& sh, hipStream_t stream) {
    if (sh.vpt == 1) launch_group_logfmt<kWeighted, 1>(p, sh.group, stream);
    else launch_group_logfmt<kWeighted, 2>(p, sh.group, stream);
}

// The LogFMT scatter's instantiations: the scatter's shape (4 waves, 1 or 2 vectors per lane, 2 / 4 rows in flight),
// weighted and not: 8 kernels.
template <bool kWeighted, int kVPT>
void launch_group_scatter_logfmt(const Params& p, int group, hipStream_t stream) {
    const int nvec = p.hidden / 8;
    const int64_t items = static_cast<int64_t>(p.num_units) * ((nvec + 64 * kVPT - 1) / (64 * kVPT));
    const dim3 grid(static_cast<unsigned>((items + 3) / 4)), block(64 * 4);
    if (group == 2)
        hipLaunchKernelGGL((combine_scatter_logfmt_kernel<kWeighted, kVPT, 2>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((combine_scatter_logfmt_kernel<kWeighted, kVPT, 4>), grid, block, 0, stream, p);
}

template <bool kWeighted>
void launch_shape_scatter_logfmt(const Params& p, const Shape& sh, hipStream_t stream) {
    if (sh.vpt == 1) launch_group_scatter_logfmt<kWeighted, 1>(p, sh.group, stream);
    else launch_group_scatter_logfmt<kWeighted, 2>(p, sh.group, stream);
}

bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

// ---------------------------------------------------------------- plan builder
__global__ void fill_kernel(int32_t* dst, int64_t n, int32_t value) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        dst[i] = value;
}

__global__ void local_plan_kernel(const int32_t* meta, int num_recv, int num_topk, int t_max, int expanded,
                                  int32_t* plan, int plan_width, int num_tokens,
                                  const int64_t* topk_idx, int32_t* wtable) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_recv) return;
    const int stride = num_topk + 2;
    const int t = meta[static_cast<int64_t>(i) * stride] % t_max;
    if (t < 0 || t >= num_tokens) return;
    if (expanded) {
        for (int k = 0; k < plan_width; ++k)
            plan[static_cast<int64_t>(t) * plan_width + k] = meta[static_cast<int64_t>(i) * stride + 2 + k];
    } else {
        plan[static_cast<int64_t>(t) * plan_width] = i;
    }
    if (wtable != nullptr)
        for (int k = 0; k < num_topk; ++k)
            wtable[static_cast<int64_t>(t) * num_topk + k] =
                topk_idx[static_cast<int64_t>(t) * num_topk + k] >= 0 ? i * num_topk + k : -1;
}

int launch_combine(int mode, int weighted, const Params& p, deepep_stream_t stream);

// The scale factors of an FP8 source (the *_fp8 entries), or none.
struct Fp8Source {
    const void* sf;
    int64_t row_stride, col_stride;
    int packed;
};

// What the *_fp8 entries require on top of their siblings' checks (src_row_stride counts e4m3fn elements).
int check_fp8_source(const void* src, int64_t src_row_stride, int hidden, const Fp8Source& f) {
    if (hidden % 128 != 0 || (f.packed && hidden % 512 != 0))
        return set_error(DEEPEP_ERR_INVALID_ARG, "an FP8 source needs hidden (%d) to be a multiple of 128 (512 with packed UE8M0 scale factors)", hidden);
    if (f.sf == nullptr || (reinterpret_cast<uintptr_t>(f.sf) & 3u) != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "an FP8 source needs 4-byte aligned scale factors");
    if (!aligned16(src))
        return set_error(DEEPEP_ERR_INVALID_ARG, "an FP8 source must be 16-byte aligned");
    if (src_row_stride % 16 != 0 || src_row_stride < hidden)
        return set_error(DEEPEP_ERR_INVALID_ARG, "an FP8 source's row stride must be >= hidden and a multiple of 16 elements");
    return DEEPEP_OK;
}

void set_fp8_source(Params& p, const Fp8Source* f) {
    p.sf = f != nullptr ? f->sf : nullptr;
    p.sf_row_stride = f != nullptr ? f->row_stride : 0;
    p.sf_col_stride = f != nullptr ? f->col_stride : 0;
    p.sf_packed = f != nullptr ? f->packed : 0;
}

int combine_reduce_impl(int mode, int weighted,
                        const void* src, int64_t num_src_rows, int64_t src_row_stride,
                        const int32_t* table, int64_t table_stride, int table_width,
                        const float* row_weights,
                        const void* bias0, const void* bias1,
                        void* out, int64_t out_row_stride,
                        int num_units, int hidden,
                        const int32_t* wtable, int64_t wtable_stride,
                        const float* wsrc, float* out_weights, int num_weights,
                        int64_t out_weights_stride, int weights_pad,
                        int units_per_block, int32_t* error_flag,
                        deepep_stream_t stream, const Fp8Source* fp8);

int combine_reduce_scatter_impl(int weighted,
                                const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                const int32_t* table, int64_t table_stride, int table_width,
                                const float* row_weights,
                                const uint64_t* out_rows, int num_units, int hidden,
                                const int32_t* wtable, int64_t wtable_stride,
                                const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                int32_t* error_flag, deepep_stream_t stream, const Fp8Source* fp8);

}  // namespace

extern "C" {

// Error reporting shared with dispatch.hip (not part of the public C-ABI).
__attribute__((visibility("hidden"))) int deepep_amd_set_error(int code, const char* msg) {
    return set_error(code, "%s", msg);
}

// Budget streams (shared with symmetric.hip; not part of the public C-ABI): cus <= 0 forgets one.
__attribute__((visibility("hidden"))) void deepep_amd_register_budget(void* stream, int cus) {
    std::lock_guard<std::mutex> lock(g_budget_mutex);
    if (cus > 0) g_budget_cus[static_cast<hipStream_t>(stream)] = cus;
    else g_budget_cus.erase(static_cast<hipStream_t>(stream));
}

int deepep_amd_abi_version(void) { return DEEPEP_AMD_ABI_VERSION; }

#ifndef DEEPEP_BUILD_ID
#define DEEPEP_BUILD_ID "unknown-build-id"
#endif
// The build id (hash of sources, header and flags, deepep_amd/_lib.py) stored with a marker so that
// it can be read from the file without loading it.
__attribute__((used)) static const char g_build_id[] = "DEEPEP_BUILD_ID=" DEEPEP_BUILD_ID;
const char* deepep_amd_build_id(void) { return g_build_id + 16; }

const char* deepep_amd_last_error(void) { return g_last_error; }

int deepep_combine_reduce(int mode, int weighted,
                          const void* src, int64_t num_src_rows, int64_t src_row_stride,
                          const int32_t* table, int64_t table_stride, int table_width,
                          const float* row_weights,
                          const void* bias0, const void* bias1,
                          void* out, int64_t out_row_stride,
                          int num_units, int hidden,
                          const int32_t* wtable, int64_t wtable_stride,
                          const float* wsrc, float* out_weights, int num_weights,
                          int64_t out_weights_stride, int weights_pad,
                          int units_per_block, int32_t* error_flag,
                          deepep_stream_t stream) {
    return combine_reduce_impl(mode, weighted, src, num_src_rows, src_row_stride, table, table_stride, table_width,
                               row_weights, bias0, bias1, out, out_row_stride, num_units, hidden, wtable, wtable_stride,
                               wsrc, out_weights, num_weights, out_weights_stride, weights_pad, units_per_block,
                               error_flag, stream, nullptr);
}

int deepep_combine_reduce_fp8(int mode, int weighted,
                              const void* src, int64_t num_src_rows, int64_t src_row_stride,
                              const void* sf, int64_t sf_row_stride, int64_t sf_col_stride, int sf_packed,
                              const int32_t* table, int64_t table_stride, int table_width,
                              const float* row_weights,
                              const void* bias0, const void* bias1,
                              void* out, int64_t out_row_stride,
                              int num_units, int hidden,
                              const int32_t* wtable, int64_t wtable_stride,
                              const float* wsrc, float* out_weights, int num_weights,
                              int64_t out_weights_stride, int weights_pad,
                              int units_per_block, int32_t* error_flag,
                              deepep_stream_t stream) {
    const Fp8Source fp8 = {sf, sf_row_stride, sf_col_stride, sf_packed != 0};
    return combine_reduce_impl(mode, weighted, src, num_src_rows, src_row_stride, table, table_stride, table_width,
                               row_weights, bias0, bias1, out, out_row_stride, num_units, hidden, wtable, wtable_stride,
                               wsrc, out_weights, num_weights, out_weights_stride, weights_pad, units_per_block,
                               error_flag, stream, &fp8);
}

int deepep_combine_reduce_scatter(int weighted,
                                  const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                  const int32_t* table, int64_t table_stride, int table_width,
                                  const float* row_weights,
                                  const uint64_t* out_rows, int num_units, int hidden,
                                  const int32_t* wtable, int64_t wtable_stride,
                                  const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                  const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                  int32_t* error_flag, deepep_stream_t stream) {
    return combine_reduce_scatter_impl(weighted, src, num_src_rows, src_row_stride, table, table_stride, table_width,
                                       row_weights, out_rows, num_units, hidden, wtable, wtable_stride, wsrc,
                                       num_weights, weights_offset, weights_pad, window_bases, num_windows,
                                       window_bytes, error_flag, stream, nullptr);
}

int deepep_combine_reduce_scatter_fp8(int weighted,
                                      const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                      const void* sf, int64_t sf_row_stride, int64_t sf_col_stride, int sf_packed,
                                      const int32_t* table, int64_t table_stride, int table_width,
                                      const float* row_weights,
                                      const uint64_t* out_rows, int num_units, int hidden,
                                      const int32_t* wtable, int64_t wtable_stride,
                                      const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                      const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                      int32_t* error_flag, deepep_stream_t stream) {
    const Fp8Source fp8 = {sf, sf_row_stride, sf_col_stride, sf_packed != 0};
    return combine_reduce_scatter_impl(weighted, src, num_src_rows, src_row_stride, table, table_stride, table_width,
                                       row_weights, out_rows, num_units, hidden, wtable, wtable_stride, wsrc,
                                       num_weights, weights_offset, weights_pad, window_bases, num_windows,
                                       window_bytes, error_flag, stream, &fp8);
}

}  // extern "C"

namespace {

int combine_reduce_impl(int mode, int weighted,
                        const void* src, int64_t num_src_rows, int64_t src_row_stride,
                        const int32_t* table, int64_t table_stride, int table_width,
                        const float* row_weights,
                        const void* bias0, const void* bias1,
                        void* out, int64_t out_row_stride,
                        int num_units, int hidden,
                        const int32_t* wtable, int64_t wtable_stride,
                        const float* wsrc, float* out_weights, int num_weights,
                        int64_t out_weights_stride, int weights_pad,
                        int units_per_block, int32_t* error_flag,
                        deepep_stream_t stream, const Fp8Source* fp8) {
    if (mode < DEEPEP_MODE_LOCAL || mode > DEEPEP_MODE_FUSED)
        return set_error(DEEPEP_ERR_INVALID_ARG, "invalid mode %d", mode);
    if (num_units < 0 || hidden < 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "negative size (num_units=%d, hidden=%d)", num_units, hidden);
    if (num_units == 0) return DEEPEP_OK;
    if (fp8 != nullptr && check_fp8_source(src, src_row_stride, hidden, *fp8) != DEEPEP_OK) return DEEPEP_ERR_INVALID_ARG;
    if (hidden % 8 != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "hidden (%d) * sizeof(bf16) must be a multiple of 16 bytes", hidden);
    if (out == nullptr || (hidden > 0 && src == nullptr && num_src_rows > 0))
        return set_error(DEEPEP_ERR_INVALID_ARG, "null src/out");
    if (!aligned16(src) || !aligned16(out) || !aligned16(bias0) || !aligned16(bias1))
        return set_error(DEEPEP_ERR_INVALID_ARG, "src/out/bias must be 16-byte aligned");
    if (src_row_stride % 8 != 0 || out_row_stride % 8 != 0 || src_row_stride < hidden || out_row_stride < hidden)
        return set_error(DEEPEP_ERR_INVALID_ARG, "row strides must be >= hidden and multiples of 8 elements");
    if (table != nullptr && (table_width < 1 || table_width > kMaxWidth || table_stride < table_width))
        return set_error(DEEPEP_ERR_INVALID_ARG, "table width %d outside [1, %d] or stride too small", table_width, kMaxWidth);
    if (weighted && row_weights == nullptr)
        return set_error(DEEPEP_ERR_INVALID_ARG, "weighted reduction needs row weights");
    if (mode == DEEPEP_MODE_LOCAL && (bias0 != nullptr || bias1 != nullptr))
        return set_error(DEEPEP_ERR_INVALID_ARG, "bias is applied by the epilogue, not the local reduce");
    if (out_weights != nullptr && (wsrc == nullptr || num_weights < 1 || num_weights > kMaxWidth))
        return set_error(DEEPEP_ERR_INVALID_ARG, "weight pass-through needs wsrc and 1 <= num_weights <= %d", kMaxWidth);
    if (out_weights_stride == 0) out_weights_stride = num_weights;
    if (weights_pad < num_weights) weights_pad = num_weights;
    if (out_weights != nullptr && (out_weights_stride < weights_pad || weights_pad > 64))
        return set_error(DEEPEP_ERR_INVALID_ARG, "out_weights_stride (%lld) < weights_pad (%d) or weights_pad > 64",
                         static_cast<long long>(out_weights_stride), weights_pad);
    Params p;
    p.src = static_cast<const uint16_t*>(src);
    p.num_src_rows = num_src_rows;
    p.src_stride = src_row_stride;
    p.table = table;
    p.table_stride = table_stride;
    p.table_width = table_width;
    p.row_weights = row_weights;
    p.bias0 = static_cast<const uint16_t*>(bias0);
    p.bias1 = static_cast<const uint16_t*>(bias1);
    p.out = static_cast<uint16_t*>(out);
    p.out_stride = out_row_stride;
    p.num_units = num_units;
    p.hidden = hidden;
    p.wtable = wtable;
    p.wtable_stride = wtable_stride;
    p.wsrc = wsrc;
    p.out_weights = out_weights;
    p.num_weights = out_weights != nullptr ? num_weights : 0;
    p.weights_pad = weights_pad;
    p.out_weights_stride = out_weights_stride;
    p.units_per_block = units_per_block;
    p.error_flag = error_flag;
    p.out_rows = nullptr;
    p.weights_offset = 0;
    p.win_bases = nullptr;
    p.win_count = 0;
    p.win_limit = 0;
    set_fp8_source(p, fp8);

    return launch_combine(mode, weighted, p, stream);
}

int combine_reduce_scatter_impl(int weighted,
                                const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                const int32_t* table, int64_t table_stride, int table_width,
                                const float* row_weights,
                                const uint64_t* out_rows, int num_units, int hidden,
                                const int32_t* wtable, int64_t wtable_stride,
                                const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                int32_t* error_flag, deepep_stream_t stream, const Fp8Source* fp8) {
    if (num_units < 0 || hidden < 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "negative size (num_units=%d, hidden=%d)", num_units, hidden);
    if (num_units == 0) return DEEPEP_OK;
    if (fp8 != nullptr && check_fp8_source(src, src_row_stride, hidden, *fp8) != DEEPEP_OK) return DEEPEP_ERR_INVALID_ARG;
    if (hidden % 8 != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "hidden (%d) * sizeof(bf16) must be a multiple of 16 bytes", hidden);
    if (out_rows == nullptr || (src == nullptr && num_src_rows > 0) || !aligned16(src))
        return set_error(DEEPEP_ERR_INVALID_ARG, "null out_rows / unaligned src");
    if (src_row_stride % 8 != 0 || src_row_stride < hidden)
        return set_error(DEEPEP_ERR_INVALID_ARG, "src row stride must be >= hidden and a multiple of 8 elements");
    if (table != nullptr && (table_width < 1 || table_width > kMaxWidth || table_stride < table_width))
        return set_error(DEEPEP_ERR_INVALID_ARG, "table width %d outside [1, %d] or stride too small", table_width, kMaxWidth);
    if (weighted && row_weights == nullptr)
        return set_error(DEEPEP_ERR_INVALID_ARG, "weighted reduction needs row weights");
    if (num_weights > 0 && (wsrc == nullptr || num_weights > kMaxWidth || weights_offset < int64_t(hidden) * 2 ||
                            weights_offset % 4 != 0))
        return set_error(DEEPEP_ERR_INVALID_ARG, "weights need wsrc, num_weights <= %d and an offset past the row", kMaxWidth);
    if (weights_pad < num_weights) weights_pad = num_weights;
    if (weights_pad > 64) return set_error(DEEPEP_ERR_INVALID_ARG, "weights_pad > 64");
    // the bytes one unit stores: the bf16 row, then (with weights) weights_pad floats at weights_offset
    const int64_t row_extent = num_weights > 0 ? std::max<int64_t>(int64_t(hidden) * 2, weights_offset + 4 * weights_pad)
                                               : int64_t(hidden) * 2;
    if (window_bases == nullptr || num_windows < 1 || num_windows > 64 || window_bytes < row_extent)
        return set_error(DEEPEP_ERR_INVALID_ARG, "scatter needs 1..64 windows of at least one row (%lld bytes)",
                         static_cast<long long>(row_extent));
    Params p;
    p.src = static_cast<const uint16_t*>(src);
    p.num_src_rows = num_src_rows;
    p.src_stride = src_row_stride;
    p.table = table;
    p.table_stride = table_stride;
    p.table_width = table_width;
    p.row_weights = row_weights;
    p.bias0 = nullptr;
    p.bias1 = nullptr;
    p.out = nullptr;
    p.out_stride = 0;
    p.num_units = num_units;
    p.hidden = hidden;
    p.wtable = wtable;
    p.wtable_stride = wtable_stride;
    p.wsrc = wsrc;
    p.out_weights = nullptr;
    p.num_weights = num_weights > 0 ? num_weights : 0;
    p.weights_pad = weights_pad;
    p.out_weights_stride = 0;
    p.units_per_block = 0;
    p.error_flag = error_flag;
    p.out_rows = out_rows;
    p.weights_offset = weights_offset;
    p.win_bases = window_bases;
    p.win_count = num_windows;
    p.win_limit = static_cast<uint64_t>(window_bytes - row_extent);
    set_fp8_source(p, fp8);
    return launch_combine(DEEPEP_MODE_LOCAL, weighted, p, stream);
}

int launch_combine(int mode, int weighted, const Params& p, deepep_stream_t stream) {
    // Launch shape: one wave per (unit, 64 x vpt x 16-byte column chunk) item, `waves` items per
    // workgroup, `group` source rows loaded per lane before any is accumulated.  Measured per shape
    // class (launch-shape sweeps of rounds 2-4: DESIGN.md section 3, CHANGELOG.md):
    //   fused reduce over top-k >= 5, rows >= 256 vectors: 1 KiB chunks, 2 rows, 4 waves -- few registers,
    //     many waves (config 2: -0.9 to -1.6 % against 2 KiB / 8 rows / 8 waves on three boxes);
    //   fused over top-k >= 5, rows of 128-255 vectors: 2 KiB chunks, 4 rows, 8 waves;
    //   epilogue (phase B) and the other fused shapes: 2 KiB chunks, 8 rows, 8 waves;
    //   phase A (LOCAL, ~1.5 local rows per received token at EP = 8): 2 KiB chunks, 4 rows, 4 waves
    //     (64 VGPRs, 8 waves per SIMD; 1 KiB chunks lose there, 297-330 vs 249.6 us);
    // rows in flight are capped at the slot table's width rounded up to 2 / 4 (top-2: 33.7 vs 40.1 us),
    // and at 4 on a CU-budget stream.
    const uint32_t cfg = g_launch_config.load(std::memory_order_relaxed);
    const int cfg_vpt = static_cast<int>(cfg & 15u), cfg_rows = static_cast<int>((cfg >> 4) & 15u);
    const int nvec = p.hidden / 8;
    const int width = p.table == nullptr ? 1 : p.table_width;
    const int width_cap = width <= 2 ? 2 : (width <= 4 ? 4 : 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int budget = budget_cus_of(s);
    Shape sh;
    sh.vpt = nvec >= 128 ? 2 : 1;
    sh.waves = mode == DEEPEP_MODE_LOCAL ? 4 : 8;
    sh.group = std::min(mode == DEEPEP_MODE_LOCAL || budget > 0 ? 4 : 8, width_cap);
    const bool automatic = cfg == 0 && p.units_per_block == 0 && budget == 0;
    if (automatic && mode == DEEPEP_MODE_FUSED && width >= 5 && nvec >= 256) {
        sh.vpt = 1;
        sh.group = 2;
        sh.waves = 4;
    } else if (automatic && mode == DEEPEP_MODE_FUSED && width >= 5 && nvec >= 128) {
        sh.group = 4;
    }
    if (automatic && p.sf != nullptr) {
        // an FP8 source halves the bytes a lane has in flight per row: the sweep at config 2 and at EP = 8's phase A
        // (CHANGELOG.md) puts 2 vectors per lane and 2 rows in flight in 4-wave workgroups first in both
        if (mode == DEEPEP_MODE_FUSED && width >= 5 && nvec >= 256) sh.vpt = 2;
        if (mode == DEEPEP_MODE_LOCAL) sh.group = 2;
    }
    if (cfg_vpt != 0) sh.vpt = cfg_vpt;
    if (cfg_rows != 0) sh.group = cfg_rows;
    if (p.units_per_block == 4 || p.units_per_block == 8) sh.waves = p.units_per_block;

#define DEEPEP_POLICY(M, AUX) \
    (weighted ? launch_shape<M, true, AUX>(p, sh, s) : launch_shape<M, false, AUX>(p, sh, s))
    if (mode == DEEPEP_MODE_LOCAL && p.out_rows != nullptr) DEEPEP_POLICY(DEEPEP_MODE_LOCAL, kAuxSys);
    else if (mode == DEEPEP_MODE_LOCAL) DEEPEP_POLICY(DEEPEP_MODE_LOCAL, kAuxSC1NT);
    else if (mode == DEEPEP_MODE_EPILOGUE) DEEPEP_POLICY(DEEPEP_MODE_EPILOGUE, kAuxSC1);
    else DEEPEP_POLICY(DEEPEP_MODE_FUSED, kAuxSC1);
#undef DEEPEP_POLICY
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return set_error(DEEPEP_ERR_HIP, "combine launch failed: %s", hipGetErrorString(err));
    return DEEPEP_OK;
}

}  // namespace

extern "C" {

int deepep_build_local_plan(const int32_t* src_metadata, int num_recv_tokens, int num_topk,
                            int num_max_tokens_per_rank, int expanded,
                            int32_t* plan, int plan_width, int num_tokens,
                            const int64_t* topk_idx, int32_t* wtable,
                            deepep_stream_t stream) {
    if (num_recv_tokens < 0 || num_tokens < 0 || num_topk < 1 || num_topk > kMaxWidth || num_max_tokens_per_rank < 1)
        return set_error(DEEPEP_ERR_INVALID_ARG, "invalid plan sizes");
    if ((num_tokens > 0 && plan == nullptr) || (num_recv_tokens > 0 && src_metadata == nullptr))
        return set_error(DEEPEP_ERR_INVALID_ARG, "null plan/metadata");
    if (plan_width != (expanded ? num_topk : 1))
        return set_error(DEEPEP_ERR_INVALID_ARG, "plan width must be num_topk (expanded) or 1");
    if (wtable != nullptr && topk_idx == nullptr)
        return set_error(DEEPEP_ERR_INVALID_ARG, "wtable needs topk_idx");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_plan = static_cast<int64_t>(num_tokens) * plan_width;
    if (n_plan > 0)
        hipLaunchKernelGGL(fill_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((n_plan + 255) / 256, 1024))), dim3(256), 0, s,
                           plan, n_plan, -1);
    if (wtable != nullptr && num_tokens > 0) {
        const int64_t n_w = static_cast<int64_t>(num_tokens) * num_topk;
        hipLaunchKernelGGL(fill_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((n_w + 255) / 256, 1024))), dim3(256), 0, s,
                           wtable, n_w, -1);
    }
    if (num_recv_tokens > 0)
        hipLaunchKernelGGL(local_plan_kernel, dim3((num_recv_tokens + 255) / 256), dim3(256), 0, s,
                           src_metadata, num_recv_tokens, num_topk, num_max_tokens_per_rank, expanded,
                           plan, plan_width, num_tokens, topk_idx, wtable);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return set_error(DEEPEP_ERR_HIP, "plan launch failed: %s", hipGetErrorString(err));
    return DEEPEP_OK;
}

int deepep_set_launch_config(int vec_per_lane, int rows_in_flight) {
    if (vec_per_lane < 0 || vec_per_lane > 2 ||
        (rows_in_flight != 0 && rows_in_flight != 2 && rows_in_flight != 4 && rows_in_flight != 8))
        return set_error(DEEPEP_ERR_INVALID_ARG, "invalid launch configuration (vec_per_lane 0-2, rows_in_flight 0/2/4/8)");
    g_launch_config.store(static_cast<uint32_t>(vec_per_lane) | (static_cast<uint32_t>(rows_in_flight) << 4),
                          std::memory_order_relaxed);
    return DEEPEP_OK;
}

int deepep_combine_reduce_logfmt(int weighted,
                                 const void* src, int64_t num_src_rows, int64_t src_row_stride_bytes,
                                 const int32_t* meta, int64_t meta_row_stride,
                                 const int32_t* table, int64_t table_stride, int table_width,
                                 const float* row_weights,
                                 const void* bias0, const void* bias1,
                                 void* out, int64_t out_row_stride,
                                 int num_units, int hidden,
                                 const int32_t* wtable, int64_t wtable_stride,
                                 const float* wsrc, float* out_weights, int num_weights,
                                 int64_t out_weights_stride, int weights_pad,
                                 int32_t* error_flag, deepep_stream_t stream) {
    if (num_units < 0 || hidden < 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "negative size (num_units=%d, hidden=%d)", num_units, hidden);
    if (num_units == 0) return DEEPEP_OK;
    if (hidden < 128 || hidden % 128 != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "a LogFMT source needs hidden (%d) to be a positive multiple of 128", hidden);
    if (out == nullptr || (src == nullptr && num_src_rows > 0) || (meta == nullptr && num_src_rows > 0))
        return set_error(DEEPEP_ERR_INVALID_ARG, "null src/meta/out");
    if (!aligned16(src) || !aligned16(out) || !aligned16(bias0) || !aligned16(bias1) ||
        (reinterpret_cast<uintptr_t>(meta) & 3u) != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "src/out/bias must be 16-byte aligned, meta 4-byte aligned");
    if (src_row_stride_bytes % 16 != 0 || src_row_stride_bytes < static_cast<int64_t>(hidden) + hidden / 4 ||
        meta_row_stride < hidden / 128)
        return set_error(DEEPEP_ERR_INVALID_ARG, "a LogFMT source's row stride must be >= hidden * 5 / 4 bytes and a multiple of 16, its meta row stride >= hidden / 128");
    if (out_row_stride % 8 != 0 || out_row_stride < hidden)
        return set_error(DEEPEP_ERR_INVALID_ARG, "row strides must be >= hidden and multiples of 8 elements");
    if (table != nullptr && (table_width < 1 || table_width > kMaxWidth || table_stride < table_width))
        return set_error(DEEPEP_ERR_INVALID_ARG, "table width %d outside [1, %d] or stride too small", table_width, kMaxWidth);
    if (weighted && row_weights == nullptr)
        return set_error(DEEPEP_ERR_INVALID_ARG, "weighted reduction needs row weights");
    if (out_weights != nullptr && (wsrc == nullptr || num_weights < 1 || num_weights > kMaxWidth))
        return set_error(DEEPEP_ERR_INVALID_ARG, "weight pass-through needs wsrc and 1 <= num_weights <= %d", kMaxWidth);
    if (out_weights_stride == 0) out_weights_stride = num_weights;
    if (weights_pad < num_weights) weights_pad = num_weights;
    if (out_weights != nullptr && (out_weights_stride < weights_pad || weights_pad > 64))
        return set_error(DEEPEP_ERR_INVALID_ARG, "out_weights_stride (%lld) < weights_pad (%d) or weights_pad > 64",
                         static_cast<long long>(out_weights_stride), weights_pad);
    Params p = {};
    p.src = static_cast<const uint16_t*>(src);
    p.num_src_rows = num_src_rows;
    p.src_stride = src_row_stride_bytes;
    p.table = table;
    p.table_stride = table_stride;
    p.table_width = table_width;
    p.row_weights = row_weights;
    p.bias0 = static_cast<const uint16_t*>(bias0);
    p.bias1 = static_cast<const uint16_t*>(bias1);
    p.out = static_cast<uint16_t*>(out);
    p.out_stride = out_row_stride;
    p.num_units = num_units;
    p.hidden = hidden;
    p.wtable = wtable;
    p.wtable_stride = wtable_stride;
    p.wsrc = wsrc;
    p.out_weights = out_weights;
    p.num_weights = out_weights != nullptr ? num_weights : 0;
    p.weights_pad = weights_pad;
    p.out_weights_stride = out_weights_stride;
    p.error_flag = error_flag;
    p.sf = meta;
    p.sf_row_stride = meta_row_stride;
    // the epilogue's launch shape (launch_combine): 2 KiB of bf16 output per chunk from 128 vectors on, 8 waves,
    // 8 rows in flight capped by the table's width (4 on a CU-budget stream); the diagnostics knob overrides
    const uint32_t cfg = g_launch_config.load(std::memory_order_relaxed);
    const int cfg_vpt = static_cast<int>(cfg & 15u), cfg_rows = static_cast<int>((cfg >> 4) & 15u);
    const int width = table == nullptr ? 1 : table_width;
    const int width_cap = width <= 2 ? 2 : (width <= 4 ? 4 : 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Shape sh;
    sh.vpt = hidden / 8 >= 128 ? 2 : 1;
    sh.waves = 8;
    sh.group = std::min(budget_cus_of(s) > 0 ? 4 : 8, width_cap);
    if (cfg_vpt != 0) sh.vpt = cfg_vpt;
    if (cfg_rows != 0) sh.group = cfg_rows;
    if (weighted) launch_shape_logfmt<true>(p, sh, s);
    else launch_shape_logfmt<false>(p, sh, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return set_error(DEEPEP_ERR_HIP, "combine launch failed: %s", hipGetErrorString(err));
    return DEEPEP_OK;
}

int deepep_combine_reduce_scatter_logfmt(int weighted,
                                         const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                         const int32_t* table, int64_t table_stride, int table_width,
                                         const float* row_weights,
                                         const uint64_t* out_rows, int num_units, int hidden,
                                         const int32_t* wtable, int64_t wtable_stride,
                                         const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                         const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                         int32_t* error_flag, deepep_stream_t stream) {
    if (num_units < 0 || hidden < 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "negative size (num_units=%d, hidden=%d)", num_units, hidden);
    if (num_units == 0) return DEEPEP_OK;
    if (hidden < 128 || hidden % 128 != 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "LogFMT wire rows need hidden (%d) to be a positive multiple of 128", hidden);
    if (out_rows == nullptr || (src == nullptr && num_src_rows > 0) || !aligned16(src))
        return set_error(DEEPEP_ERR_INVALID_ARG, "null out_rows / unaligned src");
    if (src_row_stride % 8 != 0 || src_row_stride < hidden)
        return set_error(DEEPEP_ERR_INVALID_ARG, "src row stride must be >= hidden and a multiple of 8 elements");
    if (table != nullptr && (table_width < 1 || table_width > kMaxWidth || table_stride < table_width))
        return set_error(DEEPEP_ERR_INVALID_ARG, "table width %d outside [1, %d] or stride too small", table_width, kMaxWidth);
    if (weighted && row_weights == nullptr)
        return set_error(DEEPEP_ERR_INVALID_ARG, "weighted reduction needs row weights");
    // the bytes one unit stores: the coded bytes [low | high | meta], then (with weights) weights_pad floats at
    // weights_offset
    const int64_t coded = static_cast<int64_t>(hidden) * 5 / 4 + hidden / 32;
    if (num_weights > 0 && (wsrc == nullptr || num_weights > kMaxWidth))
        return set_error(DEEPEP_ERR_INVALID_ARG, "weights need wsrc and num_weights <= %d", kMaxWidth);
    if (num_weights > 0 && (weights_offset < coded || weights_offset % 16 != 0))
        return set_error(DEEPEP_ERR_INVALID_ARG, "weights_offset (%lld) must be 16-byte aligned and past the coded bytes (%lld)",
                         static_cast<long long>(weights_offset), static_cast<long long>(coded));
    if (weights_pad < num_weights) weights_pad = num_weights;
    if (weights_pad > 64) return set_error(DEEPEP_ERR_INVALID_ARG, "weights_pad > 64");
    const int64_t row_extent = num_weights > 0 ? std::max<int64_t>(coded, weights_offset + 4 * weights_pad) : coded;
    if (window_bases == nullptr || num_windows < 1 || num_windows > 64 || window_bytes < row_extent)
        return set_error(DEEPEP_ERR_INVALID_ARG, "scatter needs 1..64 windows of at least one wire row (%lld bytes)",
                         static_cast<long long>(row_extent));
    Params p = {};
    p.src = static_cast<const uint16_t*>(src);
    p.num_src_rows = num_src_rows;
    p.src_stride = src_row_stride;
    p.table = table;
    p.table_stride = table_stride;
    p.table_width = table_width;
    p.row_weights = row_weights;
    p.num_units = num_units;
    p.hidden = hidden;
    p.wtable = wtable;
    p.wtable_stride = wtable_stride;
    p.wsrc = wsrc;
    p.num_weights = num_weights > 0 ? num_weights : 0;
    p.weights_pad = weights_pad;
    p.error_flag = error_flag;
    p.out_rows = out_rows;
    p.weights_offset = weights_offset;
    p.win_bases = window_bases;
    p.win_count = num_windows;
    p.win_limit = static_cast<uint64_t>(window_bytes - row_extent);
    // the scatter's launch shape (launch_combine, phase A): 2 vectors per lane from 128 vectors on, 4 waves, 4 rows in
    // flight capped by the table's width; the diagnostics knob overrides within the shapes built (8 rows run as 4)
    const uint32_t cfg = g_launch_config.load(std::memory_order_relaxed);
    const int cfg_vpt = static_cast<int>(cfg & 15u), cfg_rows = static_cast<int>((cfg >> 4) & 15u);
    const int width = table == nullptr ? 1 : table_width;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Shape sh;
    sh.vpt = hidden / 8 >= 128 ? 2 : 1;
    sh.waves = 4;
    sh.group = width <= 2 ? 2 : 4;
    if (cfg_vpt != 0) sh.vpt = cfg_vpt;
    if (cfg_rows != 0) sh.group = std::min(cfg_rows, 4);
    if (weighted) launch_shape_scatter_logfmt<true>(p, sh, s);
    else launch_shape_scatter_logfmt<false>(p, sh, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return set_error(DEEPEP_ERR_HIP, "combine launch failed: %s", hipGetErrorString(err));
    return DEEPEP_OK;
}

int64_t deepep_combine_buffer_size(int num_max_tokens_per_rank, int hidden, int num_topk,
                                   int num_ranks, int allow_multiple_reduction) {
    // TokenLayout(hidden * 2, 0, num_topk, false) with 32-byte alignment (layout.cuh:179-209),
    // receive slots = min(R, K) with multiple reduction else K (buffer.hpp:616-633); the
    // xGMI fabric is load/store reachable, so no separate send buffer (is_scaleup_nvlink).
    if (num_max_tokens_per_rank <= 0 || hidden <= 0 || num_ranks <= 0)
        return set_error(DEEPEP_ERR_INVALID_ARG, "invalid buffer size arguments");
    if (num_topk == 0) num_topk = 32;
    auto align = [](int64_t x, int64_t a) { return (x + a - 1) / a * a; };
    const int64_t token_bytes = align(int64_t(hidden) * 2, 32) + align(int64_t(num_topk) * 8, 32);
    const int64_t slots = allow_multiple_reduction ? std::min(num_ranks, num_topk) : num_topk;
    return slots * num_max_tokens_per_rank * token_bytes;
}

}  // extern "C"
