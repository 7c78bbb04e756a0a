// fp8_cast.hip -- the per-token FP8 cast on MI355X: alone (deepep_cast_fp8) and fused into the dispatch's
// pack (deepep_dispatch_pack_cast).
//
// Reference (paths in /root/reference):
//   per_token_cast_to_fp8   deep_ep/utils/math.py:30-39 (what every FP8-dispatch caller runs first)
//   the fused form          csrc/kernels/legacy/internode_ll.cu:220-245 (use_fp8 / round_scale inside the send
//                           kernel), calculate_fp8_scales csrc/kernels/legacy/utils.cuh:494-503
//
// The packing half (destination rows, bounds, fault record, the row's tail) restates pack_kernel of
// dispatch.hip, which stays as it is; the row layout is the same [x | sf | topk_idx | weights | src].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdio.h>

#include "../../include/deepep_amd.h"
#include "fault.h"

extern "C" __attribute__((visibility("hidden"))) int deepep_amd_set_error(int code, const char* msg);

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool kPeer, typename V>
__device__ __forceinline__ void put(V* p, V v) {
    if constexpr (kPeer) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else *p = v;
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

// ---------------------------------------------------------------- the cast (per token, per 128 columns)
// The per-token cast in front of an FP8 dispatch (reference: per_token_cast_to_fp8, deep_ep/utils/math.py:30-39;
// fused into the send kernel by the legacy low-latency path, csrc/kernels/legacy/internode_ll.cu:220-245 with
// calculate_fp8_scales, csrc/kernels/legacy/utils.cuh:494-503).  A lane holds 8 consecutive bf16 (one 16-byte
// load), so 16 lanes hold one 128-column group and a wave four groups; the group's amax is a 16-lane
// butterfly, the 8 OCP e4m3fn bytes leave in one 8-byte store.  Bitwise contract, per group:
//   round_scale == 0: amax = max(max|x|, 1e-4f); sf = amax / 448.0f; q = e4m3fn_rne(fp32(x) * ((1.0f / amax) * 448.0f))
//                     (torch evaluates the reference's `448.0 / amax` as reciprocal(amax) * 448: two roundings)
//   round_scale != 0: v = amax * fp32(1 / 448); e = exponent(v) + (mantissa(v) != 0); sf = 2^e;
//                     q = e4m3fn_rne(fp32(x) * 2^-e)
// -- true fp32 divisions, one fp32 multiply and one round-to-nearest-even conversion per element.  Inputs are
// finite bf16 (NaN / Inf: unspecified).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct Fp8Lane {
    u32x2 q;        // this lane's 8 e4m3fn bytes
    float sf;       // the group's scale factor (the same in its 16 lanes)
};

// raw: 8 bf16 of one lane (zeros in a lane past the row: it must still run the butterfly)
__device__ __forceinline__ Fp8Lane cast_group_fp8(const u32x4& raw, int round_scale) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(raw[j] << 16);
        f[2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u);
    }
    float amax = 1e-4f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    float scale, sf;
    if (round_scale) {
        const uint32_t bits = __float_as_uint(amax * (1.0f / 448.0f));
        const int e = static_cast<int>((bits >> 23) & 0xffu) - 127 + ((bits & 0x7fffffu) != 0);
        sf = __uint_as_float(static_cast<uint32_t>(e + 127) << 23);
        scale = __uint_as_float(static_cast<uint32_t>(127 - e) << 23);
    } else {
        sf = amax / 448.0f;
        scale = (1.0f / amax) * 448.0f;                  // not 448.0f / amax: see above
    }
    Fp8Lane out;
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * scale, f[1] * scale, 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * scale, f[3] * scale, lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * scale, f[5] * scale, 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * scale, f[7] * scale, hi, true);
    out.q = u32x2{static_cast<uint32_t>(lo), static_cast<uint32_t>(hi)};
    out.sf = sf;
    return out;
}

// One wave per row: q [num_rows][hidden] and sf [num_rows][hidden / 128], both contiguous; every input
// row is read once.
__global__ void __launch_bounds__(64)
cast_fp8_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden, int round_scale,
                uint8_t* __restrict__ q, float* __restrict__ sf) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const u32x4* xs = reinterpret_cast<const u32x4*>(x + t * x_stride);
    u32x2* qs = reinterpret_cast<u32x2*>(q + t * hidden);
    float* sfs = sf + t * (hidden / 128);
    const int nvec = hidden / 8;
    // a lane past the row loads nothing and holds zeros (whole 16-lane groups: hidden % 128 == 0)
    auto load = [&](int v) { return v < nvec ? __builtin_nontemporal_load(xs + v) : u32x4{0u, 0u, 0u, 0u}; };
    u32x4 next = load(lane);
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        const bool in = v < nvec;
        const u32x4 raw = next;
        next = load(v + 64);                             // in flight while this vector is reduced and cast
        const Fp8Lane c = cast_group_fp8(raw, round_scale);
        if (in) {
            qs[v] = c.q;                                 // plain stores: the dispatch reads them right back
            if ((lane & 15) == 0) sfs[v >> 4] = c.sf;
        }
    }
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

// pack_kernel (dispatch.hip) for a bf16 row cast on the way: the token's bf16 row is read once and quantised in
// registers, the e4m3fn bytes and the scale factors go into the packed row of every destination
// (layout [hidden fp8 | hidden / 128 fp32 @sf_off | ...], as pack_kernel's with an fp8 payload).
template <bool kPeer>
__global__ void __launch_bounds__(64)
pack_cast_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden, int round_scale,
                 const int64_t* __restrict__ topk_idx, const float* __restrict__ topk_weights, int K,
                 int32_t src_base, const int32_t* __restrict__ dst_slot, const int32_t* __restrict__ send_offsets, int R,
                 uint8_t* __restrict__ packed, const uint64_t* __restrict__ dest_bases, int64_t row_bytes,
                 int64_t dest_rows, int sf_off, int idx_off, int w_off, int src_off, int32_t* __restrict__ error_flag) {
    const int t = blockIdx.x, lane = threadIdx.x;
    // a timed-out window barrier before this push: nothing is stored into the peers (as pack_kernel)
    if (kPeer && error_flag != nullptr &&
        (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;
    const uint64_t my_row = pack_dest_row<kPeer>(t, lane, dst_slot, send_offsets, R, packed, dest_bases, row_bytes,
                                                 dest_rows, error_flag);
    const uint64_t dmask = __ballot(my_row != 0);
    const u32x4* xs = reinterpret_cast<const u32x4*>(x + t * x_stride);
    const int nvec = hidden / 8;
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        const bool in = v < nvec;
        const u32x4 raw = in ? __builtin_nontemporal_load(xs + v) : u32x4{0u, 0u, 0u, 0u};
        const Fp8Lane c = cast_group_fp8(raw, round_scale);
        for (uint64_t m = dmask; m; m &= m - 1) {
            uint8_t* row = pack_row_of(my_row, __builtin_ctzll(m));
            if (in) {
                put8<kPeer>(row, v * 8, c.q, static_cast<int>(row_bytes));
                if ((lane & 15) == 0) put<kPeer>(reinterpret_cast<float*>(row + sf_off) + (v >> 4), c.sf);
            }
        }
    }
    pack_tail<kPeer>(t, lane, my_row, dmask, topk_idx, topk_weights, K, src_base, idx_off, w_off, src_off);
}


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

}  // namespace

extern "C" {

int deepep_cast_fp8(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, int round_scale,
                    void* q, float* sf, deepep_stream_t stream) {
    if (num_rows == 0) return DEEPEP_OK;
    if (num_rows < 0 || hidden < 128 || hidden % 128 != 0)
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG, "cast_fp8: hidden must be a positive multiple of 128");
    if (x == nullptr || q == nullptr || sf == nullptr || !a16(x) || !a16(q) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0)
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG, "cast_fp8: null or misaligned pointers (16-byte aligned rows)");
    if (x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG,
                                    "cast_fp8: row stride below hidden * 2 bytes or not 16-byte aligned");
    hipLaunchKernelGGL(cast_fp8_kernel, dim3(num_rows), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                       static_cast<uint8_t*>(q), sf);
    return launch_status("cast_fp8");
}

int deepep_dispatch_pack_cast(const void* x, int64_t x_row_stride_bytes, int hidden, int round_scale,
                              const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                              int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks,
                              void* packed, const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows,
                              int sf_off, int idx_off, int w_off, int src_off, int32_t* error_flag,
                              deepep_stream_t stream) {
    if (num_tokens == 0) return DEEPEP_OK;
    if (hidden < 128 || hidden % 128 != 0)
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG,
                                    "dispatch_pack_cast: hidden must be a positive multiple of 128");
    if (x == nullptr || !a16(x) || x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG,
                                    "dispatch_pack_cast: x null, misaligned, or its row stride below hidden * 2 bytes "
                                    "or not 16-byte aligned");
    // the row holds [hidden fp8 | hidden / 128 fp32 @sf_off | topk_idx @idx_off | weights @w_off | src @src_off]
    if (num_tokens < 0 || num_topk < 1 || num_topk > 32 || num_ranks < 1 || num_ranks > 64 || dest_rows < 0 ||
        topk_idx == nullptr || dst_slot == nullptr || send_offsets == nullptr ||
        sf_off < hidden || sf_off % 4 || idx_off < sf_off + hidden / 128 * 4 || idx_off % 8 ||
        w_off < idx_off + num_topk * 8 || w_off % 4 || src_off < w_off + num_topk * 4 || src_off % 4 ||
        row_bytes < src_off + 4 || row_bytes % 16 || (dest_bases == nullptr && (packed == nullptr || !a16(packed))))
        return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG, "dispatch_pack_cast: invalid arguments or row layout");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dest_bases != nullptr)
        hipLaunchKernelGGL(pack_cast_kernel<true>, dim3(num_tokens), dim3(64), 0, s,
                           static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                           topk_idx, topk_weights, num_topk, src_base, dst_slot, send_offsets, num_ranks,
                           static_cast<uint8_t*>(packed), dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off, src_off,
                           error_flag);
    else
        hipLaunchKernelGGL(pack_cast_kernel<false>, dim3(num_tokens), dim3(64), 0, s,
                           static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                           topk_idx, topk_weights, num_topk, src_base, dst_slot, send_offsets, num_ranks,
                           static_cast<uint8_t*>(packed), dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off, src_off,
                           error_flag);
    return launch_status("dispatch_pack_cast");
}

}  // extern "C"
