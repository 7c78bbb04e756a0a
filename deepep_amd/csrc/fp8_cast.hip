// fp8_cast.hip -- the per-token FP8 cast on MI355X: alone (deepep_cast_fp8), fused into the dispatch's
// pack (deepep_dispatch_pack_cast) and, at one rank, into its receive-side copy (deepep_dispatch_copy_cast);
// and its inverse (deepep_cast_back_fp8).  Every kernel and launcher is written once, over a scale-factor format
// (enum Sf); all that a format decides stands in its SfFormat<> specialisation (fp8_cast_common.h):
//   Sf::kFp32    the plain entries     float32 per 128 columns
//   Sf::kExp128  the *_ue8m0 entries   a UE8M0 exponent byte per 128 columns, four to an int32
//   Sf::kExp32   the *_mx entries      MXFP8: a UE8M0 exponent byte per 32 columns, the group CDNA4's block-scaled
//                                      MFMA takes
//
// Reference (paths in /root/reference):
//   per_token_cast_to_fp8   deep_ep/utils/math.py:30-39 (what every FP8-dispatch caller runs first)
//   per_token_cast_back     deep_ep/utils/math.py:42-56 (what the expert side runs on the received pair)
//   the fused form          csrc/kernels/legacy/internode_ll.cu:220-245 (use_fp8 / round_scale inside the send
//                           kernel), calculate_fp8_scales csrc/kernels/legacy/utils.cuh:494-503
//
// The packing half (destination rows, bounds, fault record, the row's tail), the cross-lane steps and the UE8M0
// bytes stand in cast_common.h, which fp4_cast.hip (the same five kernels over e2m1 rows) shares; the scale rule, the
// e4m3fn conversion, a lane's cast of a group (cast_group_fp8) and the SfFormat<> specialisations stand in
// fp8_cast_common.h, which fp8_cast_t.hip (the transposed MXFP8 cast) shares.
#include "fp8_cast_common.h"

namespace {

// One wave per row: q [num_rows][hidden] and sf [num_rows][hidden / kElemCols], both contiguous; every input row is
// read once.  A lane holds 8 columns, a pass of the wave 512 (hidden % 128 == 0: a 16-lane row of the wave is inside
// the row of x or outside).
template <Sf kSf>
__global__ void __launch_bounds__(64)
cast_fp8_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden, int round_scale,
                uint8_t* __restrict__ q, sf_elem_t<kSf>* __restrict__ sf) {
    using F = SfFormat<kSf>;
    using Tile = SfTile<kSf, 8>;
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const u32x4* xs = reinterpret_cast<const u32x4*>(x + t * x_stride);
    u32x2* qs = reinterpret_cast<u32x2*>(q + t * hidden);
    sf_elem_t<kSf>* sfs = sf + t * (hidden / F::kElemCols);
    const int nvec = hidden / 8;
    // a lane past the row loads nothing and holds zeros (whole 16-lane groups: hidden % 128 == 0)
    auto load = [&](int v) { return v < nvec ? __builtin_nontemporal_load(xs + v) : u32x4{0u, 0u, 0u, 0u}; };
    u32x4 next = load(lane);
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        const bool in = v < nvec;
        const u32x4 raw = next;
        next = load(v + 64);                             // in flight while this vector is reduced and cast
        const Fp8Lane<1> c = cast_group_fp8<1, F::kGroupCols>(&raw, round_scale);
        const auto w = Tile::word(c.sf, lane);
        if (in) {
            qs[v] = c.q;                                 // plain stores: the dispatch reads them right back
            if (Tile::owns(lane)) sfs[Tile::index(v, lane)] = w;
        }
    }
}

// ---------------------------------------------------------------- the cast back (per token, per group of columns)
// The inverse (reference: per_token_cast_back, deep_ep/utils/math.py:42-56) for the pair an FP8 dispatch returns:
// out bf16 [num_rows][hidden] = bf16_rne(fp32(q) * sf) -- e4m3fn -> fp32 is exact, one fp32 multiply by the group's
// scale factor, one round-to-nearest-even to bf16 (v_cvt_pk_bf16_f32).  A lane holds 16 consecutive e4m3fn bytes
// (one 16-byte load) and stores their 32 bytes of bf16 as two 16-byte stores; 8 lanes hold 128 columns, whose
// scale factor(s) the format loads and hands round (SfFormat<>::back_*).  One wave per row, 1024 columns a pass, the
// next pass's loads in flight.  The scale factors are addressed by strides (counted in the format's stride_unit), so
// the column-major tensor of use_tma_aligned_col_major_sf is read in place.
// (the arithmetic is deepep::dequant16 / deepep::ue8m0_factor of fp8_dequant.h, which the combine's FP8 source shares)
constexpr int kCastBackWaves = 4;                              // rows per workgroup, one wave each

template <Sf kSf>
__global__ void __launch_bounds__(64 * kCastBackWaves)
cast_back_fp8_kernel(const uint8_t* __restrict__ q, int64_t q_stride, const sf_elem_t<kSf>* __restrict__ sf,
                     int64_t sf_row_stride, int64_t sf_col_stride, int num_rows, int hidden,
                     uint8_t* __restrict__ out) {
    using F = SfFormat<kSf>;
    const int lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kCastBackWaves +
                      __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= num_rows) return;
    const u32x4* qs = reinterpret_cast<const u32x4*>(q + t * q_stride);
    const auto* sfs = reinterpret_cast<const sf_elem_t<kSf>*>(
        reinterpret_cast<const typename F::stride_unit*>(sf) + t * sf_row_stride);
    u32x4* os = reinterpret_cast<u32x4*>(out + t * hidden * 2);
    const int nvec = hidden / 16;
    // a lane past the row loads nothing (whole 8-lane groups: hidden % 128 == 0)
    auto load = [&](int u) { return u < nvec ? __builtin_nontemporal_load(qs + u) : u32x4{0u, 0u, 0u, 0u}; };
    const bool sf_dwords = F::back_dwords(sf_row_stride, sf_col_stride);                 // wave-uniform
    auto load_sf = [&](int u) { return F::back_load(sfs, u, u < nvec, lane, sf_col_stride, sf_dwords); };
    u32x4 next = load(lane);
    auto next_sf = load_sf(lane);
    for (int u0 = 0; u0 < nvec; u0 += 64) {
        const int u = u0 + lane;
        const u32x4 raw = next;
        const float s = F::back_factor(next_sf, lane, sf_dwords);
        next = load(u + 64);                                 // in flight while this vector is converted
        next_sf = load_sf(u + 64);
        if (u < nvec) {
            u32x4 lo, hi;
            deepep::dequant16(raw, s, lo, hi);
            os[2 * u] = lo;
            os[2 * u + 1] = hi;
        }
    }
}

// pack_kernel (dispatch.hip) for a bf16 row cast on the way: the token's bf16 row is read once and quantised in
// registers (the cast kernel's tiling), the e4m3fn bytes and the scale factors go into the packed row of every
// destination: layout [hidden fp8 | hidden / kElemCols elements @sf_off | ...], as pack_kernel's with an fp8 payload
// (sf_off % 4 == 0).  The scale factors are stored with put<kPeer>, as every other field.
template <bool kPeer, Sf kSf>
__global__ void __launch_bounds__(64)
pack_cast_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden, int round_scale,
                 const int64_t* __restrict__ topk_idx, const float* __restrict__ topk_weights, int K,
                 int32_t src_base, const int32_t* __restrict__ dst_slot, const int32_t* __restrict__ send_offsets, int R,
                 uint8_t* __restrict__ packed, const uint64_t* __restrict__ dest_bases, int64_t row_bytes,
                 int64_t dest_rows, int sf_off, int idx_off, int w_off, int src_off, int32_t* __restrict__ error_flag) {
    using F = SfFormat<kSf>;
    using Tile = SfTile<kSf, 8>;
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
        const Fp8Lane<1> c = cast_group_fp8<1, F::kGroupCols>(&raw, round_scale);
        const auto w = Tile::word(c.sf, lane);
        for (uint64_t m = dmask; m; m &= m - 1) {
            uint8_t* row = pack_row_of(my_row, __builtin_ctzll(m));
            if (in) {
                put8<kPeer>(row, v * 8, c.q, static_cast<int>(row_bytes));
                if (Tile::owns(lane))
                    put<kPeer>(reinterpret_cast<sf_elem_t<kSf>*>(row + sf_off) + Tile::index(v, lane), w);
            }
        }
    }
    pack_tail<kPeer>(t, lane, my_row, dmask, topk_idx, topk_weights, K, src_base, idx_off, w_off, src_off);
}

// ---------------------------------------------------------------- the one-rank copy with the cast on the way
// The direct forms of dispatch.hip's copy kernels (one rank: received row i's x is the sender's row
// meta[i][0] % num_max_tokens) for a bf16 source quantised in registers.  The row stores are write-through, and a
// write-through store narrower than 16 bytes costs a fabric write of its own, so here a lane holds 16 consecutive
// bf16 (two 16-byte loads) and its 16 e4m3fn bytes leave in one 16-byte store: 8 lanes hold 128 columns.  The source
// rows are read through a buffer descriptor of the row's 2 * hidden bytes: a lane past the row end loads zeros and
// still runs the butterfly.  A column chunk is 128 such stores per row = 2 KiB of fp8 = 16 whole groups of 128,
// read as 4 KiB of bf16: four 16-byte loads per lane and row.
constexpr int kCastChunkVecs = 128;                      // 16-byte output vectors: 64 lanes x 2
constexpr int kBlockRows = DEEPEP_DISPATCH_BLOCK_ROWS;

// the 32 bytes of bf16 behind output vector u of a row (the descriptor's range check: zeros past the row end)
__device__ __forceinline__ void load16(const uint8_t* row, int hidden, int u, u32x4* ab) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(row), 0, hidden * 2,
                                                                        0x00020000);
    ab[0] = __builtin_amdgcn_raw_buffer_load_b128(rs, u * 32, 0, 0);
    ab[1] = __builtin_amdgcn_raw_buffer_load_b128(rs, u * 32 + 16, 0, 0);
}

// Output vector u of one destination row: the cast, the 16-byte row store (the descriptor's range check drops the
// lanes past the row end) and, from the lanes that own an element, the scale factors (plain stores; sf_row: the
// destination row's hidden / kElemCols elements).
template <int kAux, Sf kSf>
__device__ __forceinline__ void cast_store16(const u32x4* ab, int round_scale, int u, bool in, int lane,
                                             const __amdgpu_buffer_rsrc_t& rs,
                                             sf_elem_t<kSf>* __restrict__ sf_row) {
    using Tile = SfTile<kSf, 16>;
    const Fp8Lane<2> c = cast_group_fp8<2, SfFormat<kSf>::kGroupCols>(ab, round_scale);
    __builtin_amdgcn_raw_buffer_store_b128(c.q, rs, u * 16, 0, kAux);
    const auto w = Tile::word(c.sf, lane);
    if (in && Tile::owns(lane)) sf_row[Tile::index(u, lane)] = w;
}

// copy_kernel's direct case: work item = (received row, column chunk), one wave per item; the row goes to
// recv_x[i] (non-expanded) or to every local slot of the row (expanded; lane k holds slot k's row), weights as
// copy_kernel's (chunk 0).  Row stores are write-through (sc1), as copy_kernel's.  recv_sf: [num_out_rows]
// [hidden / kElemCols] elements.
template <Sf kSf>
__global__ void __launch_bounds__(256)
copy_cast_kernel(const uint8_t* __restrict__ packed, int64_t row_bytes, int w_off, int N, int K,
                 const int32_t* __restrict__ meta, int expanded, const uint8_t* __restrict__ x, int64_t x_stride,
                 int hidden, int round_scale, int num_max_tokens, uint8_t* __restrict__ recv_x,
                 sf_elem_t<kSf>* __restrict__ recv_sf, float* __restrict__ recv_w, int64_t num_out_rows,
                 const int32_t* __restrict__ row_map, int32_t* __restrict__ error_flag) {
    using F = SfFormat<kSf>;
    using Tile = SfTile<kSf, 16>;
    const int lane = threadIdx.x & 63;
    if (error_flag != nullptr && (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;                                            // a timed-out window barrier: store nothing
    const int nvec = hidden / 16;
    const int nch = (nvec + kCastChunkVecs - 1) / kCastChunkVecs;
    const int64_t it = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (it >= static_cast<int64_t>(N) * nch) return;
    const int64_t i = it / nch;
    const int c = static_cast<int>(it - i * nch);
    const int32_t src = __builtin_amdgcn_readfirstlane(meta[i * (K + 2)]);
    if (src < 0) return;                                  // past the received rows (count_kernel)
    const uint8_t* xs = x + static_cast<int64_t>(src % num_max_tokens) * x_stride;
    int32_t my_dst = -1;
    if (expanded) {
        if (lane < K) my_dst = meta[i * (K + 2) + 2 + lane];
    } else if (lane == 0) {
        my_dst = static_cast<int32_t>(i);
    }
    if (my_dst >= num_out_rows) {                          // never store past the outputs
        if (error_flag != nullptr) atomicOr(error_flag, 1);
        my_dst = -1;
    }
    const uint64_t dmask = __ballot(my_dst >= 0);
    const int sf_n = hidden / F::kElemCols;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (c * kCastChunkVecs + p * 64 >= nvec) break;    // wave-uniform: no group of this half is in the row
        const int u = c * kCastChunkVecs + p * 64 + lane;
        const bool in = u < nvec;
        u32x4 ab[2];
        load16(xs, hidden, u, ab);
        const Fp8Lane<2> q = cast_group_fp8<2, F::kGroupCols>(ab, round_scale);
        const auto w = Tile::word(q.sf, lane);
        for (uint64_t m = dmask; m; m &= m - 1) {
            const int64_t d = __builtin_amdgcn_readlane(my_dst, __builtin_ctzll(m));
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(recv_x + d * hidden, 0, hidden,
                                                                                0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(q.q, rs, u * 16, 0, 16);
            if (in && Tile::owns(lane)) recv_sf[d * sf_n + Tile::index(u, lane)] = w;
        }
    }
    if (c != 0) return;
    if (recv_w != nullptr && lane < K) {
        const uint8_t* row = packed + (row_map != nullptr ? static_cast<int64_t>(row_map[i]) : i) * row_bytes;
        const float w = reinterpret_cast<const float*>(row + w_off)[lane];
        if (expanded) {
            if (my_dst >= 0) recv_w[my_dst] = w;
        } else {
            recv_w[i * K + lane] = w;
        }
    }
}

// copy_expanded_kernel<true> (dispatch.hip) with the cast on the way: the same blocked
// destination-major tiling -- one wave per (block of kBlockRows received rows, local expert, column chunk) writes
// the run of consecutive expanded rows [block_offsets[b][e], block_offsets[b + 1][e]) and finds their sources
// through inv; workgroups w = x (mod 8) run on XCD x and take blocks x, x + 8, ..., so a block's bf16 source rows
// are read once from HBM and re-read (and re-quantised) once per local expert from that XCD's L2.  Row stores are
// streaming write-through (sc1 nt), scale factors and weights plain.  recv_sf: [num_out_rows][hidden / kElemCols]
// elements (cast_store16).
template <Sf kSf>
__global__ void __launch_bounds__(256)
copy_cast_expanded_kernel(const uint8_t* __restrict__ packed, int64_t row_bytes, int w_off, int N, int K,
                          const int32_t* __restrict__ meta, const uint8_t* __restrict__ x, int64_t x_stride,
                          int hidden, int round_scale, int num_max_tokens, const int32_t* __restrict__ inv,
                          const int32_t* __restrict__ block_offsets, const int32_t* __restrict__ expert_end, int nb,
                          int epr, uint8_t* __restrict__ recv_x, sf_elem_t<kSf>* __restrict__ recv_sf,
                          float* __restrict__ recv_w, int64_t num_out_rows, const int32_t* __restrict__ row_map,
                          int32_t* __restrict__ error_flag) {
    constexpr int kRows = 4;                               // destination rows in flight per wave
    constexpr int kAux = 18;                               // sc1 | nt
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (error_flag != nullptr && (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;                                            // a timed-out window barrier: store nothing
    const int nvec = hidden / 16;
    const int nch = (nvec + kCastChunkVecs - 1) / kCastChunkVecs;
    const int64_t wg_per_block = (static_cast<int64_t>(epr) * nch + 3) / 4;
    const int64_t xcd = blockIdx.x % 8, kk = blockIdx.x / 8;
    const int64_t b = xcd + 8 * (kk / wg_per_block);
    const int64_t it = (kk % wg_per_block) * 4 + wave;
    const int e = static_cast<int>(it / nch), c = static_cast<int>(it - static_cast<int64_t>(e) * nch);
    if (b >= nb || e >= epr) return;
    const int r0 = block_offsets[b * epr + e];
    const int r1 = b + 1 < nb ? block_offsets[(b + 1) * epr + e] : expert_end[e];
    const int u0 = c * kCastChunkVecs + lane, u1 = u0 + 64;
    const bool in0 = u0 < nvec, in1 = u1 < nvec;
    const bool half1 = c * kCastChunkVecs + 64 < nvec;     // wave-uniform: the chunk's second half holds a group
    const int sf_n = hidden / SfFormat<kSf>::kElemCols;
    for (int j = r0; j < r1; j += kRows) {
        int32_t src_i[kRows], src_k[kRows];
        u32x4 a[kRows][4];
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
            src_i[q] = -1;
            src_k[q] = 0;
            if (j + q < r1) {
                const int32_t code = __builtin_amdgcn_readfirstlane(inv[j + q]);
                const int32_t i = code >= 0 ? code / K : -1;
                const int32_t src =
                    i >= 0 && i < N ? __builtin_amdgcn_readfirstlane(meta[static_cast<int64_t>(i) * (K + 2)]) : -1;
                if (src >= 0) {
                    src_i[q] = i;
                    src_k[q] = code - i * K;
                    const uint8_t* xs = x + static_cast<int64_t>(src % num_max_tokens) * x_stride;
                    load16(xs, hidden, u0, a[q]);
                    if (half1) load16(xs, hidden, u1, a[q] + 2);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
            if (src_i[q] < 0) continue;
            const int64_t d = j + q;
            if (d >= num_out_rows) {                       // never store past the outputs
                if (lane == 0 && error_flag != nullptr) atomicOr(error_flag, 1);
                continue;
            }
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(recv_x + d * hidden, 0, hidden,
                                                                                0x00020000);
            sf_elem_t<kSf>* sf_row = recv_sf + d * sf_n;
            cast_store16<kAux, kSf>(a[q], round_scale, u0, in0, lane, rs, sf_row);
            if (half1) cast_store16<kAux, kSf>(a[q] + 2, round_scale, u1, in1, lane, rs, sf_row);
            if (c != 0) continue;
            if (recv_w != nullptr && lane == 0) {
                const int64_t prow = row_map != nullptr ? static_cast<int64_t>(row_map[src_i[q]]) : src_i[q];
                recv_w[d] = reinterpret_cast<const float*>(packed + prow * row_bytes + w_off)[src_k[q]];
            }
        }
    }
}

// hidden (and, where the entry takes one, a non-negative row count)
template <Sf kSf>
int bad_hidden(const char* what, int hidden, int num_rows = 0) {
    constexpr int kMultiple = SfFormat<kSf>::kElemCols;      // rows of whole elements
    if (num_rows >= 0 && hidden >= kMultiple && hidden % kMultiple == 0) return DEEPEP_OK;
    char msg[64];
    snprintf(msg, sizeof(msg), "hidden must be a positive multiple of %d", kMultiple);
    return invalid(what, msg);
}

template <Sf kSf>
int cast_fp8(const char* what, const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, int round_scale,
             void* q, void* sf, deepep_stream_t stream) {
    if (num_rows == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden<kSf>(what, hidden, num_rows)) return rc;
    if (x == nullptr || q == nullptr || sf == nullptr || !a16(x) || !a16(q) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden * 2 bytes or not 16-byte aligned");
    hipLaunchKernelGGL((cast_fp8_kernel<kSf>), dim3(num_rows), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                       static_cast<uint8_t*>(q), static_cast<sf_elem_t<kSf>*>(sf));
    return launch_status(what);
}

template <Sf kSf>
int cast_back_fp8(const char* what, const void* q, int64_t q_row_stride_bytes, const void* sf,
                  int64_t sf_row_stride, int64_t sf_col_stride, int num_rows, int hidden, void* out,
                  deepep_stream_t stream) {
    if (num_rows == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden<kSf>(what, hidden, num_rows)) return rc;
    if (q == nullptr || out == nullptr || sf == nullptr || !a16(q) || !a16(out) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (q_row_stride_bytes < static_cast<int64_t>(hidden) || q_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden bytes or not 16-byte aligned");
    if (sf_row_stride < 0 || sf_col_stride < 0) return invalid(what, "negative scale-factor stride");
    // contiguous columns may be read as dwords, so their rows start on 4 bytes (strides in whole dwords: always)
    if (sf_col_stride == 1 && sf_row_stride * sizeof(typename SfFormat<kSf>::stride_unit) % 4 != 0)
        return invalid(what, "scale-factor rows of unit column stride must start 4-byte aligned");
    const unsigned grid = static_cast<unsigned>((static_cast<int64_t>(num_rows) + kCastBackWaves - 1) / kCastBackWaves);
    hipLaunchKernelGGL((cast_back_fp8_kernel<kSf>), dim3(grid), dim3(64 * kCastBackWaves), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(q), q_row_stride_bytes,
                       static_cast<const sf_elem_t<kSf>*>(sf), sf_row_stride, sf_col_stride, num_rows,
                       hidden, static_cast<uint8_t*>(out));
    return launch_status(what);
}

template <Sf kSf>
int dispatch_pack_cast(const char* what, const void* x, int64_t x_row_stride_bytes, int hidden, int round_scale,
                       const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                       int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks,
                       void* packed, const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows,
                       int sf_off, int idx_off, int w_off, int src_off, int32_t* error_flag, deepep_stream_t stream) {
    using F = SfFormat<kSf>;
    if (num_tokens == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden<kSf>(what, hidden)) return rc;
    if (x == nullptr || !a16(x) || x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "x null, misaligned, or its row stride below hidden * 2 bytes or not 16-byte aligned");
    // the row holds [hidden fp8 | hidden / kElemCols elements @sf_off | topk_idx @idx_off | weights @w_off |
    // src @src_off]
    const int sf_bytes = hidden / F::kElemCols * static_cast<int>(sizeof(sf_elem_t<kSf>));
    if (num_tokens < 0 || num_topk < 1 || num_topk > 32 || num_ranks < 1 || num_ranks > 64 || dest_rows < 0 ||
        topk_idx == nullptr || dst_slot == nullptr || send_offsets == nullptr ||
        sf_off < hidden || sf_off % 4 || idx_off < sf_off + sf_bytes || idx_off % 8 ||
        w_off < idx_off + num_topk * 8 || w_off % 4 || src_off < w_off + num_topk * 4 || src_off % 4 ||
        row_bytes < src_off + 4 || row_bytes % 16 || (dest_bases == nullptr && (packed == nullptr || !a16(packed))))
        return invalid(what, "invalid arguments or row layout");
    const auto kernel = dest_bases != nullptr ? pack_cast_kernel<true, kSf> : pack_cast_kernel<false, kSf>;
    hipLaunchKernelGGL(kernel, dim3(num_tokens), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                       topk_idx, topk_weights, num_topk, src_base, dst_slot, send_offsets, num_ranks,
                       static_cast<uint8_t*>(packed), dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off, src_off,
                       error_flag);
    return launch_status(what);
}

template <Sf kSf>
int dispatch_copy_cast(const char* what, const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                       const int32_t* src_metadata, int expanded, const void* x, int64_t x_row_stride_bytes,
                       int hidden, int round_scale, int num_max_tokens, void* recv_x, void* recv_sf,
                       float* recv_topk_weights, int64_t num_out_rows, const int32_t* inv,
                       const int32_t* block_offsets, const int32_t* expert_end, int num_local_experts,
                       const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream) {
    if (num_recv == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden<kSf>(what, hidden)) return rc;
    if (x == nullptr || !a16(x) || x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "x null, misaligned, or its row stride below hidden * 2 bytes or not 16-byte aligned");
    if (num_recv < 0 || num_topk < 1 || num_topk > 32 || num_max_tokens < 1 || num_out_rows < 0 ||
        src_metadata == nullptr || recv_x == nullptr || !a16(recv_x) || recv_sf == nullptr ||
        (reinterpret_cast<uintptr_t>(recv_sf) & 3u) != 0 ||
        (recv_topk_weights != nullptr && (packed == nullptr || !a16(packed) || row_bytes % 16 || w_off < 0 ||
                                          w_off % 4 || row_bytes < w_off + num_topk * 4)) ||
        (inv != nullptr && (!expanded || block_offsets == nullptr || expert_end == nullptr || num_local_experts < 1 ||
                            num_local_experts > 1024)))
        return invalid(what, "invalid arguments or alignment");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nch = (hidden / 16 + kCastChunkVecs - 1) / kCastChunkVecs;
    if (inv != nullptr) {
        const int nb = (num_recv + kBlockRows - 1) / kBlockRows;
        const int64_t wg_per_block = (static_cast<int64_t>(num_local_experts) * nch + 3) / 4;
        const int64_t grid = 8 * wg_per_block * ((nb + 7) / 8);
        hipLaunchKernelGGL((copy_cast_expanded_kernel<kSf>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, s,
                           static_cast<const uint8_t*>(packed), row_bytes, w_off, num_recv, num_topk, src_metadata,
                           static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale, num_max_tokens,
                           inv, block_offsets, expert_end, nb, num_local_experts, static_cast<uint8_t*>(recv_x),
                           static_cast<sf_elem_t<kSf>*>(recv_sf), recv_topk_weights, num_out_rows, row_map, error_flag);
        return launch_status(what);
    }
    const int64_t items = static_cast<int64_t>(num_recv) * nch;
    hipLaunchKernelGGL((copy_cast_kernel<kSf>), dim3(static_cast<unsigned>((items + 3) / 4)), dim3(256), 0, s,
                       static_cast<const uint8_t*>(packed), row_bytes, w_off, num_recv, num_topk, src_metadata,
                       expanded, static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, round_scale,
                       num_max_tokens, static_cast<uint8_t*>(recv_x), static_cast<sf_elem_t<kSf>*>(recv_sf),
                       recv_topk_weights, num_out_rows, row_map, error_flag);
    return launch_status(what);
}

}  // namespace

extern "C" {

int deepep_cast_fp8(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, int round_scale,
                    void* q, float* sf, deepep_stream_t stream) {
    return cast_fp8<Sf::kFp32>("cast_fp8", x, x_row_stride_bytes, num_rows, hidden, round_scale, q, sf, stream);
}

int deepep_cast_fp8_ue8m0(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, int32_t* sf,
                          deepep_stream_t stream) {
    return cast_fp8<Sf::kExp128>("cast_fp8_ue8m0", x, x_row_stride_bytes, num_rows, hidden, 1, q, sf, stream);
}

int deepep_cast_back_fp8(const void* q, int64_t q_row_stride_bytes, const float* sf, int64_t sf_row_stride,
                         int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream) {
    return cast_back_fp8<Sf::kFp32>("cast_back_fp8", q, q_row_stride_bytes, sf, sf_row_stride, sf_col_stride, num_rows,
                                    hidden, out, stream);
}

int deepep_cast_back_fp8_ue8m0(const void* q, int64_t q_row_stride_bytes, const int32_t* sf, int64_t sf_row_stride,
                               int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream) {
    return cast_back_fp8<Sf::kExp128>("cast_back_fp8_ue8m0", q, q_row_stride_bytes, sf, sf_row_stride, sf_col_stride,
                                      num_rows, hidden, out, stream);
}

int deepep_dispatch_pack_cast(const void* x, int64_t x_row_stride_bytes, int hidden, int round_scale,
                              const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                              int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks,
                              void* packed, const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows,
                              int sf_off, int idx_off, int w_off, int src_off, int32_t* error_flag,
                              deepep_stream_t stream) {
    return dispatch_pack_cast<Sf::kFp32>("dispatch_pack_cast", x, x_row_stride_bytes, hidden, round_scale, topk_idx,
                                         topk_weights, num_tokens, num_topk, src_base, dst_slot, send_offsets,
                                         num_ranks, packed, dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off,
                                         src_off, error_flag, stream);
}

int deepep_dispatch_pack_cast_ue8m0(const void* x, int64_t x_row_stride_bytes, int hidden,
                                    const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                                    int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets,
                                    int num_ranks, void* packed, const uint64_t* dest_bases, int64_t row_bytes,
                                    int64_t dest_rows, int sf_off, int idx_off, int w_off, int src_off,
                                    int32_t* error_flag, deepep_stream_t stream) {
    return dispatch_pack_cast<Sf::kExp128>("dispatch_pack_cast_ue8m0", x, x_row_stride_bytes, hidden, 1, topk_idx,
                                           topk_weights, num_tokens, num_topk, src_base, dst_slot, send_offsets,
                                           num_ranks, packed, dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off,
                                           src_off, error_flag, stream);
}

int deepep_dispatch_copy_cast(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                              const int32_t* src_metadata, int expanded, const void* x, int64_t x_row_stride_bytes,
                              int hidden, int round_scale, int num_max_tokens, void* recv_x, float* recv_sf,
                              float* recv_topk_weights, int64_t num_out_rows, const int32_t* inv,
                              const int32_t* block_offsets, const int32_t* expert_end, int num_local_experts,
                              const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream) {
    return dispatch_copy_cast<Sf::kFp32>("dispatch_copy_cast", packed, row_bytes, w_off, num_recv, num_topk,
                                         src_metadata, expanded, x, x_row_stride_bytes, hidden, round_scale,
                                         num_max_tokens, recv_x, recv_sf, recv_topk_weights, num_out_rows, inv,
                                         block_offsets, expert_end, num_local_experts, row_map, error_flag, stream);
}

int deepep_dispatch_copy_cast_ue8m0(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                    const int32_t* src_metadata, int expanded, const void* x,
                                    int64_t x_row_stride_bytes, int hidden, int num_max_tokens, void* recv_x,
                                    int32_t* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                                    const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                                    int num_local_experts, const int32_t* row_map, int32_t* error_flag,
                                    deepep_stream_t stream) {
    return dispatch_copy_cast<Sf::kExp128>("dispatch_copy_cast_ue8m0", packed, row_bytes, w_off, num_recv, num_topk,
                                           src_metadata, expanded, x, x_row_stride_bytes, hidden, 1, num_max_tokens,
                                           recv_x, recv_sf, recv_topk_weights, num_out_rows, inv, block_offsets,
                                           expert_end, num_local_experts, row_map, error_flag, stream);
}

// MXFP8: the *_ue8m0 entries' arguments, the scale factors one exponent byte per 32 columns
int deepep_cast_fp8_mx(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, uint8_t* sf,
                       deepep_stream_t stream) {
    return cast_fp8<Sf::kExp32>("cast_fp8_mx", x, x_row_stride_bytes, num_rows, hidden, 1, q, sf, stream);
}

int deepep_cast_back_fp8_mx(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf, int64_t sf_row_stride,
                            int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream) {
    return cast_back_fp8<Sf::kExp32>("cast_back_fp8_mx", q, q_row_stride_bytes, sf, sf_row_stride, sf_col_stride,
                                     num_rows, hidden, out, stream);
}

int deepep_dispatch_pack_cast_mx(const void* x, int64_t x_row_stride_bytes, int hidden, const int64_t* topk_idx,
                                 const float* topk_weights, int num_tokens, int num_topk, int32_t src_base,
                                 const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks, void* packed,
                                 const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows, int sf_off,
                                 int idx_off, int w_off, int src_off, int32_t* error_flag, deepep_stream_t stream) {
    return dispatch_pack_cast<Sf::kExp32>("dispatch_pack_cast_mx", x, x_row_stride_bytes, hidden, 1, topk_idx,
                                          topk_weights, num_tokens, num_topk, src_base, dst_slot, send_offsets,
                                          num_ranks, packed, dest_bases, row_bytes, dest_rows, sf_off, idx_off, w_off,
                                          src_off, error_flag, stream);
}

int deepep_dispatch_copy_cast_mx(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                 const int32_t* src_metadata, int expanded, const void* x, int64_t x_row_stride_bytes,
                                 int hidden, int num_max_tokens, void* recv_x, uint8_t* recv_sf,
                                 float* recv_topk_weights, int64_t num_out_rows, const int32_t* inv,
                                 const int32_t* block_offsets, const int32_t* expert_end, int num_local_experts,
                                 const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream) {
    return dispatch_copy_cast<Sf::kExp32>("dispatch_copy_cast_mx", packed, row_bytes, w_off, num_recv, num_topk,
                                          src_metadata, expanded, x, x_row_stride_bytes, hidden, 1, num_max_tokens,
                                          recv_x, recv_sf, recv_topk_weights, num_out_rows, inv, block_offsets,
                                          expert_end, num_local_experts, row_map, error_flag, stream);
}

}  // extern "C"
