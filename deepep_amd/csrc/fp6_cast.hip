// fp6_cast.hip -- MXFP6 on MI355X: OCP e2m3 rows, 32 codes to 24 bytes, with one UE8M0 exponent byte per 32 columns,
// the FP6 operand of gfx950's block-scaled MFMA (v_mfma_scale_f32_{32x32x64,16x16x128}_f8f6f4), which runs it at the
// FP4 rate.  The five kernels of fp4_cast.hip over that element type: the cast alone (deepep_cast_fp6_mx), fused into
// the dispatch's pack (deepep_dispatch_pack_cast_fp6_mx) and, at one rank, into its receive-side copy
// (deepep_dispatch_copy_cast_fp6_mx); and its inverse (deepep_cast_back_fp6_mx).  No counterpart in the reference.
//
// The format (include/deepep_amd.h has the whole contract), hidden % 128 == 0:
//   rows           uint8 [rows][3 * hidden / 4]: group g of 32 columns is bytes [24g, 24g + 24), a little-endian
//                  192-bit string with column c in bits 6c + 5 : 6c; a code is s ee mmm, magnitude mmm / 8 for ee == 0,
//                  else (1 + mmm / 8) * 2^(ee - 1): 0 .. 7.5
//   scale factors  uint8 [rows][hidden / 32], MXFP8's tensor: whole dwords per row, stored as dwords
//   the cast       amax = max(max|x|, 1e-4f); v = amax * fp32(1 / 7.5); e = exponent(v) + (mantissa(v) != 0);
//                  byte = e + 127; code = sign(x) | e2m3_rne(|fp32(x)| * 2^-e)    (the round_scale rule, 7.5 for 448)
//   the cast back  bf16 = bf16_rne(fp32(code) * float_from_bits(byte << 23))
// Both conversions are the hardware's, a whole group at a time: v_cvt_scalef32_pk32_fp6_bf16 (32 bf16 in 16 registers
// divided by the group's 2^e, round to nearest even, the sign kept, the 32 codes dense in 6 registers in the order
// above) and v_cvt_scalef32_pk32_f32_fp6 (with the scale 1.0f, the factor applied by an fp32 multiply of its own).
// tests/test_fp6_gpu.py holds them to the contract over every finite bf16 pattern, every code and every position.
//
// In every kernel a lane holds one whole group: four 16-byte loads in, 24 bytes out, the amax in the lane, a quad
// forms the dword of exponent bytes.  24 is no multiple of 16, and a write-through or system-scope store narrower than
// 16 bytes costs a fabric write of its own: a lane pair holds 48 contiguous bytes = three aligned 16-byte vectors (a
// row starts 16-byte aligned: 3 * hidden / 4 % 96 == 0), so the even lane takes the odd lane's first two dwords (two
// DPP moves) and the pair issues three 16-byte stores.  hidden % 128 == 0 keeps quads, and so pairs, whole.
//
// The scale rule, the e2m3 conversion and a lane's cast of a group are fp6_cast_common.h's, shared with the transposed
// cast (fp46_cast_t.hip); the packing half, the cross-lane steps and the UE8M0 bytes are cast_common.h's, shared with
// fp8_cast.hip and fp4_cast.hip, whose tiling comments give the reasons for the shapes below.
#include "fp6_cast_common.h"
#include "fp6_dequant.h"

namespace {

constexpr int kCastStoreBytes = 8;                       // the store form deepep_cast_fp6_mx runs (cast_fp6_kernel)

// (the cast back's conversion: dequant32_fp6 of fp6_dequant.h, shared with requant_t.hip)

// The 48 bytes of a lane pair (group u even: bytes [24u, 24u + 48) of the row) as three aligned 16-byte vectors: every
// lane stores `a` at a_off(u) -- the even lane its dwords 0-3 at 24u, the odd lane its dwords 2-5 at 24u + 8 -- and
// the even lane stores `b`, its dwords 4-5 and the odd lane's 0-1, at 24u + 16.  Every lane of the pair must be active.
struct PairVecs {
    u32x4 a, b;
    bool even;
    __device__ __forceinline__ int a_off(int u) const { return u * kGroupBytes + (even ? 0 : 8); }
    __device__ __forceinline__ int b_off(int u) const { return u * kGroupBytes + 16; }
};

__device__ __forceinline__ PairVecs pair_vecs(const u32x6& q, int lane) {
    PairVecs p;
    p.even = (lane & 1) == 0;
    const uint32_t o0 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(q[0]), kDppXor1, 0xf, 0xf, true));
    const uint32_t o1 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(q[1]), kDppXor1, 0xf, 0xf, true));
    p.a = p.even ? u32x4{q[0], q[1], q[2], q[3]} : u32x4{q[2], q[3], q[4], q[5]};
    p.b = u32x4{q[4], q[5], o0, o1};
    return p;
}

// a 16-byte store into a destination row that may lie in a peer window (system scope there, as put8)
template <bool kPeer>
__device__ __forceinline__ void put16(uint8_t* row, int off, const u32x4& v, int row_bytes) {
    if constexpr (kPeer) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, row_bytes, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 17);          // sc0 sc1: system scope
    } else {
        *reinterpret_cast<u32x4*>(row + off) = v;
    }
}

// the group's four 16-byte loads (zeros past the row: u >= nvec)
__device__ __forceinline__ void load_group(const u32x4* xs, int u, int nvec, u32x4* ab) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ab[j] = u32x4{0u, 0u, 0u, 0u};
    if (u < nvec) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ab[j] = __builtin_nontemporal_load(xs + 4 * u + j);
    }
}

// ---------------------------------------------------------------- the cast
// One wave per row: q [num_rows][3 * hidden / 4] and sf [num_rows][hidden / 32], both contiguous; every input row is
// read once.  A lane holds one group (four 16-byte loads), 4 lanes hold 128 columns = one dword of exponent bytes,
// stored by their first lane; a pass of the wave is 2048 columns, the next pass's loads in flight (hidden % 128 == 0:
// the 4 lanes of a dword are inside the row of x or outside).  kPair: the pair's three 16-byte stores; else three
// 8-byte stores a lane (plain stores either way; deepep_cast_fp6_mx runs the form measured faster, CHANGELOG).
template <bool kPair>
__global__ void __launch_bounds__(64)
cast_fp6_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden, uint8_t* __restrict__ q,
                uint32_t* __restrict__ sf) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const u32x4* xs = reinterpret_cast<const u32x4*>(x + t * x_stride);
    uint8_t* qs = q + t * (hidden / 4 * 3);
    uint32_t* sfs = sf + t * (hidden / 128);
    const int nvec = hidden / 32;
    u32x4 next[4];
    load_group(xs, lane, nvec, next);
    for (int u0 = 0; u0 < nvec; u0 += 64) {
        const int u = u0 + lane;
        const u32x4 raw[4] = {next[0], next[1], next[2], next[3]};
        load_group(xs, u + 64, nvec, next);              // in flight while this group is reduced and cast
        const Fp6Lane c = cast_group_fp6(raw);
        const uint32_t w = ue8m0_or4<1>(c.byte, lane);
        if constexpr (kPair) {
            const PairVecs p = pair_vecs(c.q, lane);
            if (u < nvec) {                              // plain stores: the dispatch reads them right back
                *reinterpret_cast<u32x4*>(qs + p.a_off(u)) = p.a;
                if (p.even) *reinterpret_cast<u32x4*>(qs + p.b_off(u)) = p.b;
            }
        } else if (u < nvec) {
            u32x2* o = reinterpret_cast<u32x2*>(qs + u * kGroupBytes);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = u32x2{c.q[2 * j], c.q[2 * j + 1]};
        }
        if (u < nvec && (lane & 3) == 0) sfs[u >> 2] = w;
    }
}

// ---------------------------------------------------------------- the cast back
// out bf16 [num_rows][hidden], contiguous.  A lane holds one group: three 8-byte loads (24 bytes at 24u), one factor,
// and stores the 64 bytes of bf16 as four 16-byte stores.  One wave per row, 2048 columns a pass, the next pass's
// loads in flight.  The scale factors are addressed by byte strides.  Column stride 1 and rows 4 bytes apart: the
// first lane of every quad loads the dword of its four groups and hands it on; any other strides: every lane loads its
// own byte.
constexpr int kCastBackWaves = 4;                              // rows per workgroup, one wave each

__global__ void __launch_bounds__(64 * kCastBackWaves)
cast_back_fp6_kernel(const uint8_t* __restrict__ q, int64_t q_stride, const uint8_t* __restrict__ sf,
                     int64_t sf_row_stride, int64_t sf_col_stride, int num_rows, int hidden,
                     uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kCastBackWaves +
                      __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= num_rows) return;
    const u32x2* qs = reinterpret_cast<const u32x2*>(q + t * q_stride);
    const uint8_t* sfs = sf + t * sf_row_stride;
    u32x4* os = reinterpret_cast<u32x4*>(out + t * hidden * 2);
    const int nvec = hidden / 32;
    // a lane past the row loads nothing (whole quads: hidden % 128 == 0)
    auto load = [&](int u) {
        u32x6 r = {0u, 0u, 0u, 0u, 0u, 0u};
        if (u < nvec) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x2 d = __builtin_nontemporal_load(qs + 3 * u + j);
                r[2 * j] = d[0];
                r[2 * j + 1] = d[1];
            }
        }
        return r;
    };
    const bool sf_dwords = sf_col_stride == 1 && (sf_row_stride & 3) == 0;               // wave-uniform
    auto load_sf = [&](int u) {
        uint32_t w = 0;
        if (u < nvec) {
            if (!sf_dwords) w = sfs[u * sf_col_stride];
            else if ((lane & 3) == 0) w = reinterpret_cast<const uint32_t*>(sfs)[u >> 2];
        }
        return w;
    };
    u32x6 next = load(lane);
    uint32_t next_sf = load_sf(lane);
    for (int u0 = 0; u0 < nvec; u0 += 64) {
        const int u = u0 + lane;
        const u32x6 raw = next;
        uint32_t byte = next_sf;
        if (sf_dwords) {
            const int w = __builtin_amdgcn_mov_dpp(static_cast<int>(next_sf), kDppQuadFirst, 0xf, 0xf, true);
            byte = (static_cast<uint32_t>(w) >> ((lane & 3) * 8)) & 0xffu;
        }
        const float s = deepep::ue8m0_factor(byte);
        next = load(u + 64);                                 // in flight while this group is converted
        next_sf = load_sf(u + 64);
        if (u < nvec) {
            u32x4 r[4];
            deepep::dequant32_fp6(raw, s, r);
#pragma unroll
            for (int j = 0; j < 4; ++j) os[4 * u + j] = r[j];
        }
    }
}

// ---------------------------------------------------------------- the EP > 1 pack with the cast on the way
// pack_cast_fp4_kernel over e2m3 rows: the token's bf16 row is read once and quantised in registers (the cast kernel's
// tiling), the codes and the exponent bytes go into the packed row of every destination: layout
// [3 * hidden / 4 codes | hidden / 32 exponent bytes @sf_off | topk_idx | weights | src] (sf_off % 4 == 0).  The codes
// leave as the pair's three 16-byte stores (put16<kPeer>), the exponent bytes as dwords with put<kPeer>, as every
// other field: never a byte store into a window.
template <bool kPeer>
__global__ void __launch_bounds__(64)
pack_cast_fp6_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int hidden,
                     const int64_t* __restrict__ topk_idx, const float* __restrict__ topk_weights, int K,
                     int32_t src_base, const int32_t* __restrict__ dst_slot, const int32_t* __restrict__ send_offsets,
                     int R, uint8_t* __restrict__ packed, const uint64_t* __restrict__ dest_bases, int64_t row_bytes,
                     int64_t dest_rows, int sf_off, int idx_off, int w_off, int src_off,
                     int32_t* __restrict__ error_flag) {
    const int t = blockIdx.x, lane = threadIdx.x;
    // a timed-out window barrier before this push: nothing is stored into the peers (as pack_kernel)
    if (kPeer && error_flag != nullptr &&
        (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;
    const uint64_t my_row = pack_dest_row<kPeer>(t, lane, dst_slot, send_offsets, R, packed, dest_bases, row_bytes,
                                                 dest_rows, error_flag);
    const uint64_t dmask = __ballot(my_row != 0);
    const u32x4* xs = reinterpret_cast<const u32x4*>(x + t * x_stride);
    const int nvec = hidden / 32;
    for (int u0 = 0; u0 < nvec; u0 += 64) {
        const int u = u0 + lane;
        const bool in = u < nvec;
        u32x4 raw[4];
        load_group(xs, u, nvec, raw);
        const Fp6Lane c = cast_group_fp6(raw);
        const uint32_t w = ue8m0_or4<1>(c.byte, lane);
        const PairVecs p = pair_vecs(c.q, lane);
        for (uint64_t m = dmask; m; m &= m - 1) {
            uint8_t* row = pack_row_of(my_row, __builtin_ctzll(m));
            if (in) {
                put16<kPeer>(row, p.a_off(u), p.a, static_cast<int>(row_bytes));
                if (p.even) put16<kPeer>(row, p.b_off(u), p.b, static_cast<int>(row_bytes));
                if ((lane & 3) == 0) put<kPeer>(reinterpret_cast<uint32_t*>(row + sf_off) + (u >> 2), w);
            }
        }
    }
    pack_tail<kPeer>(t, lane, my_row, dmask, topk_idx, topk_weights, K, src_base, idx_off, w_off, src_off);
}

// ---------------------------------------------------------------- the one-rank copy with the cast on the way
// copy_cast_fp4_kernel / copy_cast_expanded_fp4_kernel over e2m3 rows.  The codes leave as the pair's three 16-byte
// stores, and unlike the siblings' these are not write-through: the two store instructions of a wave interleave
// inside every 128-byte line (16 bytes of every 48 come with the second one), and written through (sc1) each leaves
// as a partial line -- the cached expanded dispatch took 395 us at 8192 x 7168, against 110 us with the L2 merging
// them (plain stores; nt in the expanded copy).  A lane is one group: four 16-byte loads through the row's buffer
// descriptor (a lane past the row end loads zeros), the amax in-lane, and the four lanes of a quad form one dword of
// exponent bytes (two DPP steps), stored by the quad's first lane.  A column chunk is 128 groups per row = 3 KiB of
// codes = 4096 columns, read as 8 KiB of bf16: eight 16-byte loads per lane and row.
constexpr int kCastChunkVecs = 128;                      // groups: 64 lanes x 2
constexpr int kBlockRows = DEEPEP_DISPATCH_BLOCK_ROWS;

// the 64 bytes of bf16 behind group u of a row (the descriptor's range check: zeros past the row end)
__device__ __forceinline__ void load32(const uint8_t* row, int hidden, int u, u32x4* ab) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(row), 0, hidden * 2,
                                                                        0x00020000);
#pragma unroll
    for (int j = 0; j < 4; ++j) ab[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, u * 64 + 16 * j, 0, 0);
}

// The pair's three 16-byte stores through the destination row's descriptor (row_q = 3 * hidden / 4 bytes): its range
// check drops the lanes past the row end, whose offsets start at or past row_q; the odd lane's `b` goes to row_q too.
template <int kAux>
__device__ __forceinline__ void store_pair(const u32x6& q, int u, int lane, const __amdgpu_buffer_rsrc_t& rs,
                                           int row_q) {
    const PairVecs p = pair_vecs(q, lane);
    __builtin_amdgcn_raw_buffer_store_b128(p.a, rs, p.a_off(u), 0, kAux);
    __builtin_amdgcn_raw_buffer_store_b128(p.b, rs, p.even ? p.b_off(u) : row_q, 0, kAux);
}

// Group u of one destination row: the cast, the row stores and, from the first lane of a quad inside the row, the
// quad's exponent bytes (a plain dword store; sf_row: the destination row's hidden / 128 dwords).
template <int kAux>
__device__ __forceinline__ void cast_store32(const u32x4* ab, int u, bool in, int lane,
                                             const __amdgpu_buffer_rsrc_t& rs, int row_q,
                                             uint32_t* __restrict__ sf_row) {
    const Fp6Lane c = cast_group_fp6(ab);
    store_pair<kAux>(c.q, u, lane, rs, row_q);
    const uint32_t w = ue8m0_or4<1>(c.byte, lane);
    if (in && (lane & 3) == 0) sf_row[u >> 2] = w;
}

// copy_cast_kernel's form: work item = (received row, column chunk), one wave per item; the row goes to recv_x[i]
// (non-expanded) or to every local slot of the row (expanded; lane k holds slot k's row), weights as copy_kernel's
// (chunk 0).  Row stores are plain (see above).  recv_sf: [num_out_rows][hidden / 128] dwords.
__global__ void __launch_bounds__(256)
copy_cast_fp6_kernel(const uint8_t* __restrict__ packed, int64_t row_bytes, int w_off, int N, int K,
                     const int32_t* __restrict__ meta, int expanded, const uint8_t* __restrict__ x, int64_t x_stride,
                     int hidden, int num_max_tokens, uint8_t* __restrict__ recv_x, uint32_t* __restrict__ recv_sf,
                     float* __restrict__ recv_w, int64_t num_out_rows, const int32_t* __restrict__ row_map,
                     int32_t* __restrict__ error_flag) {
    const int lane = threadIdx.x & 63;
    if (error_flag != nullptr && (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;                                            // a timed-out window barrier: store nothing
    const int nvec = hidden / 32;
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
    const int row_q = hidden / 4 * 3, sf_n = hidden / 128;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (c * kCastChunkVecs + p * 64 >= nvec) break;    // wave-uniform: no group of this half is in the row
        const int u = c * kCastChunkVecs + p * 64 + lane;
        const bool in = u < nvec;
        u32x4 ab[4];
        load32(xs, hidden, u, ab);
        const Fp6Lane q = cast_group_fp6(ab);
        const uint32_t w = ue8m0_or4<1>(q.byte, lane);
        const PairVecs pv = pair_vecs(q.q, lane);
        for (uint64_t m = dmask; m; m &= m - 1) {
            const int64_t d = __builtin_amdgcn_readlane(my_dst, __builtin_ctzll(m));
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(recv_x + d * row_q, 0, row_q,
                                                                                0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(pv.a, rs, pv.a_off(u), 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(pv.b, rs, pv.even ? pv.b_off(u) : row_q, 0, 0);
            if (in && (lane & 3) == 0) recv_sf[d * sf_n + (u >> 2)] = w;
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

// copy_cast_expanded_kernel's form: the blocked destination-major tiling -- one wave per (block of kBlockRows received
// rows, local expert, column chunk) writes the run of consecutive expanded rows [block_offsets[b][e],
// block_offsets[b + 1][e]) and finds their sources through inv; workgroups w = x (mod 8) run on XCD x and take blocks
// x, x + 8, ..., so a block's bf16 source rows are read once from HBM and re-read (and re-quantised) once per local
// expert from that XCD's L2.  Row stores are streaming (nt; not write-through, see above), exponent bytes and weights plain.
__global__ void __launch_bounds__(256)
copy_cast_expanded_fp6_kernel(const uint8_t* __restrict__ packed, int64_t row_bytes, int w_off, int N, int K,
                              const int32_t* __restrict__ meta, const uint8_t* __restrict__ x, int64_t x_stride,
                              int hidden, int num_max_tokens, const int32_t* __restrict__ inv,
                              const int32_t* __restrict__ block_offsets, const int32_t* __restrict__ expert_end,
                              int nb, int epr, uint8_t* __restrict__ recv_x, uint32_t* __restrict__ recv_sf,
                              float* __restrict__ recv_w, int64_t num_out_rows, const int32_t* __restrict__ row_map,
                              int32_t* __restrict__ error_flag) {
    constexpr int kRows = 4;                               // destination rows in flight per wave
    constexpr int kAux = 2;                                // nt
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (error_flag != nullptr && (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2))
        return;                                            // a timed-out window barrier: store nothing
    const int nvec = hidden / 32;
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
    const int row_q = hidden / 4 * 3, sf_n = hidden / 128;
    for (int j = r0; j < r1; j += kRows) {
        int32_t src_i[kRows], src_k[kRows];
        u32x4 a[kRows][8];
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
                    load32(xs, hidden, u0, a[q]);
                    if (half1) load32(xs, hidden, u1, a[q] + 4);
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
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(recv_x + d * row_q, 0, row_q,
                                                                                0x00020000);
            uint32_t* sf_row = recv_sf + d * sf_n;
            cast_store32<kAux>(a[q], u0, in0, lane, rs, row_q, sf_row);
            if (half1) cast_store32<kAux>(a[q] + 4, u1, in1, lane, rs, row_q, sf_row);
            if (c != 0) continue;
            if (recv_w != nullptr && lane == 0) {
                const int64_t prow = row_map != nullptr ? static_cast<int64_t>(row_map[src_i[q]]) : src_i[q];
                recv_w[d] = reinterpret_cast<const float*>(packed + prow * row_bytes + w_off)[src_k[q]];
            }
        }
    }
}

// hidden (and, where the entry takes one, a non-negative row count): rows of whole dwords of exponent bytes
int bad_hidden(const char* what, int hidden, int num_rows = 0) {
    if (num_rows >= 0 && hidden >= 128 && hidden % 128 == 0) return DEEPEP_OK;
    return invalid(what, "hidden must be a positive multiple of 128");
}

int cast_fp6(const char* what, const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q,
             uint8_t* sf, int store_bytes, deepep_stream_t stream) {
    if (num_rows == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden(what, hidden, num_rows)) return rc;
    if (store_bytes != 8 && store_bytes != 16) return invalid(what, "store_bytes must be 8 or 16");
    if (x == nullptr || q == nullptr || sf == nullptr || !a16(x) || !a16(q) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden * 2 bytes or not 16-byte aligned");
    const auto kernel = store_bytes == 16 ? cast_fp6_kernel<true> : cast_fp6_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(num_rows), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, static_cast<uint8_t*>(q),
                       reinterpret_cast<uint32_t*>(sf));
    return launch_status(what);
}

}  // namespace

extern "C" {

int deepep_cast_fp6_mx(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, uint8_t* sf,
                       deepep_stream_t stream) {
    return cast_fp6("cast_fp6_mx", x, x_row_stride_bytes, num_rows, hidden, q, sf, kCastStoreBytes, stream);
}

int deepep_cast_fp6_mx_stores(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q,
                              uint8_t* sf, int store_bytes, deepep_stream_t stream) {
    return cast_fp6("cast_fp6_mx_stores", x, x_row_stride_bytes, num_rows, hidden, q, sf, store_bytes, stream);
}

int deepep_cast_back_fp6_mx(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf, int64_t sf_row_stride,
                            int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream) {
    const char* what = "cast_back_fp6_mx";
    if (num_rows == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden(what, hidden, num_rows)) return rc;
    if (q == nullptr || out == nullptr || sf == nullptr || !a16(q) || !a16(out) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (q_row_stride_bytes < static_cast<int64_t>(hidden) / 4 * 3 || q_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below 3 * hidden / 4 bytes or not 16-byte aligned");
    if (sf_row_stride < 0 || sf_col_stride < 0) return invalid(what, "negative scale-factor stride");
    // contiguous columns may be read as dwords, so their rows start on 4 bytes
    if (sf_col_stride == 1 && sf_row_stride % 4 != 0)
        return invalid(what, "scale-factor rows of unit column stride must start 4-byte aligned");
    const unsigned grid = static_cast<unsigned>((static_cast<int64_t>(num_rows) + kCastBackWaves - 1) / kCastBackWaves);
    hipLaunchKernelGGL(cast_back_fp6_kernel, dim3(grid), dim3(64 * kCastBackWaves), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(q), q_row_stride_bytes, sf,
                       sf_row_stride, sf_col_stride, num_rows, hidden, static_cast<uint8_t*>(out));
    return launch_status(what);
}

int deepep_dispatch_pack_cast_fp6_mx(const void* x, int64_t x_row_stride_bytes, int hidden, const int64_t* topk_idx,
                                     const float* topk_weights, int num_tokens, int num_topk, int32_t src_base,
                                     const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks, void* packed,
                                     const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows, int sf_off,
                                     int idx_off, int w_off, int src_off, int32_t* error_flag,
                                     deepep_stream_t stream) {
    const char* what = "dispatch_pack_cast_fp6_mx";
    if (num_tokens == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden(what, hidden)) return rc;
    if (x == nullptr || !a16(x) || x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "x null, misaligned, or its row stride below hidden * 2 bytes or not 16-byte aligned");
    // the row holds [3 * hidden / 4 codes | hidden / 32 exponent bytes @sf_off | topk_idx @idx_off | weights @w_off |
    // src @src_off]
    if (num_tokens < 0 || num_topk < 1 || num_topk > 32 || num_ranks < 1 || num_ranks > 64 || dest_rows < 0 ||
        topk_idx == nullptr || dst_slot == nullptr || send_offsets == nullptr ||
        sf_off < hidden / 4 * 3 || sf_off % 4 || idx_off < sf_off + hidden / 32 || idx_off % 8 ||
        w_off < idx_off + num_topk * 8 || w_off % 4 || src_off < w_off + num_topk * 4 || src_off % 4 ||
        row_bytes < src_off + 4 || row_bytes % 16 || (dest_bases == nullptr && (packed == nullptr || !a16(packed))))
        return invalid(what, "invalid arguments or row layout");
    const auto kernel = dest_bases != nullptr ? pack_cast_fp6_kernel<true> : pack_cast_fp6_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(num_tokens), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, topk_idx, topk_weights, num_topk,
                       src_base, dst_slot, send_offsets, num_ranks, static_cast<uint8_t*>(packed), dest_bases,
                       row_bytes, dest_rows, sf_off, idx_off, w_off, src_off, error_flag);
    return launch_status(what);
}

int deepep_dispatch_copy_cast_fp6_mx(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                     const int32_t* src_metadata, int expanded, const void* x,
                                     int64_t x_row_stride_bytes, int hidden, int num_max_tokens, void* recv_x,
                                     uint8_t* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                                     const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                                     int num_local_experts, const int32_t* row_map, int32_t* error_flag,
                                     deepep_stream_t stream) {
    const char* what = "dispatch_copy_cast_fp6_mx";
    if (num_recv == 0) return DEEPEP_OK;
    if (const int rc = bad_hidden(what, hidden)) return rc;
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
    const int nch = (hidden / 32 + kCastChunkVecs - 1) / kCastChunkVecs;
    if (inv != nullptr) {
        const int nb = (num_recv + kBlockRows - 1) / kBlockRows;
        const int64_t wg_per_block = (static_cast<int64_t>(num_local_experts) * nch + 3) / 4;
        const int64_t grid = 8 * wg_per_block * ((nb + 7) / 8);
        hipLaunchKernelGGL(copy_cast_expanded_fp6_kernel, dim3(static_cast<unsigned>(grid)), dim3(256), 0, s,
                           static_cast<const uint8_t*>(packed), row_bytes, w_off, num_recv, num_topk, src_metadata,
                           static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, num_max_tokens, inv,
                           block_offsets, expert_end, nb, num_local_experts, static_cast<uint8_t*>(recv_x),
                           reinterpret_cast<uint32_t*>(recv_sf), recv_topk_weights, num_out_rows, row_map, error_flag);
        return launch_status(what);
    }
    const int64_t items = static_cast<int64_t>(num_recv) * nch;
    hipLaunchKernelGGL(copy_cast_fp6_kernel, dim3(static_cast<unsigned>((items + 3) / 4)), dim3(256), 0, s,
                       static_cast<const uint8_t*>(packed), row_bytes, w_off, num_recv, num_topk, src_metadata,
                       expanded, static_cast<const uint8_t*>(x), x_row_stride_bytes, hidden, num_max_tokens,
                       static_cast<uint8_t*>(recv_x), reinterpret_cast<uint32_t*>(recv_sf), recv_topk_weights,
                       num_out_rows, row_map, error_flag);
    return launch_status(what);
}

}  // extern "C"
