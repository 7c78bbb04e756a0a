// swiglu_cast.hip -- SwiGLU fused into the MX casts between the experts' two GEMMs on MI355X (deepep_swiglu_cast_mx):
// h = [gate | up], bf16 [num_rows][2 * inter], as the first grouped GEMM writes it, becomes the second GEMM's operand
// -- the row-wise pair of act = silu(gate) * up, and for training the token-axis pair of the weight gradient -- in one
// read of h and without the bf16 [num_rows][inter] buffer between (it is written only when asked for: `act`).  There
// is no counterpart in the reference.
//
// Two rules.  (1) act = bf16_rne(g / (1 + exp(-g)) * u) in fp32 from the widened bf16, one rounding: swiglu() below,
// the only definition, used by both kernels.  (2) Every pair is bit for bit what the library's casts give for act:
// nothing here is new quantisation.  The rows go through cast_group_fp8<1, 32> / cast_group_fp4<1> / cast_group_fp6<1>
// (fp8_cast_common.h, fp4_cast_common.h, fp6_cast_common.h), the token axis through the tile of cast_fp8_mx_t_kernel /
// cast_mx_t_kernel restated behind a load stage, as requant_t.hip restates it (fp8_cast_t.hip and fp46_cast_t.hip stay
// as they are; their comments give the reasons for the tile's shapes).
//
// expert_ends (optional): rows at or past align_up(expert_ends[num_experts - 1], expert_alignment) -- the tail of a
// worst-case-sized handle, which the grouped GEMM leaves unwritten -- are neither read nor written, in any output.
// Every wave reads that one int32 itself; nothing is read on the host.
//
// Resources (hipcc --offload-arch=gfx950 -O3 with this file's flags, -Rpass-analysis=kernel-resource-usage; no
// instance uses scratch or AGPRs):
//   swiglu_cast_rows_kernel  FP8 / FP6 / FP4   VGPRs 62 / 66 / 60, occupancy 8 / 7 / 8 waves a SIMD, no LDS
//   swiglu_cast_t_kernel     FP8 / FP6 / FP4   VGPRs 222 / 251 / 223, occupancy 2 waves a SIMD, LDS 16.5 / 12.5 / 8.5 KiB
#include "swiglu_cast_common.h"

namespace {

// ---------------------------------------------------------------- rule 1: the activation
// g / (1 + exp(-g)) * u with t = exp(-|g|) in (0, 1]: the sigmoid is 1 / (1 + t) for g >= 0 and t / (1 + t) below, so
// 1 + t stays in (1, 2] and no finite g overflows the exponential or flushes the reciprocal.  v_exp_f32 and v_rcp_f32
// are good to 1 ulp of fp32, the argument's rounding adds |g| * 2^-24 relative: some 2^-20 in all, against the 2^-9 of
// the rounding to bf16.
__device__ __forceinline__ float swiglu(float g, float u) {
    const float t = __builtin_amdgcn_exp2f(-fabsf(g) * 1.44269504f);
    const float r = __builtin_amdgcn_rcpf(1.0f + t);
    return g * ((g < 0.0f ? t : 1.0f) * r) * u;
}

// the 8 columns of one 16-byte load of the gate and one of the up projection, as the 8 bf16 of act (v_cvt_pk_bf16_f32)
__device__ __forceinline__ u32x4 swiglu8(const u32x4& gate, const u32x4& up) {
    float g[8], u[8];
    unpack8(gate, g);
    unpack8(up, u);
    u32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        out[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{swiglu(g[2 * j], u[2 * j]),
                                                                            swiglu(g[2 * j + 1], u[2 * j + 1])}, bf16x2));
    return out;
}

// ---------------------------------------------------------------- the row-wise kernel: inference, any num_rows
// A streaming kernel: no tile, no LDS.  The work is the segments (row, block of 128 columns), column blocks fastest;
// 16 lanes take a segment -- a 256-byte run of the gate and one of the up projection, whole lines -- and the four
// segments of one wave instruction are consecutive, so a wave reads 1 KiB runs of a row where the row has them and no
// lane idles where inter is an odd multiple of 128.  A wave takes kRowsInFlight such instructions' segments, 16 in all
// and consecutive: all their loads, 2 * kRowsInFlight 16-byte non-temporal loads a lane (32 VGPRs), are issued before
// the first is used.  At 8 waves a SIMD that is 16 KiB a wave and 128 KiB a SIMD in flight; a deeper queue would only
// cost occupancy.  Stores: act 16 bytes a lane (256-byte runs), the codes 8, 8-of-6 or 4 bytes a lane (128, 96 or 64
// byte runs a segment, contiguous across the wave's segments of a row), one exponent dword a segment.
constexpr int kRowsInFlight = 4;
constexpr int kWaveSegments = 4 * kRowsInFlight;
constexpr int kRowsKernelWaves = 4;

template <int kFormat>
__global__ void __launch_bounds__(64 * kRowsKernelWaves)
swiglu_cast_rows_kernel(const uint8_t* __restrict__ h, int64_t h_stride, int64_t num_rows, int inter,
                        const int32_t* __restrict__ expert_ends, int num_experts, int expert_alignment,
                        uint8_t* __restrict__ q, uint32_t* __restrict__ sf, uint8_t* __restrict__ act, int col_blocks) {
    const int lane = threadIdx.x & 63, cl = lane & 15;
    const int64_t live = live_rows(num_rows, expert_ends, num_experts, expert_alignment);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * kRowsKernelWaves +
                         __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t s0 = wave * kWaveSegments;               // the wave's first segment: row s0 / col_blocks
    const int64_t row0 = s0 / col_blocks;
    if (row0 >= live) return;                              // wave-uniform
    // the lane's segment of instruction k is s0 + 4 k + (lane >> 4): one division, then steps of 4 segments
    const uint32_t ncb = static_cast<uint32_t>(col_blocks);
    const uint32_t first = static_cast<uint32_t>(s0 - row0 * col_blocks) + (lane >> 4);
    int64_t row = row0 + first / ncb;
    uint32_t cb = first % ncb;
    const uint32_t step_rows = 4u / ncb, step_cb = 4u % ncb;
    const int64_t q_pitch = static_cast<int64_t>(col_blocks) * (4 * kBlockBytes<kFormat>);
    int64_t rows[kRowsInFlight];
    uint32_t cbs[kRowsInFlight];
    u32x4 gate[kRowsInFlight], up[kRowsInFlight];
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) {
        rows[k] = row;
        cbs[k] = cb;
        gate[k] = up[k] = u32x4{0u, 0u, 0u, 0u};           // (a segment past the live rows still runs the quad steps)
        if (row < live) {
            const u32x4* p = reinterpret_cast<const u32x4*>(h + row * h_stride + cb * (kTile * 2)) + cl;
            gate[k] = __builtin_nontemporal_load(p);       // read once
            up[k] = __builtin_nontemporal_load(p + inter / 8);
        }
        row += step_rows;
        cb += step_cb;
        if (cb >= ncb) {
            cb -= ncb;
            ++row;
        }
    }
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) {
        const u32x4 a = swiglu8(gate[k], up[k]);
        u32x2 piece;
        uint32_t w;
        cast_row<kFormat>(a, lane, piece, w);
        if (rows[k] < live) {
            const int64_t seg = rows[k] * col_blocks + cbs[k];
            if (act != nullptr) reinterpret_cast<u32x4*>(act)[seg * 16 + cl] = a;
            uint8_t* dst = q + rows[k] * q_pitch + cbs[k] * (4 * kBlockBytes<kFormat>) + piece_off<kFormat>(cl);
            if constexpr (kFormat == DEEPEP_MX_FP4) *reinterpret_cast<uint32_t*>(dst) = piece[0];
            else if (piece_stored<kFormat>(cl)) *reinterpret_cast<u32x2*>(dst) = piece;
            if (cl == 0) sf[seg] = w;
        }
    }
}

// ---------------------------------------------------------------- the row-wise and the transposed pair: training
// One wave (a workgroup of its own) per run of up to kWaveTiles tiles of 128 tokens x 128 columns of act, the tiles
// consecutive along the token axis: cast_fp8_mx_t_kernel<true> / cast_mx_t_kernel<kFmt, true> behind a SwiGLU load
// stage.  Every tile lies inside the live rows (num_rows, expert_alignment and inter are multiples of 128).
//
// The load stage.  As in those kernels lane = 16 g + cl holds columns [8 cl, 8 cl + 8) of the 32 tokens n0 + 32 g + i
// of the tile's group g, and raw[i] is what a bf16 load of act would have given; but a token is two loads now, and
// the tile's raw[32] (128 VGPRs) leaves no room for 64 raw loads.  Gate and up stream through two buffers of
// kChunkRows tokens each (2 * 2 * kChunkRows 16-byte vectors: 64 VGPRs): the loads of chunk c + 1 are issued, then
// chunk c goes through swiglu8 into raw[].  So 4 kChunkRows = 16 loads of 16 bytes a lane are in flight while the
// wave waits and 8 while it computes, against the plain cast's 32; the buffers are dead when the tile's conversions
// start, which keeps their 200-246 VGPRs.  Through the tile's descriptors (a scalar row offset and the lane's 32-bit
// offset; the launcher bounds the row stride so that the tile's extent fits), non-temporal.
//
// After the load the tile is the casts', restated: the transposed half per element type, the row-wise half through
// cast_row, act (when asked for) stored from raw[] beside the row's codes, 16 bytes a lane.
constexpr int kChunkRows = 4;

template <int kFormat>
__global__ void __launch_bounds__(64)
swiglu_cast_t_kernel(const uint8_t* __restrict__ h, int64_t h_stride, int64_t num_rows, int inter,
                     const int32_t* __restrict__ expert_ends, int num_experts, int expert_alignment,
                     uint8_t* __restrict__ q_t, uint8_t* __restrict__ sf_t, uint8_t* __restrict__ q,
                     uint32_t* __restrict__ sf, uint8_t* __restrict__ act, int col_blocks, int64_t num_items,
                     int sf16) {
    constexpr int kColBytes = 4 * kBlockBytes<kFormat>;    // a column's bytes of one tile, and a row's
    // FP8: [column][8 slots of 16 bytes], slot ^ ((column >> 3) & 7); FP4 / FP6: fp46_cast_t.hip's image
    __shared__ __attribute__((aligned(16))) uint8_t image_bytes[kTile * kColBytes];
    // [column]: byte g the exponent byte of the tile's group g
    __shared__ __attribute__((aligned(16))) uint32_t sf_image[kTile];
    const int lane = threadIdx.x, g = lane >> 4, cl = lane & 15;
    const int64_t item = tile_item();
    if (item >= num_items) return;
    const int cb = static_cast<int>(item % col_blocks);
    const int64_t n_base = item / col_blocks * (kTile * kWaveTiles);
    const int c0 = cb * kTile;
    const int64_t left = (live_rows(num_rows, expert_ends, num_experts, expert_alignment) - n_base) / kTile;
    if (left <= 0) return;                                 // the whole run is past the live rows
    const int ntile = left < kWaveTiles ? static_cast<int>(left) : kWaveTiles;
    u32x4 acc[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
#pragma clang loop unroll(disable)
    for (int t = 0; t < ntile; ++t) {
        const int64_t n0 = n_base + t * kTile;
        u32x4 raw[32];
        {
            const uint32_t stride32 = static_cast<uint32_t>(h_stride);
            const uint8_t* tile = h + n0 * h_stride + c0 * 2;
            const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(tile), 0, (kTile - 1) * stride32 + kTile * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(tile + static_cast<int64_t>(inter) * 2), 0, (kTile - 1) * stride32 + kTile * 2,
                0x00020000);
            const uint32_t lane_off = 32u * g * stride32 + 16u * cl;
            u32x4 gate[2][kChunkRows], up[2][kChunkRows];
#pragma unroll
            for (int i = 0; i < kChunkRows; ++i) {
                gate[0][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, lane_off, i * stride32, 2);    // nt: read once
                up[0][i] = __builtin_amdgcn_raw_buffer_load_b128(ru, lane_off, i * stride32, 2);
            }
#pragma unroll
            for (int c = 0; c < 32 / kChunkRows; ++c) {
                if (c + 1 < 32 / kChunkRows) {
#pragma unroll
                    for (int i = 0; i < kChunkRows; ++i) {
                        const uint32_t off = ((c + 1) * kChunkRows + i) * stride32;
                        gate[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, lane_off, off, 2);
                        up[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(ru, lane_off, off, 2);
                    }
                }
#pragma unroll
                for (int i = 0; i < kChunkRows; ++i) raw[c * kChunkRows + i] = swiglu8(gate[c & 1][i], up[c & 1][i]);
                __builtin_amdgcn_sched_barrier(0);         // a chunk at a time: the next one's loads stay in front
            }
        }
        // the transposed half: per column, the amax of the lane's 32 tokens, the scale rule, the codes
        u16x2 m[4];
        token_amax(raw, m);
        uint8_t* sf_bytes = reinterpret_cast<uint8_t*>(sf_image);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int col = 8 * cl + c;
            uint32_t byte;
            if constexpr (kFormat == DEEPEP_MX_FP8) {
                u32x4* image = reinterpret_cast<u32x4*>(image_bytes);
                // (a bf16 magnitude orders as its bits, and is the high half of the fp32 of the same value)
                const float amax = fmaxf(1e-4f, __uint_as_float(static_cast<uint32_t>(m[c >> 1][c & 1]) << 16));
                float scale, factor;
                group_scales(amax, 1, scale, factor);
                byte = ue8m0_byte(factor);
                uint32_t d[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float f[8];                            // tokens 8k .. 8k + 7 of column c
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t w = raw[8 * k + i][c >> 1];
                        f[i] = __uint_as_float((c & 1) ? w & 0xffff0000u : w << 16);
                    }
                    const u32x2 e = cvt8(f, scale);
                    d[2 * k] = e[0];
                    d[2 * k + 1] = e[1];
                    __builtin_amdgcn_sched_barrier(0);     // 8 tokens' temporaries at a time beside raw[]
                }
                image[col * 8 + ((2 * g) ^ (cl & 7))] = u32x4{d[0], d[1], d[2], d[3]};
                image[col * 8 + ((2 * g + 1) ^ (cl & 7))] = u32x4{d[4], d[5], d[6], d[7]};
            } else {
                const float amax = amax_floor(m[c >> 1][c & 1]);
                const int p = 16 * c + cl;                 // the image's place of column 8 cl + c
                if constexpr (kFormat == DEEPEP_MX_FP4) {
                    u32x4* image = reinterpret_cast<u32x4*>(image_bytes);
                    byte = fp4_exp_byte(amax);
                    const float factor = deepep::ue8m0_factor(byte);
                    u32x4 d;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        u32x4 pr;                          // tokens 8k .. 8k + 7 of column c
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            pr[j] = pair_tokens(raw[8 * k + 2 * j][c >> 1], raw[8 * k + 2 * j + 1][c >> 1], c & 1);
                        d[k] = cvt8_fp4(pr, factor);
                        __builtin_amdgcn_sched_barrier(0); // 8 tokens' temporaries at a time beside raw[]
                    }
                    image[(4 * p + g) ^ ((cl >> 2) & 3)] = d;
                } else {
                    u32x2* image = reinterpret_cast<u32x2*>(image_bytes);
                    byte = fp6_exp_byte(amax);
                    const float factor = deepep::ue8m0_factor(byte);
                    u32x16 v;                              // the 32 tokens of column c
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        v[j] = pair_tokens(raw[2 * j][c >> 1], raw[2 * j + 1][c >> 1], c & 1);
                    const u32x6 d = cvt32_fp6(v, factor);
#pragma unroll
                    for (int j = 0; j < 3; ++j) image[12 * p + 3 * g + j] = u32x2{d[2 * j], d[2 * j + 1]};
                    __builtin_amdgcn_sched_barrier(0);     // one column's temporaries at a time beside raw[]
                }
            }
            sf_bytes[col * 4 + g] = static_cast<uint8_t>(byte);
        }
        // the row-wise half and act (stores as loads: a descriptor over what the tile may write, a scalar offset per
        // row and the lane's 32-bit offset; the launcher bounds inter so that the extents fit)
        {
            const uint32_t i32 = static_cast<uint32_t>(inter);
            const uint32_t q_pitch = i32 / 32 * kBlockBytes<kFormat>, sf_pitch = i32 / 32, act_pitch = i32 * 2;
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
                q + n0 * q_pitch + cb * kColBytes, 0, (kTile - 1) * q_pitch + kColBytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsf = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<uint8_t*>(sf) + n0 * sf_pitch + cb * 4, 0, (kTile - 1) * sf_pitch + 4, 0x00020000);
            // (act == nullptr: a descriptor of no bytes, never used)
            const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
                act + (act != nullptr ? n0 * act_pitch + c0 * 2 : 0), 0,
                act != nullptr ? (kTile - 1) * act_pitch + kTile * 2 : 0u, 0x00020000);
            const uint32_t q_off = 32u * g * q_pitch + piece_off<kFormat>(cl), sf_off = 32u * g * sf_pitch;
            const uint32_t act_off = 32u * g * act_pitch + 16u * cl;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                // (the row's dwords through an empty asm: the compiler then works on them here, for this row alone)
                u32x4 row = raw[i];
                asm volatile("" : "+v"(row));
                if (act != nullptr) __builtin_amdgcn_raw_buffer_store_b128(row, ra, act_off, i * act_pitch, 0);
                u32x2 piece;
                uint32_t w;
                cast_row<kFormat>(row, lane, piece, w);
                if constexpr (kFormat == DEEPEP_MX_FP4)
                    __builtin_amdgcn_raw_buffer_store_b32(piece[0], rq, q_off, i * q_pitch, 0);
                else if (piece_stored<kFormat>(cl))
                    __builtin_amdgcn_raw_buffer_store_b64(piece, rq, q_off, i * q_pitch, 0);
                if (cl == 0) __builtin_amdgcn_raw_buffer_store_b32(w, rsf, sf_off, i * sf_pitch, 0);
                __builtin_amdgcn_sched_barrier(0);         // one row's temporaries at a time beside raw[]
            }
        }
        __syncthreads();
        if constexpr (kFormat == DEEPEP_MX_FP8) {
            // (a descriptor over what the tile may write and the lane's 32-bit offset; the launcher bounds num_rows so
            // that the extents fit, and the descriptor's range check drops anything outside them)
            const u32x4* image = reinterpret_cast<const u32x4*>(image_bytes);
            const uint32_t n32 = static_cast<uint32_t>(num_rows);
            const uint32_t qt_off = (lane >> 3) * n32 + 16u * (lane & 7);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int col = (lane >> 3) + 8 * k;       // (col >> 3) & 7 == k & 7
                const u32x4 v = image[col * 8 + ((lane & 7) ^ (k & 7))];
                const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
                    q_t + (c0 + 8 * k) * num_rows + n0, 0, 7 * n32 + kTile, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(v, rk, qt_off, 0, 0);
            }
        } else {
            // the tile's share of q_t: row c0 + column, bytes [n0 / 32 * kBlockBytes, + kColBytes) (64-bit addresses:
            // nothing else is live here)
            const int64_t qt_pitch = num_rows / 32 * kBlockBytes<kFormat>;
            uint8_t* qt_tile = q_t + c0 * qt_pitch + n0 / 32 * kBlockBytes<kFormat>;
#pragma unroll
            for (int k = 0; k < kColBytes / 16 * 2; ++k) {
                const int i = 64 * k + lane;               // the image's 16 bytes at 16 i: place p, 16-byte piece
                int p, piece;
                u32x4 v;
                if constexpr (kFormat == DEEPEP_MX_FP4) {
                    p = i >> 2;
                    piece = i & 3;
                    v = reinterpret_cast<const u32x4*>(image_bytes)[i ^ ((lane >> 4) & 3)];
                } else {
                    p = i / 6;
                    piece = i - 6 * p;
                    const u32x2* image = reinterpret_cast<const u32x2*>(image_bytes);
                    const u32x2 a = image[2 * i], b = image[2 * i + 1];
                    v = u32x4{a[0], a[1], b[0], b[1]};
                }
                const int col = 8 * (p & 15) + (p >> 4);
                *reinterpret_cast<u32x4*>(qt_tile + col * qt_pitch + 16 * piece) = v;
            }
        }
        keep_sf(acc, sf_image, t, lane);
        __syncthreads();                                   // the image is free for the next tile
    }
    store_sf(acc, sf_t, num_rows, c0, n_base, ntile, sf16, lane);
}

// ---------------------------------------------------------------- the checks and the launches, over the element type
struct Args {
    const uint8_t* h;
    int64_t h_stride;
    int num_rows, inter;
    const int32_t* expert_ends;
    int num_experts, expert_alignment;
    uint8_t *q, *sf, *q_t, *sf_t, *act;
    hipStream_t stream;
};

template <int kFormat>
int swiglu_cast(const char* what, const Args& a) {
    const int col_blocks = a.inter / kTile;
    if (a.q_t == nullptr) {
        const int64_t segments = static_cast<int64_t>(a.num_rows) * col_blocks;
        constexpr int kGroupSegments = kWaveSegments * kRowsKernelWaves;
        const int64_t grid = (segments + kGroupSegments - 1) / kGroupSegments;
        if (grid > 0x7fffffff) return invalid(what, "too many segments for one launch");
        hipLaunchKernelGGL(swiglu_cast_rows_kernel<kFormat>, dim3(static_cast<unsigned>(grid)),
                           dim3(64 * kRowsKernelWaves), 0, a.stream, a.h, a.h_stride,
                           static_cast<int64_t>(a.num_rows), a.inter, a.expert_ends, a.num_experts, a.expert_alignment,
                           a.q, reinterpret_cast<uint32_t*>(a.sf), a.act, col_blocks);
        return launch_status(what);
    }
    const int64_t runs = (static_cast<int64_t>(a.num_rows) + kTile * kWaveTiles - 1) / (kTile * kWaveTiles);
    const int64_t num_items = runs * col_blocks;
    const int64_t grid = (num_items + 7) / 8 * 8;
    if (grid > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const int sf16 = a.num_rows % (kTile * kWaveTiles) == 0 && a16(a.sf_t);
    hipLaunchKernelGGL(swiglu_cast_t_kernel<kFormat>, dim3(static_cast<unsigned>(grid)), dim3(64), 0, a.stream, a.h,
                       a.h_stride, static_cast<int64_t>(a.num_rows), a.inter, a.expert_ends, a.num_experts,
                       a.expert_alignment, a.q_t, a.sf_t, a.q, reinterpret_cast<uint32_t*>(a.sf), a.act, col_blocks,
                       num_items, sf16);
    return launch_status(what);
}

}  // namespace

extern "C" {

int deepep_swiglu_cast_mx(int format, const void* h, int64_t h_row_stride_bytes, void* q, uint8_t* sf, void* q_t,
                          uint8_t* sf_t, void* act, const int32_t* expert_ends, int num_experts, int expert_alignment,
                          int num_rows, int inter, deepep_stream_t stream) {
    const char* what = "swiglu_cast_mx";
    if (num_rows == 0) return DEEPEP_OK;
    if (format != DEEPEP_MX_FP8 && format != DEEPEP_MX_FP6 && format != DEEPEP_MX_FP4)
        return invalid(what, "format is DEEPEP_MX_FP8, DEEPEP_MX_FP6 or DEEPEP_MX_FP4");
    if (inter < kTile || inter % kTile != 0) return invalid(what, "inter must be a positive multiple of 128");
    if ((q_t == nullptr) != (sf_t == nullptr))
        return invalid(what, "the transposed pair is both q_t and sf_t, or neither");
    if (num_rows < 0 || (q_t != nullptr && num_rows % kTile != 0))
        return invalid(what, "num_rows must not be negative, and a multiple of 128 with the transposed pair (four "
                             "groups of 32 tokens to a scale-factor dword)");
    if (h == nullptr || q == nullptr || sf == nullptr || !a16(h) || !a16(q) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0 || !a16(act))
        return invalid(what, "null or misaligned pointers (16-byte aligned rows, 4-byte aligned scale factors)");
    if (q_t != nullptr && (!a16(q_t) || (reinterpret_cast<uintptr_t>(sf_t) & 3u) != 0))
        return invalid(what, "misaligned transposed outputs (16-byte aligned rows, 4-byte aligned scale factors)");
    if (h_row_stride_bytes < static_cast<int64_t>(inter) * 4 || h_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below 2 * inter * 2 bytes or not 16-byte aligned");
    // the tile addresses h, q, sf, act and q_t through 32-bit offsets from the tile's own base (the bases are 64-bit)
    if (h_row_stride_bytes > (1 << 24) || inter > (1 << 24) || num_rows >= (1 << 29))
        return invalid(what, "row stride or inter above 2^24, or 2^29 rows or more");
    if (expert_ends != nullptr &&
        (num_experts < 1 || expert_alignment < 1 || (q_t != nullptr && expert_alignment % kTile != 0)))
        return invalid(what, "expert_ends needs num_experts >= 1 and a positive expert_alignment, a multiple of 128 "
                             "with the transposed pair");
    const Args a{static_cast<const uint8_t*>(h), h_row_stride_bytes, num_rows, inter, expert_ends, num_experts,
                 expert_alignment, static_cast<uint8_t*>(q), sf, static_cast<uint8_t*>(q_t), sf_t,
                 static_cast<uint8_t*>(act), reinterpret_cast<hipStream_t>(stream)};
    if (format == DEEPEP_MX_FP8) return swiglu_cast<DEEPEP_MX_FP8>(what, a);
    if (format == DEEPEP_MX_FP6) return swiglu_cast<DEEPEP_MX_FP6>(what, a);
    return swiglu_cast<DEEPEP_MX_FP4>(what, a);
}

}  // extern "C"
