// swiglu_backward_cast.hip -- SwiGLU's backward fused into the MX casts on MI355X (deepep_swiglu_backward_cast_mx):
// h = [gate | up], bf16 [num_rows][2 * inter], what the forward consumed, and dact, bf16 [num_rows][inter], the
// gradient of act = silu(gate) * up as the dgrad GEMM of W2 writes it, become dh = [dgate | dup] as the operands of
// the first GEMM's two gradients -- the row-wise pair for dX = dh . W13, the token-axis pair for dW13 = dh^T . X --
// without the bf16 [num_rows][2 * inter] buffer between (it is written only when asked for: `dh`).  There is no
// counterpart in the reference.
//
// Two rules, the forward's.  (1) dgate and dup in fp32 from the widened bf16, one rounding each: swiglu_backward()
// below, the only definition, used by both kernels.  (2) Every pair is bit for bit what the library's casts give for
// dh: the rows go through cast_row (swiglu_cast_common.h), the token axis through the tile of cast_fp8_mx_t_kernel /
// cast_mx_t_kernel restated behind a load stage, as swiglu_cast.hip restates it.
//
// expert_ends (optional): rows at or past align_up(expert_ends[num_experts - 1], expert_alignment) are neither read,
// in h or in dact, nor written, in any output.  Every wave reads that one int32 itself; nothing is read on the host.
//
// Resources (hipcc --offload-arch=gfx950 -O3 with this file's flags, -Rpass-analysis=kernel-resource-usage; no
// instance uses scratch or AGPRs):
//   swiglu_backward_cast_rows_kernel  FP8 / FP6 / FP4   VGPRs 64 / 73 / 60, occupancy 8 / 6 / 8 waves a SIMD, no LDS
//   swiglu_backward_cast_t_kernel     FP8 / FP6 / FP4   VGPRs 180 / 255 / 180, occupancy 2 waves a SIMD, LDS 20 / 16 / 12 KiB
#include "swiglu_cast_common.h"

namespace {

// ---------------------------------------------------------------- rule 1: the activation's derivative
// With t = exp(-|g|) in (0, 1] and r = 1 / (1 + t): sigmoid(g) = s is r for g >= 0 and t r below, and 1 - sigmoid(g)
// = c is the other of the two -- never a subtraction, so c keeps its relative accuracy where s is near 1.  Then
//   dgate = da * u * (s * (1 + g c))        dup = da * (g * s)
// 1 + t stays in (1, 2]: no finite g overflows the exponential or flushes the reciprocal.  v_exp_f32 and v_rcp_f32 are
// good to 1 ulp of fp32; silu' has a zero near g = -1.2785, where bf16 values of g are 2^-7 apart, so |1 + g c| is
// some 2^-9 at the least on representable inputs and the relative error stays near 2^-13, against the 2^-9 of the
// rounding to bf16.  1 + g c is one fused multiply-add, written out so that both kernels round alike.
__device__ __forceinline__ void swiglu_backward(float g, float u, float da, float& dgate, float& dup) {
    const float t = __builtin_amdgcn_exp2f(-fabsf(g) * 1.44269504f);
    const float r = __builtin_amdgcn_rcpf(1.0f + t);
    const float tr = t * r;
    const float s = g < 0.0f ? tr : r, c = g < 0.0f ? r : tr;
    dgate = da * u * (s * __builtin_fmaf(g, c, 1.0f));
    dup = da * (g * s);
}

__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {      // v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

// the 8 columns of one 16-byte load each of the gate, the up projection and dact, as the 8 bf16 of dgate and of dup
__device__ __forceinline__ void swiglu_backward8(const u32x4& gate, const u32x4& up, const u32x4& dact, u32x4& dgate,
                                                 u32x4& dup) {
    float g[8], u[8], da[8], dg[8], du[8];
    unpack8(gate, g);
    unpack8(up, u);
    unpack8(dact, da);
#pragma unroll
    for (int j = 0; j < 8; ++j) swiglu_backward(g[j], u[j], da[j], dg[j], du[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dgate[j] = bf16_pair(dg[2 * j], dg[2 * j + 1]);
        dup[j] = bf16_pair(du[2 * j], du[2 * j + 1]);
    }
}

// one half alone (the tile kernel makes dh a half at a time; the same arithmetic, the other result dropped)
__device__ __forceinline__ u32x4 swiglu_backward8_gate(const u32x4& gate, const u32x4& up, const u32x4& dact) {
    u32x4 dgate, dup;
    swiglu_backward8(gate, up, dact, dgate, dup);
    return dgate;
}

__device__ __forceinline__ u32x4 swiglu_backward8_up(const u32x4& gate, const u32x4& dact) {
    u32x4 dgate, dup;
    swiglu_backward8(gate, u32x4{0u, 0u, 0u, 0u}, dact, dgate, dup);
    return dup;
}

// ---------------------------------------------------------------- the row-wise kernel: inference-style, any num_rows
// The forward's streaming kernel with a third load and a second output segment.  The work is the segments (row, block
// b of 128 columns of inter), column blocks fastest; 16 lanes take a segment -- a 256-byte run each of the gate, the up
// projection and dact -- and the four segments of one wave instruction are consecutive.  A segment yields two
// segments of dh's row: dgate at column block b and dup at column block inter / 128 + b, each through cast_row on
// its own (a group of 32 columns never straddles the halves), so each has its exponent dword and its codes, stored as
// the forward stores them.  A wave takes kRowsInFlight such instructions' segments and issues all their loads,
// 3 * kRowsInFlight 16-byte non-temporal loads a lane, before the first is used: two instructions are 6 loads (24 VGPRs)
// against the forward's 8 and keep its 8 waves a SIMD (FP6: 6); three are 9 loads at 78 / 88 / 74 VGPRs and 6 / 5 / 6
// waves, four 12 loads at 5 / 4 / 5 waves -- no more bytes in flight a SIMD, and fewer waves to hide the arithmetic.
constexpr int kRowsInFlight = 2;
constexpr int kWaveSegments = 4 * kRowsInFlight;
constexpr int kRowsKernelWaves = 4;

template <int kFormat>
__global__ void __launch_bounds__(64 * kRowsKernelWaves)
swiglu_backward_cast_rows_kernel(const uint8_t* __restrict__ h, int64_t h_stride, const uint8_t* __restrict__ dact,
                                 int64_t dact_stride, int64_t num_rows, int inter,
                                 const int32_t* __restrict__ expert_ends, int num_experts, int expert_alignment,
                                 uint8_t* __restrict__ q, uint32_t* __restrict__ sf, uint8_t* __restrict__ dh,
                                 int col_blocks) {
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
    int64_t rows[kRowsInFlight];
    uint32_t cbs[kRowsInFlight];
    u32x4 gate[kRowsInFlight], up[kRowsInFlight], da[kRowsInFlight];
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) {
        rows[k] = row;
        cbs[k] = cb;
        gate[k] = up[k] = da[k] = u32x4{0u, 0u, 0u, 0u};   // (a segment past the live rows still runs the quad steps)
        if (row < live) {
            const u32x4* p = reinterpret_cast<const u32x4*>(h + row * h_stride + cb * (kTile * 2)) + cl;
            gate[k] = __builtin_nontemporal_load(p);       // read once
            up[k] = __builtin_nontemporal_load(p + inter / 8);
            da[k] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4*>(dact + row * dact_stride + cb * (kTile * 2)) + cl);
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
        u32x4 d[2];                                        // dgate, dup
        swiglu_backward8(gate[k], up[k], da[k], d[0], d[1]);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            u32x2 piece;
            uint32_t w;
            cast_row<kFormat>(d[half], lane, piece, w);
            if (rows[k] < live) {
                // dh's row is 2 * col_blocks segments; the half's is (half ? col_blocks : 0) + cb of them
                const int64_t seg = rows[k] * (2 * col_blocks) + half * col_blocks + cbs[k];
                if (dh != nullptr) reinterpret_cast<u32x4*>(dh)[seg * 16 + cl] = d[half];
                uint8_t* dst = q + seg * (4 * kBlockBytes<kFormat>) + piece_off<kFormat>(cl);
                if constexpr (kFormat == DEEPEP_MX_FP4) *reinterpret_cast<uint32_t*>(dst) = piece[0];
                else if (piece_stored<kFormat>(cl)) *reinterpret_cast<u32x2*>(dst) = piece;
                if (cl == 0) sf[seg] = w;
            }
        }
    }
}

// ---------------------------------------------------------------- the row-wise and the transposed pair: training
// One wave (a workgroup of its own) per run of up to kWaveTiles tiles of 128 tokens x 128 columns of inter, the tiles
// consecutive along the token axis, as swiglu_cast_t_kernel; but a tile of the inputs is two tiles of dh, dgate at
// columns c0 and dup at columns inter + c0, and the tile's raw[32] (128 VGPRs) holds one of them.  The wave makes them
// back to back: the gate pass loads g, u and dact of the tile and casts dgate, the up pass loads g and dact again --
// dup = da g s needs no u -- and casts dup.  The second pass asks for 64 KiB that the same wave read a tile's cast
// ago, so it is served from the L2 or the Infinity Cache where they still hold it and HBM sees h and dact once; the
// gate pass therefore loads g and dact with the default policy and only u, and everything in the up pass,
// non-temporal.  Holding both halves would need the second in LDS (32 KiB a wave: three waves a CU).
//
// The load stage.  As in the forward, lane = 16 g + cl holds columns [8 cl, 8 cl + 8) of the 32 tokens n0 + 32 g + i
// of the tile's group g, and the inputs stream through two buffers of a few tokens each: the loads of chunk c + 1 are
// issued, then chunk c goes through swiglu_backward8 into raw[].  The gate pass has three streams of kGateChunkRows = 2
// tokens (2 * 3 * 2 vectors: 48 VGPRs, 12 loads in flight while the wave waits), the up pass two of kUpChunkRows = 4
// (64 VGPRs, 16 loads, the forward's); the buffers are dead when the tile's conversions start.
//
// After the load the tile is the casts', restated as in swiglu_cast_t_kernel, over dh's 2 * inter columns; the
// exponent dwords of both halves' runs wait in LDS (sf_run, 4 KiB) for the 16-byte store of sf_t at the run's end,
// where the forward keeps its one run in 8 VGPRs: two runs' 16 beside raw[] would not fit the FP6 instance.
constexpr int kGateChunkRows = 2, kUpChunkRows = 4;

template <int kFormat>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
swiglu_backward_cast_t_kernel(const uint8_t* __restrict__ h, int64_t h_stride, const uint8_t* __restrict__ dact,
                              int64_t dact_stride, int64_t num_rows, int inter,
                              const int32_t* __restrict__ expert_ends, int num_experts, int expert_alignment,
                              uint8_t* __restrict__ q_t, uint8_t* __restrict__ sf_t, uint8_t* __restrict__ q,
                              uint32_t* __restrict__ sf, uint8_t* __restrict__ dh, int col_blocks, int64_t num_items,
                              int sf16) {
    constexpr int kColBytes = 4 * kBlockBytes<kFormat>;    // a column's bytes of one tile, and a row's
    // FP8: [column][8 slots of 16 bytes], slot ^ ((column >> 3) & 7); FP4 / FP6: fp46_cast_t.hip's image
    __shared__ __attribute__((aligned(16))) uint8_t image_bytes[kTile * kColBytes];
    // [half][tile of the run][column]: byte g the exponent byte of the tile's group g
    __shared__ __attribute__((aligned(16))) uint32_t sf_run[2][kWaveTiles][kTile];
    const int64_t item = tile_item();
    if (item >= num_items) return;
    const int cb = static_cast<int>(item % col_blocks);
    const int64_t n_base = item / col_blocks * (kTile * kWaveTiles);
    const int64_t left = (live_rows(num_rows, expert_ends, num_experts, expert_alignment) - n_base) / kTile;
    if (left <= 0) return;                                 // the whole run is past the live rows
    const int ntile = left < kWaveTiles ? static_cast<int>(left) : kWaveTiles;
#pragma clang loop unroll(disable)
    for (int pass = 0; pass < 2 * ntile; ++pass) {
        const int t = pass >> 1, half = pass & 1;          // the tile of the run; 0: dgate, 1: dup
        // (the lane through an empty asm: what a pass derives from it -- offsets, LDS places -- is then made in the
        // pass, where it is used, and not kept in registers around the loop beside raw[])
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const int g = lane >> 4, cl = lane & 15;
        const int64_t n0 = n_base + t * kTile;
        const int c0 = (half * col_blocks + cb) * kTile;   // the tile's first column of dh
        u32x4 raw[32];
        {
            const uint32_t hs = static_cast<uint32_t>(h_stride), ds = static_cast<uint32_t>(dact_stride);
            const uint8_t* tile = h + n0 * h_stride + cb * (kTile * 2);
            const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(tile), 0, (kTile - 1) * hs + kTile * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(tile + static_cast<int64_t>(inter) * 2), 0, (kTile - 1) * hs + kTile * 2,
                0x00020000);
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(dact + n0 * dact_stride + cb * (kTile * 2)), 0, (kTile - 1) * ds + kTile * 2,
                0x00020000);
            const uint32_t h_off = 32u * g * hs + 16u * cl, d_off = 32u * g * ds + 16u * cl;
            if (half == 0) {
                constexpr int kRows = kGateChunkRows;
                u32x4 gate[2][kRows], up[2][kRows], da[2][kRows];
#pragma unroll
                for (int i = 0; i < kRows; ++i) {
                    gate[0][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, h_off, i * hs, 0);     // read again below
                    up[0][i] = __builtin_amdgcn_raw_buffer_load_b128(ru, h_off, i * hs, 2);       // nt: read once
                    da[0][i] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, i * ds, 0);
                }
#pragma unroll
                for (int c = 0; c < 32 / kRows; ++c) {
                    if (c + 1 < 32 / kRows) {
#pragma unroll
                        for (int i = 0; i < kRows; ++i) {
                            const uint32_t row = (c + 1) * kRows + i;
                            gate[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, h_off, row * hs, 0);
                            up[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(ru, h_off, row * hs, 2);
                            da[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, row * ds, 0);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < kRows; ++i)
                        raw[c * kRows + i] = swiglu_backward8_gate(gate[c & 1][i], up[c & 1][i], da[c & 1][i]);
                    __builtin_amdgcn_sched_barrier(0);     // a chunk at a time: the next one's loads stay in front
                }
            } else {
                constexpr int kRows = kUpChunkRows;
                u32x4 gate[2][kRows], da[2][kRows];
#pragma unroll
                for (int i = 0; i < kRows; ++i) {
                    gate[0][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, h_off, i * hs, 2);     // nt: the last read
                    da[0][i] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, i * ds, 2);
                }
#pragma unroll
                for (int c = 0; c < 32 / kRows; ++c) {
                    if (c + 1 < 32 / kRows) {
#pragma unroll
                        for (int i = 0; i < kRows; ++i) {
                            const uint32_t row = (c + 1) * kRows + i;
                            gate[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(rg, h_off, row * hs, 2);
                            da[(c + 1) & 1][i] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, row * ds, 2);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < kRows; ++i)
                        raw[c * kRows + i] = swiglu_backward8_up(gate[c & 1][i], da[c & 1][i]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // the transposed half: per column, the amax of the lane's 32 tokens, the scale rule, the codes
        u16x2 m[4];
        token_amax(raw, m);
        uint8_t* sf_bytes = reinterpret_cast<uint8_t*>(sf_run[half][t]);
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
        // the row-wise half and dh (stores as loads: a descriptor over what the tile may write, a scalar offset per
        // row and the lane's 32-bit offset; the launcher bounds inter so that the extents fit)
        {
            const uint32_t i32 = static_cast<uint32_t>(inter);
            const uint32_t q_pitch = i32 / 16 * kBlockBytes<kFormat>, sf_pitch = i32 / 16, dh_pitch = i32 * 4;
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
                q + n0 * q_pitch + c0 / kTile * kColBytes, 0, (kTile - 1) * q_pitch + kColBytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsf = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<uint8_t*>(sf) + n0 * sf_pitch + c0 / kTile * 4, 0, (kTile - 1) * sf_pitch + 4,
                0x00020000);
            // (dh == nullptr: a descriptor of no bytes, never used)
            const __amdgpu_buffer_rsrc_t rdh = __builtin_amdgcn_make_buffer_rsrc(
                dh + (dh != nullptr ? n0 * dh_pitch + c0 * 2 : 0), 0,
                dh != nullptr ? (kTile - 1) * dh_pitch + kTile * 2 : 0u, 0x00020000);
            const uint32_t q_off = 32u * g * q_pitch + piece_off<kFormat>(cl), sf_off = 32u * g * sf_pitch;
            const uint32_t dh_off = 32u * g * dh_pitch + 16u * cl;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                // (the row's dwords through an empty asm: the compiler then works on them here, for this row alone)
                u32x4 row = raw[i];
                asm volatile("" : "+v"(row));
                if (dh != nullptr) __builtin_amdgcn_raw_buffer_store_b128(row, rdh, dh_off, i * dh_pitch, 0);
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
        __syncthreads();                                // the image is free for the next tile
    }
    const int lane = threadIdx.x;
    // the run's exponent dwords (lane l: columns 2l and 2l + 1 of each half; a tile past ntile is never stored)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        u32x4 acc[2];
#pragma unroll
        for (int k = 0; k < kWaveTiles; ++k) {
            const u32x2 s = reinterpret_cast<const u32x2*>(sf_run[half][k])[lane];
            acc[0][k] = s[0];
            acc[1][k] = s[1];
        }
        store_sf(acc, sf_t, num_rows, (half * col_blocks + cb) * kTile, n_base, ntile, sf16, lane);
    }
}

// ---------------------------------------------------------------- the checks and the launches, over the element type
struct Args {
    const uint8_t *h, *dact;
    int64_t h_stride, dact_stride;
    int num_rows, inter;
    const int32_t* expert_ends;
    int num_experts, expert_alignment;
    uint8_t *q, *sf, *q_t, *sf_t, *dh;
    hipStream_t stream;
};

template <int kFormat>
int swiglu_backward_cast(const char* what, const Args& a) {
    const int col_blocks = a.inter / kTile;
    if (a.q_t == nullptr) {
        const int64_t segments = static_cast<int64_t>(a.num_rows) * col_blocks;
        constexpr int kGroupSegments = kWaveSegments * kRowsKernelWaves;
        const int64_t grid = (segments + kGroupSegments - 1) / kGroupSegments;
        if (grid > 0x7fffffff) return invalid(what, "too many segments for one launch");
        hipLaunchKernelGGL(swiglu_backward_cast_rows_kernel<kFormat>, dim3(static_cast<unsigned>(grid)),
                           dim3(64 * kRowsKernelWaves), 0, a.stream, a.h, a.h_stride, a.dact, a.dact_stride,
                           static_cast<int64_t>(a.num_rows), a.inter, a.expert_ends, a.num_experts, a.expert_alignment,
                           a.q, reinterpret_cast<uint32_t*>(a.sf), a.dh, col_blocks);
        return launch_status(what);
    }
    const int64_t runs = (static_cast<int64_t>(a.num_rows) + kTile * kWaveTiles - 1) / (kTile * kWaveTiles);
    const int64_t num_items = runs * col_blocks;
    const int64_t grid = (num_items + 7) / 8 * 8;
    if (grid > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const int sf16 = a.num_rows % (kTile * kWaveTiles) == 0 && a16(a.sf_t);
    hipLaunchKernelGGL(swiglu_backward_cast_t_kernel<kFormat>, dim3(static_cast<unsigned>(grid)), dim3(64), 0, a.stream,
                       a.h, a.h_stride, a.dact, a.dact_stride, static_cast<int64_t>(a.num_rows), a.inter,
                       a.expert_ends, a.num_experts, a.expert_alignment, a.q_t, a.sf_t, a.q,
                       reinterpret_cast<uint32_t*>(a.sf), a.dh, col_blocks, num_items, sf16);
    return launch_status(what);
}

}  // namespace

extern "C" {

int deepep_swiglu_backward_cast_mx(int format, const void* h, int64_t h_row_stride_bytes, const void* dact,
                                   int64_t dact_row_stride_bytes, void* q, uint8_t* sf, void* q_t, uint8_t* sf_t,
                                   void* dh, const int32_t* expert_ends, int num_experts, int expert_alignment,
                                   int num_rows, int inter, deepep_stream_t stream) {
    const char* what = "swiglu_backward_cast_mx";
    if (num_rows == 0) return DEEPEP_OK;
    if (format != DEEPEP_MX_FP8 && format != DEEPEP_MX_FP6 && format != DEEPEP_MX_FP4)
        return invalid(what, "format is DEEPEP_MX_FP8, DEEPEP_MX_FP6 or DEEPEP_MX_FP4");
    if (inter < kTile || inter % kTile != 0) return invalid(what, "inter must be a positive multiple of 128");
    if ((q_t == nullptr) != (sf_t == nullptr))
        return invalid(what, "the transposed pair is both q_t and sf_t, or neither");
    if (num_rows < 0 || (q_t != nullptr && num_rows % kTile != 0))
        return invalid(what, "num_rows must not be negative, and a multiple of 128 with the transposed pair (four "
                             "groups of 32 tokens to a scale-factor dword)");
    if (h == nullptr || dact == nullptr || q == nullptr || sf == nullptr || !a16(h) || !a16(dact) || !a16(q) ||
        (reinterpret_cast<uintptr_t>(sf) & 3u) != 0 || !a16(dh))
        return invalid(what, "null or misaligned pointers (16-byte aligned rows, 4-byte aligned scale factors)");
    if (q_t != nullptr && (!a16(q_t) || (reinterpret_cast<uintptr_t>(sf_t) & 3u) != 0))
        return invalid(what, "misaligned transposed outputs (16-byte aligned rows, 4-byte aligned scale factors)");
    if (h_row_stride_bytes < static_cast<int64_t>(inter) * 4 || h_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride of h below 2 * inter * 2 bytes or not 16-byte aligned");
    if (dact_row_stride_bytes < static_cast<int64_t>(inter) * 2 || dact_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride of dact below inter * 2 bytes or not 16-byte aligned");
    // the tile addresses h, dact, q, sf, dh and q_t through 32-bit offsets from the tile's own base (the bases are
    // 64-bit); dh's rows are 4 * inter bytes
    if (h_row_stride_bytes > (1 << 24) || dact_row_stride_bytes > (1 << 24) || inter > (1 << 23) ||
        num_rows >= (1 << 29))
        return invalid(what, "a row stride above 2^24, inter above 2^23, or 2^29 rows or more");
    if (expert_ends != nullptr &&
        (num_experts < 1 || expert_alignment < 1 || (q_t != nullptr && expert_alignment % kTile != 0)))
        return invalid(what, "expert_ends needs num_experts >= 1 and a positive expert_alignment, a multiple of 128 "
                             "with the transposed pair");
    const Args a{static_cast<const uint8_t*>(h), static_cast<const uint8_t*>(dact), h_row_stride_bytes,
                 dact_row_stride_bytes, num_rows, inter, expert_ends, num_experts, expert_alignment,
                 static_cast<uint8_t*>(q), sf, static_cast<uint8_t*>(q_t), sf_t, static_cast<uint8_t*>(dh),
                 reinterpret_cast<hipStream_t>(stream)};
    if (format == DEEPEP_MX_FP8) return swiglu_backward_cast<DEEPEP_MX_FP8>(what, a);
    if (format == DEEPEP_MX_FP6) return swiglu_backward_cast<DEEPEP_MX_FP6>(what, a);
    return swiglu_backward_cast<DEEPEP_MX_FP4>(what, a);
}

}  // extern "C"
