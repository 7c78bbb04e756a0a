// grouped_gemm_mx.hip -- the experts' GEMMs over the block-scaled MFMA of MI355X (deepep_grouped_gemm_mx): the
// consumer of every MX pair this library produces.  Both operands are (codes, exponent bytes) pairs with the
// contraction axis contiguous and one UE8M0 byte per 32 elements along it -- what the row-wise casts, the casting
// dispatch, the transposed casts and the requantisation return -- in FP8 (e4m3fn), FP6 (e2m3) or FP4 (e2m1), the two
// formats independent.  There is no counterpart in the reference, which leaves the experts to the caller.
//
// One kernel, two schedules.  A workgroup of 4 waves owns a 128 x 128 tile of the output, described by the first row
// of each operand, the contraction range [k_begin, k_end) and the number of valid rows:
//   fprop  out[n, :] = A[n, :] . B[e(n)]^T   the tile's expert is found from expert_ends (staged in LDS); the
//                                            contraction is the whole row; rows past the expert's end are zeros
//   wgrad  dW[e] = dY_t[:, seg_e] . X_t[:, seg_e]^T   the contraction is the expert's token segment
// expert_alignment % 128 == 0, so a tile never holds rows of two experts.
//
// The instruction: v_mfma_scale_f32_16x16x128_f8f6f4, D[16 x 16] += P[16 x 128] . Q[16 x 128]^T.  Measured on the
// MI355X with one-hot operands: lane l = 16 kb + r holds 32 elements of row r of each operand,
//   FP8  registers 0-3 the 16 bytes of elements [16 kb, 16 kb + 16), registers 4-7 those of [64 + 16 kb, 64 + 16 kb + 16)
//        -- the instruction is two 16 x 16 x 64 halves -- each in memory order;
//   FP6  registers 0-5 the 24 bytes of elements [32 kb, 32 kb + 32), element c in bits 6c + 5 : 6c;
//   FP4  registers 0-3 the 16 bytes of elements [32 kb, 32 kb + 32), element c in nibble c;
// and byte `opsel` of the lane's scale register is the exponent byte of elements [32 kb, 32 kb + 32) of row r, whatever
// the format (for FP8 these are not the lane's own elements).  The result: lane l holds D[4 kb + i][r] in register i.
// The library's formats are these to the bit, so an operand is loaded from global memory straight into the
// instruction's registers: no LDS, no shuffle.
//
// The first operand here is the B tile and the second the A tile, so a lane ends up with four CONSECUTIVE output
// columns of one output row (16 bytes of fp32, 8 of bf16 a store).  A wave owns 64 x 64 of the tile: 4 x 4
// accumulators of 4 floats, and per step of 128 along the contraction 4 + 4 operand fragments (the next step's are in
// flight while this step's 16 MFMAs run: two register sets) and 4 + 4 exponent bytes, one byte load each.
#include "grouped_gemm_mx_common.h"

namespace {

constexpr int kTile = 128;                                 // rows and columns of a workgroup's tile
constexpr int kStep = 128;                                 // elements along the contraction per MFMA

struct Problem {
    Operand a, b;
    const int32_t* __restrict__ expert_ends;
    int num_experts, expert_alignment;
    void* out;
    int64_t num_tokens;
    int dim0, dim1;                                        // fprop: K, O; wgrad: O, H
    int wgrad;
};

// one step's registers of a wave: the fragments and exponent bytes of its 4 row blocks of A and 4 of B
struct Step {
    i32x8 a[4], b[4];
    int sa[4], sb[4];
};

template <int kFmtA, int kFmtB>
__device__ __forceinline__ void load_step(Step& s, const uint8_t* a_tile, const uint8_t* a_sf_tile,
                                          const uint8_t* b_tile, const uint8_t* b_sf_tile,
                                          const uint32_t* a_off, const uint32_t* a_sf_off, const uint32_t* b_off,
                                          const uint32_t* b_sf_off, int64_t k32) {
    const uint8_t* ap = a_tile + k32 * block_bytes(kFmtA);
    const uint8_t* bp = b_tile + k32 * block_bytes(kFmtB);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.a[i] = load_codes<kFmtA>(ap + a_off[i]);
        s.b[i] = load_codes<kFmtB>(bp + b_off[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.sa[i] = a_sf_tile[k32 + a_sf_off[i]];
        s.sb[i] = b_sf_tile[k32 + b_sf_off[i]];
    }
}

template <int kFmtA, int kFmtB>
__device__ __forceinline__ void mfma_step(const Step& s, f32x4 (*acc)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(s.b[j], s.a[i], acc[i][j], kFmtB, kFmtA, 0,
                                                                          s.sb[j], 0, s.sa[i]);
    }
}

__device__ __forceinline__ int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

template <int kFmtA, int kFmtB, bool kF32>
__global__ void __launch_bounds__(256)
grouped_gemm_mx_kernel(Problem p) {
    __shared__ int32_t s_ends[kMaxExperts];
    __shared__ int32_t s_expert;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kb = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;               // the wave's 64 x 64 quarter of the tile

    // ------------------------------------------------------------ the tile
    int64_t a_row0, b_row0, k_begin, k_end, out_stride;
    int valid_rows;
    uint8_t* out_tile;
    if (!p.wgrad) {
        const int col_blocks = p.dim1 / kTile;
        const int64_t row0 = static_cast<int64_t>(blockIdx.x / col_blocks) * kTile;
        const int col0 = blockIdx.x % col_blocks * kTile;
        for (int e = tid; e < p.num_experts; e += 256) s_ends[e] = p.expert_ends[e];
        if (tid == 0) s_expert = -1;
        __syncthreads();
        for (int e = tid; e < p.num_experts; e += 256) {
            const int64_t lo = e ? align_up(s_ends[e - 1], p.expert_alignment) : 0;
            if (lo <= row0 && row0 < align_up(s_ends[e], p.expert_alignment)) s_expert = e;
        }
        __syncthreads();
        const int e = s_expert;
        if (e < 0) return;                                 // past the last expert's rows: nothing is loaded or written
        const int64_t left = s_ends[e] - row0;
        valid_rows = left < 0 ? 0 : left > kTile ? kTile : static_cast<int>(left);
        a_row0 = row0;
        b_row0 = static_cast<int64_t>(e) * p.dim1 + col0;
        k_begin = 0;
        k_end = valid_rows ? p.dim0 : 0;
        out_stride = p.dim1;
        out_tile = static_cast<uint8_t*>(p.out) + (row0 * out_stride + col0) * (kF32 ? 4 : 2);
    } else {
        const int hb = p.dim1 / kTile, ob = p.dim0 / kTile;
        const int e = blockIdx.x / (hb * ob);
        a_row0 = static_cast<int64_t>(blockIdx.x / hb % ob) * kTile;
        b_row0 = static_cast<int64_t>(blockIdx.x % hb) * kTile;
        // the expert's tokens [start, align_up(end, 128)), kept inside the operands whatever expert_ends holds
        const int64_t start = e ? align_up(p.expert_ends[e - 1], p.expert_alignment) : 0;
        const int64_t end = align_up(p.expert_ends[e], kStep);
        k_begin = start < 0 ? 0 : start / kStep * kStep;
        k_end = end > p.num_tokens ? p.num_tokens : end;
        valid_rows = kTile;
        out_stride = p.dim1;
        out_tile = static_cast<uint8_t*>(p.out) +
                   ((static_cast<int64_t>(e) * p.dim0 + a_row0) * out_stride + b_row0) * 4;
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    // ------------------------------------------------------------ the contraction
    // (a wave whose 64 rows are all padding has nothing to add)
    if (k_begin < k_end && 64 * wm < valid_rows) {
        const uint8_t* a_tile = p.a.q + a_row0 * p.a.q_stride;
        const uint8_t* b_tile = p.b.q + b_row0 * p.b.q_stride;
        const uint8_t* a_sf_tile = p.a.sf + a_row0 * p.a.sf_stride;
        const uint8_t* b_sf_tile = p.b.sf + b_row0 * p.b.sf_stride;
        // the lane's 32-bit offsets inside the tile (the launcher bounds the strides)
        uint32_t a_off[4], a_sf_off[4], b_off[4], b_sf_off[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t ar = 64 * wm + 16 * i + r, br = 64 * wn + 16 * i + r;
            a_off[i] = ar * static_cast<uint32_t>(p.a.q_stride) + lane_bytes(kFmtA, kb);
            b_off[i] = br * static_cast<uint32_t>(p.b.q_stride) + lane_bytes(kFmtB, kb);
            a_sf_off[i] = ar * static_cast<uint32_t>(p.a.sf_stride) + kb;
            b_sf_off[i] = br * static_cast<uint32_t>(p.b.sf_stride) + kb;
        }
        const int64_t k32_end = k_end / 32;
        int64_t k32 = k_begin / 32;
        Step s0, s1;
        load_step<kFmtA, kFmtB>(s0, a_tile, a_sf_tile, b_tile, b_sf_tile, a_off, a_sf_off, b_off, b_sf_off,
                                k32);
        while (true) {
            if (k32 + 4 < k32_end)
                load_step<kFmtA, kFmtB>(s1, a_tile, a_sf_tile, b_tile, b_sf_tile, a_off, a_sf_off, b_off,
                                        b_sf_off, k32 + 4);
            mfma_step<kFmtA, kFmtB>(s0, acc);
            k32 += 4;
            if (k32 >= k32_end) break;
            if (k32 + 4 < k32_end)
                load_step<kFmtA, kFmtB>(s0, a_tile, a_sf_tile, b_tile, b_sf_tile, a_off, a_sf_off, b_off,
                                        b_sf_off, k32 + 4);
            mfma_step<kFmtA, kFmtB>(s1, acc);
            k32 += 4;
            if (k32 >= k32_end) break;
        }
    }

    // ------------------------------------------------------------ the tile's rows: zeros past the valid ones
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 64 * wm + 16 * i + r;
        const bool live = row < valid_rows;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 64 * wn + 16 * j + 4 * kb;
            const f32x4 v = live ? acc[i][j] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            store4<kF32>(out_tile + (row * out_stride + col) * (kF32 ? 4 : 2), v);
        }
    }
}

}  // namespace

extern "C" int deepep_grouped_gemm_mx(int schedule, int a_format, int b_format, const void* a,
                                      int64_t a_row_stride_bytes, const uint8_t* a_sf, int64_t a_sf_row_stride,
                                      const void* b, int64_t b_row_stride_bytes, const uint8_t* b_sf,
                                      int64_t b_sf_row_stride, const int32_t* expert_ends, int num_experts,
                                      int expert_alignment, void* out, int out_fp32, int64_t num_tokens, int dim0,
                                      int dim1, deepep_stream_t stream) {
    const char* what = "grouped_gemm_mx";
    const bool wgrad = schedule == DEEPEP_GEMM_WGRAD;
    if (schedule != DEEPEP_GEMM_FPROP && !wgrad)
        return invalid(what, "schedule is DEEPEP_GEMM_FPROP or DEEPEP_GEMM_WGRAD");
    if (!is_format(a_format) || !is_format(b_format))
        return invalid(what, "a format is DEEPEP_MX_FP8, DEEPEP_MX_FP6 or DEEPEP_MX_FP4");
    if (num_tokens < 0 || num_tokens % kTile != 0 || num_tokens >= (int64_t(1) << 31))
        return invalid(what, "num_tokens must be a multiple of 128 below 2^31");
    if (dim0 < kTile || dim0 % kTile != 0 || dim1 < kTile || dim1 % kTile != 0 || dim0 > (1 << 24) || dim1 > (1 << 24))
        return invalid(what, "dim0 and dim1 must be positive multiples of 128, at most 2^24");
    if (num_experts < 1 || num_experts > kMaxExperts) return invalid(what, "num_experts must be in [1, 1024]");
    if (expert_alignment < kTile || expert_alignment % kTile != 0)
        return invalid(what, "expert_alignment must be a positive multiple of 128");
    if (out_fp32 != 0 && out_fp32 != 1) return invalid(what, "out_fp32 is 0 or 1");
    if (wgrad && !out_fp32) return invalid(what, "the wgrad schedule writes float");
    if (out == nullptr || !a16(out) || expert_ends == nullptr || (reinterpret_cast<uintptr_t>(expert_ends) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned out, 4-byte aligned expert_ends)");
    if (num_tokens == 0 && !wgrad) return DEEPEP_OK;
    const int64_t k = wgrad ? num_tokens : dim0;
    if (num_tokens != 0) {
        if (const char* msg = operand_fault(a, a_row_stride_bytes, a_sf, a_sf_row_stride, a_format, k))
            return invalid(what, msg);
        if (const char* msg = operand_fault(b, b_row_stride_bytes, b_sf, b_sf_row_stride, b_format, k))
            return invalid(what, msg);
    }
    const int64_t tiles = wgrad ? static_cast<int64_t>(num_experts) * (dim0 / kTile) * (dim1 / kTile)
                                : num_tokens / kTile * (dim1 / kTile);
    if (tiles > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const Problem p{{static_cast<const uint8_t*>(a), a_sf, a_row_stride_bytes, a_sf_row_stride},
                    {static_cast<const uint8_t*>(b), b_sf, b_row_stride_bytes, b_sf_row_stride},
                    expert_ends, num_experts, expert_alignment, out, num_tokens, dim0, dim1, wgrad};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = static_cast<unsigned>(tiles);
    for_formats(a_format, b_format, out_fp32, [&](auto fa, auto fb, auto f32) {
        hipLaunchKernelGGL((grouped_gemm_mx_kernel<decltype(fa)::value, decltype(fb)::value, decltype(f32)::value>),
                           dim3(grid), dim3(256), 0, s, p);
    });
    return launch_status(what);
}
