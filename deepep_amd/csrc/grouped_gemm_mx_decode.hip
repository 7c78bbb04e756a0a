// grouped_gemm_mx_decode.hip -- the experts' GEMM at 16-row granularity (deepep_grouped_gemm_mx_decode): the fprop
// contract of grouped_gemm_mx.hip for a decoding step, where an expert has 1 to 64 tokens and the time goes into
// streaming its weights from HBM once.  Same operands (MX pairs, contraction axis contiguous, one UE8M0 byte per 32
// elements, FP8 / FP6 / FP4 independently), same instruction (v_mfma_scale_f32_16x16x128_f8f6f4, layouts in
// grouped_gemm_mx.hip and DESIGN.md section 3), another split of the work:
//
//   tile     a workgroup of 4 waves owns 16 rows x 64 columns of the output; expert_alignment % 16 == 0, so a tile
//            never holds rows of two experts.  The grid is (N / 16) * (O / 64) with the ROW tile fastest: the row tiles
//            of one expert, which need the same 64 weight rows, are neighbours in launch order.
//   split-K  wave w contracts a contiguous range of the K / 128 steps (ranges differ by at most one step; with fewer
//            steps than waves some waves have none).  A wave therefore streams whole cache lines of its 64 weight
//            rows in every format.  Per step: one A fragment, four B fragments, five exponent bytes, 4 MFMAs into
//            4 accumulators of 4 floats.
//   ring     the fragments of kDepth steps are in flight per wave, in a register ring that is unrolled (no dynamic
//            index); the steady-state loop has no branch between a step's MFMAs and the load that refills its slot.
//   reduce   each wave writes its four 16 x 16 partials to LDS (4 x 4 x 1 KiB); after one barrier wave j adds the four
//            partials of column block j in the order wave 0, 1, 2, 3, masks the rows past the expert's end and stores
//            16 bytes (fp32) or 8 bytes (bf16) a lane.  No atomics: the result is a function of the inputs alone.
//
// The first MFMA operand is the B block and the second the A tile, so lane 16 kb + r ends with columns [4 kb, 4 kb + 4)
// of row r of a 16 x 16 block.  An output row depends on its own A row only, so rows of A past the expert's end may
// hold anything (exponent bytes 0xff included): they are masked at the store.
#include "grouped_gemm_mx_common.h"

namespace {

constexpr int kRows = 16;                                  // rows of a workgroup's tile
constexpr int kCols = 64;                                  // its columns: four 16 x 16 blocks
constexpr int kStep = 128;                                 // elements along the contraction per MFMA
constexpr int kWaves = 4;

// Steps in flight per wave.  A step is 1 + 4 fragments (8 / 6 / 4 registers each) and 5 exponent bytes: 45 registers
// for FP8 x FP8, 25 for FP4 x FP4, and 15 / 20 / 10 loads with B in FP8 / FP6 / FP4.  Two bounds: 256 registers a wave
// (2 waves a SIMD) with the accumulators and addresses, and fewer than 64 loads outstanding (the counter's range).
__host__ __device__ constexpr int ring_depth(int /*fmt_a*/, int fmt_b) { return fmt_b == DEEPEP_MX_FP4 ? 4 : 3; }

struct DecodeProblem {
    Operand a, b;
    const int32_t* __restrict__ expert_ends;
    int num_experts, expert_alignment;
    void* out;
    int row_tiles;                                         // N / 16
    int k, o;
};

// one slot of the ring: a step's fragments and exponent bytes of the tile's A rows and the wave's 4 blocks of B rows
struct Slot {
    i32x8 a, b[4];
    int sa, sb[4];
};

// what a lane adds to the tile's pointers: its row's offsets, 32-bit (the launcher bounds the strides)
struct LaneOffsets {
    uint32_t a, a_sf, b[4], b_sf[4];
};

template <int kFmtA, int kFmtB>
__device__ __forceinline__ void load_slot(Slot& s, const uint8_t* a_tile, const uint8_t* a_sf_tile,
                                          const uint8_t* b_tile, const uint8_t* b_sf_tile, const LaneOffsets& off,
                                          int step) {
    const int64_t k32 = static_cast<int64_t>(step) * (kStep / 32);
    const uint8_t* bp = b_tile + k32 * block_bytes(kFmtB);
#pragma unroll
    for (int j = 0; j < 4; ++j) s.b[j] = load_codes<kFmtB>(bp + off.b[j]);
    s.a = load_codes<kFmtA>(a_tile + k32 * block_bytes(kFmtA) + off.a);
#pragma unroll
    for (int j = 0; j < 4; ++j) s.sb[j] = b_sf_tile[k32 + off.b_sf[j]];
    s.sa = a_sf_tile[k32 + off.a_sf];
}

template <int kFmtA, int kFmtB>
__device__ __forceinline__ void mfma_slot(const Slot& s, f32x4* acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(s.b[j], s.a, acc[j], kFmtB, kFmtA, 0, s.sb[j], 0,
                                                                   s.sa);
}

// an end (below 2^31; a negative one counts as 0) rounded up to the alignment (below 2^31): 32-bit, no overflow
__device__ __forceinline__ uint32_t align_up(int32_t v, int32_t a) {
    const uint32_t u = v < 0 ? 0u : static_cast<uint32_t>(v), ua = static_cast<uint32_t>(a);
    return (u + ua - 1) / ua * ua;
}

template <int kFmtA, int kFmtB, bool kF32>
__global__ void __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2)))
grouped_gemm_mx_decode_kernel(DecodeProblem p) {
    constexpr int kDepth = ring_depth(kFmtA, kFmtB);
    __shared__ int32_t s_ends[kMaxExperts];
    __shared__ int32_t s_expert;
    __shared__ f32x4 s_part[kWaves][4][64];                // [wave][column block][lane]: 16 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: the wave's pointers and loop stay scalar
    const int r = lane & 15, kb = lane >> 4;

    // ------------------------------------------------------------ the tile and its expert
    const int64_t row0 = static_cast<int64_t>(blockIdx.x % p.row_tiles) * kRows;
    const int col0 = blockIdx.x / p.row_tiles * kCols;
    for (int e = tid; e < p.num_experts; e += 64 * kWaves) s_ends[e] = p.expert_ends[e];
    if (tid == 0) s_expert = -1;
    __syncthreads();
    for (int e = tid; e < p.num_experts; e += 64 * kWaves) {
        const uint32_t lo = e ? align_up(s_ends[e - 1], p.expert_alignment) : 0;
        if (lo <= row0 && row0 < align_up(s_ends[e], p.expert_alignment)) s_expert = e;
    }
    __syncthreads();
    const int e = __builtin_amdgcn_readfirstlane(s_expert);
    if (e < 0) return;                                     // past the last expert's rows: nothing is loaded or written
    const int64_t left = __builtin_amdgcn_readfirstlane(s_ends[e]) - row0;
    const int valid_rows = left < 0 ? 0 : left > kRows ? kRows : static_cast<int>(left);
    // wave `wave` stores column block `wave`: the lane's 4 columns of row r
    uint8_t* dst = static_cast<uint8_t*>(p.out) +
                   ((row0 + r) * p.o + col0 + 16 * wave + 4 * kb) * (kF32 ? 4 : 2);
    if (valid_rows == 0) {                                 // alignment padding only: zeros, no operand is loaded
        store4<kF32>(dst, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
        return;
    }

    // ------------------------------------------------------------ the wave's share of the contraction
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int steps = p.k / kStep;
    const int begin = wave * steps / kWaves, n = (wave + 1) * steps / kWaves - begin;
    if (n > 0) {
        const int64_t b_row0 = static_cast<int64_t>(e) * p.o + col0;
        const uint8_t* a_tile = p.a.q + row0 * p.a.q_stride;
        const uint8_t* a_sf_tile = p.a.sf + row0 * p.a.sf_stride;
        const uint8_t* b_tile = p.b.q + b_row0 * p.b.q_stride;
        const uint8_t* b_sf_tile = p.b.sf + b_row0 * p.b.sf_stride;
        LaneOffsets off;
        off.a = r * static_cast<uint32_t>(p.a.q_stride) + lane_bytes(kFmtA, kb);
        off.a_sf = r * static_cast<uint32_t>(p.a.sf_stride) + kb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            off.b[j] = (16 * j + r) * static_cast<uint32_t>(p.b.q_stride) + lane_bytes(kFmtB, kb);
            off.b_sf[j] = (16 * j + r) * static_cast<uint32_t>(p.b.sf_stride) + kb;
        }
        Slot ring[kDepth];
#pragma unroll
        for (int s = 0; s < kDepth; ++s) {
            if (s < n) load_slot<kFmtA, kFmtB>(ring[s], a_tile, a_sf_tile, b_tile, b_sf_tile, off, begin + s);
        }
        int i = 0;
        // full rounds: every slot is consumed and refilled, no branch in between
        for (; i + 2 * kDepth <= n; i += kDepth) {
#pragma unroll
            for (int s = 0; s < kDepth; ++s) {
                mfma_slot<kFmtA, kFmtB>(ring[s], acc);
                load_slot<kFmtA, kFmtB>(ring[s], a_tile, a_sf_tile, b_tile, b_sf_tile, off, begin + i + s + kDepth);
            }
        }
        // the last n - i < 2 kDepth steps
        for (; i < n; i += kDepth) {
#pragma unroll
            for (int s = 0; s < kDepth; ++s) {
                if (i + s < n) {
                    mfma_slot<kFmtA, kFmtB>(ring[s], acc);
                    if (i + s + kDepth < n)
                        load_slot<kFmtA, kFmtB>(ring[s], a_tile, a_sf_tile, b_tile, b_sf_tile, off,
                                                begin + i + s + kDepth);
                }
            }
        }
    }

    // ------------------------------------------------------------ the four partials of a block, in the waves' order
#pragma unroll
    for (int j = 0; j < 4; ++j) s_part[wave][j][lane] = acc[j];
    __syncthreads();
    f32x4 sum = s_part[0][wave][lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        const f32x4 v = s_part[w][wave][lane];
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] = sum[c] + v[c];
    }
    store4<kF32>(dst, r < valid_rows ? sum : f32x4{0.0f, 0.0f, 0.0f, 0.0f});
}

}  // namespace

extern "C" int deepep_grouped_gemm_mx_decode(int a_format, int b_format, const void* a, int64_t a_row_stride_bytes,
                                             const uint8_t* a_sf, int64_t a_sf_row_stride, const void* b,
                                             int64_t b_row_stride_bytes, const uint8_t* b_sf, int64_t b_sf_row_stride,
                                             const int32_t* expert_ends, int num_experts, int expert_alignment,
                                             void* out, int out_fp32, int64_t num_tokens, int k, int o,
                                             deepep_stream_t stream) {
    const char* what = "grouped_gemm_mx_decode";
    if (!is_format(a_format) || !is_format(b_format))
        return invalid(what, "a format is DEEPEP_MX_FP8, DEEPEP_MX_FP6 or DEEPEP_MX_FP4");
    if (num_tokens < 0 || num_tokens % kRows != 0 || num_tokens >= (int64_t(1) << 31))
        return invalid(what, "num_tokens must be a multiple of 16 below 2^31");
    if (k < kStep || k % kStep != 0 || k > (1 << 24))
        return invalid(what, "k must be a positive multiple of 128, at most 2^24");
    if (o < kCols || o % kCols != 0 || o > (1 << 24))
        return invalid(what, "o must be a positive multiple of 64, at most 2^24");
    if (num_experts < 1 || num_experts > kMaxExperts) return invalid(what, "num_experts must be in [1, 1024]");
    if (expert_alignment < kRows || expert_alignment % kRows != 0)
        return invalid(what, "expert_alignment must be a positive multiple of 16");
    if (out_fp32 != 0 && out_fp32 != 1) return invalid(what, "out_fp32 is 0 or 1");
    if (out == nullptr || !a16(out) || expert_ends == nullptr || (reinterpret_cast<uintptr_t>(expert_ends) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned out, 4-byte aligned expert_ends)");
    if (num_tokens == 0) return DEEPEP_OK;
    if (const char* msg = operand_fault(a, a_row_stride_bytes, a_sf, a_sf_row_stride, a_format, k))
        return invalid(what, msg);
    if (const char* msg = operand_fault(b, b_row_stride_bytes, b_sf, b_sf_row_stride, b_format, k))
        return invalid(what, msg);
    const int64_t tiles = num_tokens / kRows * (o / kCols);
    if (tiles > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const DecodeProblem p{{static_cast<const uint8_t*>(a), a_sf, a_row_stride_bytes, a_sf_row_stride},
                          {static_cast<const uint8_t*>(b), b_sf, b_row_stride_bytes, b_sf_row_stride},
                          expert_ends, num_experts, expert_alignment, out, static_cast<int>(num_tokens / kRows), k, o};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = static_cast<unsigned>(tiles);
    for_formats(a_format, b_format, out_fp32, [&](auto fa, auto fb, auto f32) {
        hipLaunchKernelGGL(
            (grouped_gemm_mx_decode_kernel<decltype(fa)::value, decltype(fb)::value, decltype(f32)::value>),
            dim3(grid), dim3(64 * kWaves), 0, s, p);
    });
    return launch_status(what);
}
