// fp8_cast_t.hip -- the transposed MXFP8 cast on MI355X (deepep_cast_fp8_mx_transposed): the groups of 32 that share
// a UE8M0 exponent byte run along the TOKEN axis and the e4m3fn bytes are stored K-contiguous, [hidden][num_rows] --
// the operand of a block-scaled MFMA (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32 elements along K) that
// contracts over tokens, the experts' weight gradient dW_e = dY_e^T . X_e.  The result is, bit for bit, the MXFP8 pair
// of deepep_cast_fp8_mx for the transposed matrix; the same launch can also write that entry's pair for x itself (the
// row-wise pair) from the same read.  There is no counterpart in the reference.
//
// The scale rule, the exponent byte, the e4m3fn conversion and the row-wise group's cast are the definitions of
// cast_common.h and fp8_cast_common.h (SfFormat<Sf::kExp32>), shared with fp8_cast.hip.
#include "fp8_cast_common.h"

namespace {

// One wave (a workgroup of its own) per run of up to kWaveTiles tiles of 128 tokens x 128 columns, the tiles
// consecutive along the token axis.
//
// Loads: lane = 16 * g + cl holds columns [8 cl, 8 cl + 8) of the tile -- one 16-byte load per row -- and walks the 32
// tokens of the tile's group g: a wave load instruction covers four rows' 256-byte segments (whole lines), and the
// lane ends up with all 32 tokens of its 8 columns in registers, so the token-axis amax is in-lane (on packed
// 16-bit magnitudes, as amax8's), with no cross-lane step.
//
// Transposition: v_cvt_pk_fp8_f32 packs any two values, so the lane converts (token, token + 1) pairs of ONE column
// (cvt8 over 8 consecutive tokens): the transposition inside a lane costs nothing, and what moves between lanes is
// e4m3fn bytes, never bf16.  A column's 128 tokens are then 32 bytes in each of the lanes cl, cl + 16, cl + 32, cl + 48;
// they meet in a 16 KiB LDS image [column][128 bytes] whose 16-byte slots are XOR-swizzled by cl (the writes of 8
// consecutive lanes are 8 columns apart = 1 KiB: unswizzled, one bank group), and are read back so that 8 consecutive
// lanes hold one column's 128 bytes: every q_t store instruction writes 8 whole 128-byte lines, 16 bytes a lane.
//
// Scale factors: a column's four exponent bytes of the tile (one per group g) are one dword of sf_t; they meet in LDS
// as bytes and lane l keeps the dwords of columns 2l and 2l + 1 of up to kWaveTiles tiles, which leave as one 16-byte
// store per column (sf16: num_rows % 512 == 0 and a 16-byte aligned sf_t) or as dwords (the tail).  No byte is ever
// stored to memory.
//
// The row-wise pair (kRowwise): the lane's 8 columns of a row are a quarter of a group of 32 columns, so each row is
// cast by cast_group_fp8<1, 32> (the quad steps of group_max) exactly as in cast_fp8_kernel<Sf::kExp32>; 16 lanes
// store a row's 128 bytes (a whole line), the first of them the dword of the tile's four column groups.
//
// Every tile lies inside the matrix (num_rows % 128 == 0, hidden % 128 == 0): no lane is ever out of range, and a
// group's output depends on its own 32 rows only (no value crosses groups: the LDS image moves finished bytes).
// Workgroups w = x (mod 8) share an XCD (observed, for speed only): they take consecutive items, column blocks
// fastest, so the partial lines of the row-wise scale factors (4 bytes per row and column block) meet in one L2.
constexpr int kTile = 128;                                // tokens and columns of a tile
constexpr int kWaveTiles = 4;                             // tiles per wave: 512 tokens = 16 bytes of sf_t per column

template <bool kRowwise>
__global__ void __launch_bounds__(64)
cast_fp8_mx_t_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int64_t num_rows, int hidden,
                     uint8_t* __restrict__ q_t, uint8_t* __restrict__ sf_t, uint8_t* __restrict__ q,
                     uint32_t* __restrict__ sf, int col_blocks, int64_t num_items, int sf16) {
    using Tile = SfTile<Sf::kExp32, 8>;
    __shared__ u32x4 image[kTile * kTile / 16];            // [column][8 slots of 16 bytes], slot ^ ((column >> 3) & 7)
    // [column]: byte g the exponent byte of the tile's group g
    __shared__ __attribute__((aligned(16))) uint32_t sf_image[kTile];
    const int lane = threadIdx.x, g = lane >> 4, cl = lane & 15;
    const int64_t per_xcd = gridDim.x / 8;
    const int64_t item = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (item >= num_items) return;
    const int cb = static_cast<int>(item % col_blocks);
    const int64_t n_base = item / col_blocks * (kTile * kWaveTiles);
    const int c0 = cb * kTile;
    const int64_t left = (num_rows - n_base) / kTile;
    const int ntile = left < kWaveTiles ? static_cast<int>(left) : kWaveTiles;
    u32x4 acc[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
#pragma clang loop unroll(disable)
    for (int t = 0; t < ntile; ++t) {
        const int64_t n0 = n_base + t * kTile;
        // (one descriptor for the tile: a scalar row offset and the lane's 32-bit offset, so that 32 loads are in
        // flight without 32 address pairs; the launcher bounds the row stride so that the tile's extent fits)
        const uint32_t stride32 = static_cast<uint32_t>(x_stride);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(x + n0 * x_stride + c0 * 2), 0, (kTile - 1) * stride32 + kTile * 2, 0x00020000);
        const uint32_t lane_off = 32u * g * stride32 + 16u * cl;
        u32x4 raw[32];
#pragma unroll
        for (int i = 0; i < 32; ++i)
            raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, i * stride32, 2);    // nt: read once
        // the transposed half: per column, the amax of the lane's 32 tokens, the scale rule, the bytes
        u16x2 m[4] = {u16x2{0, 0}, u16x2{0, 0}, u16x2{0, 0}, u16x2{0, 0}};
#pragma unroll
        for (int i = 0; i < 32; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                m[j] = __builtin_elementwise_max(m[j], __builtin_bit_cast(u16x2, raw[i][j] & 0x7fff7fffu));
        }
        uint8_t* sf_bytes = reinterpret_cast<uint8_t*>(sf_image);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            // (a bf16 magnitude orders as its bits, and is the high half of the fp32 of the same value)
            const float amax = fmaxf(1e-4f, __uint_as_float(static_cast<uint32_t>(m[c >> 1][c & 1]) << 16));
            float scale, factor;
            group_scales(amax, 1, scale, factor);
            uint32_t d[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float f[8];                                // tokens 8k .. 8k + 7 of column c
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t w = raw[8 * k + i][c >> 1];
                    f[i] = __uint_as_float((c & 1) ? w & 0xffff0000u : w << 16);
                }
                const u32x2 h = cvt8(f, scale);
                d[2 * k] = h[0];
                d[2 * k + 1] = h[1];
                __builtin_amdgcn_sched_barrier(0);         // 8 tokens' temporaries at a time beside raw[]
            }
            const int col = 8 * cl + c;
            image[col * 8 + ((2 * g) ^ (cl & 7))] = u32x4{d[0], d[1], d[2], d[3]};
            image[col * 8 + ((2 * g + 1) ^ (cl & 7))] = u32x4{d[4], d[5], d[6], d[7]};
            sf_bytes[col * 4 + g] = static_cast<uint8_t>(ue8m0_byte(factor));
        }
        // (stores as loads: a descriptor over what the tile may write, a scalar offset per row or column and the lane's
        // 32-bit offset, so that no address pair per store lives across the tile loop; the launcher bounds hidden and
        // num_rows so that the extents fit, and the descriptor's range check drops anything outside them)
        if constexpr (kRowwise) {
            const uint32_t h32 = static_cast<uint32_t>(hidden), sf_pitch = h32 / 32;    // bytes per row of q and of sf
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
                q + n0 * hidden + c0, 0, (kTile - 1) * h32 + kTile, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsf = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<uint8_t*>(sf) + n0 * sf_pitch + cb * 4, 0, (kTile - 1) * sf_pitch + 4, 0x00020000);
            const uint32_t q_off = 32u * g * h32 + 8u * cl, sf_off = 32u * g * sf_pitch;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                // (the row's dwords through an empty asm: the compiler then unpacks them here, for this row alone,
                // and does not keep the transposed half's 256 unpacked values for this one)
                u32x4 row = raw[i];
                asm volatile("" : "+v"(row));
                const Fp8Lane<1> r = cast_group_fp8<1, 32>(&row, 1);
                const uint32_t w = Tile::word(r.sf, lane);
                __builtin_amdgcn_raw_buffer_store_b64(r.q, rq, q_off, i * h32, 0);
                if (Tile::owns(lane)) __builtin_amdgcn_raw_buffer_store_b32(w, rsf, sf_off, i * sf_pitch, 0);
                __builtin_amdgcn_sched_barrier(0);         // one row's temporaries at a time beside raw[]
            }
        }
        __syncthreads();
        const uint32_t n32 = static_cast<uint32_t>(num_rows);
        const uint32_t qt_off = (lane >> 3) * n32 + 16u * (lane & 7);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int col = (lane >> 3) + 8 * k;           // (col >> 3) & 7 == k & 7
            const u32x4 v = image[col * 8 + ((lane & 7) ^ (k & 7))];
            const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
                q_t + (c0 + 8 * k) * num_rows + n0, 0, 7 * n32 + kTile, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(v, rk, qt_off, 0, 0);
        }
        const u32x2 s = reinterpret_cast<const u32x2*>(sf_image)[lane];
#pragma unroll
        for (int k = 0; k < kWaveTiles; ++k) {
            acc[0][k] = t == k ? s[0] : acc[0][k];
            acc[1][k] = t == k ? s[1] : acc[1][k];
        }
        __syncthreads();                                   // the image is free for the next tile
    }
    const int64_t sf_t_pitch = num_rows / 32;              // bytes per row of sf_t (a multiple of 4)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        uint8_t* dst = sf_t + (c0 + 2 * lane + p) * sf_t_pitch + n_base / 32;
        if (sf16 && ntile == kWaveTiles) {
            *reinterpret_cast<u32x4*>(dst) = acc[p];
        } else {
#pragma unroll
            for (int k = 0; k < kWaveTiles; ++k)
                if (k < ntile) reinterpret_cast<uint32_t*>(dst)[k] = acc[p][k];
        }
    }
}

}  // namespace

extern "C" {

int deepep_cast_fp8_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream) {
    const char* what = "cast_fp8_mx_transposed";
    if (num_rows == 0) return DEEPEP_OK;
    if (hidden < kTile || hidden % kTile != 0) return invalid(what, "hidden must be a positive multiple of 128");
    if (num_rows < 0 || num_rows % kTile != 0)
        return invalid(what, "num_rows must be a multiple of 128 (four groups of 32 tokens to a scale-factor dword)");
    if (x == nullptr || q_t == nullptr || sf_t == nullptr || !a16(x) || !a16(q_t) ||
        (reinterpret_cast<uintptr_t>(sf_t) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows, 4-byte aligned scale factors)");
    if ((q == nullptr) != (sf == nullptr))
        return invalid(what, "the row-wise pair is both q and sf, or neither");
    if (q != nullptr && (!a16(q) || (reinterpret_cast<uintptr_t>(sf) & 3u) != 0))
        return invalid(what, "misaligned row-wise outputs (16-byte aligned rows, 4-byte aligned scale factors)");
    if (x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden * 2 bytes or not 16-byte aligned");
    // the kernel addresses a tile through 32-bit offsets from the tile's own base (the bases are 64-bit)
    if (x_row_stride_bytes > (1 << 24) || hidden > (1 << 24) || num_rows >= (1 << 29))
        return invalid(what, "row stride or hidden above 2^24, or 2^29 rows or more");
    const int col_blocks = hidden / kTile;
    const int64_t runs = (static_cast<int64_t>(num_rows) + kTile * kWaveTiles - 1) / (kTile * kWaveTiles);
    const int64_t num_items = runs * col_blocks;
    const int64_t grid = (num_items + 7) / 8 * 8;
    if (grid > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const int sf16 = num_rows % (kTile * kWaveTiles) == 0 && a16(sf_t);
    const auto kernel = q != nullptr ? cast_fp8_mx_t_kernel<true> : cast_fp8_mx_t_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, static_cast<int64_t>(num_rows), hidden,
                       static_cast<uint8_t*>(q_t), sf_t, static_cast<uint8_t*>(q), reinterpret_cast<uint32_t*>(sf),
                       col_blocks, num_items, sf16);
    return launch_status(what);
}

}  // extern "C"
