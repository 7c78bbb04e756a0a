// fp46_cast_t.hip -- the transposed MXFP4 and MXFP6 casts on MI355X (deepep_cast_fp4_mx_transposed,
// deepep_cast_fp6_mx_transposed): the groups of 32 that share a UE8M0 exponent byte run along the TOKEN axis and the
// codes are stored K-contiguous, [hidden][num_rows / 2] (e2m1) or [hidden][3 * num_rows / 4] (e2m3) -- the FP4 / FP6
// operand of a block-scaled MFMA (v_mfma_scale_f32_*_f8f6f4: one E8M0 scale per 32 elements along K) that contracts
// over tokens, the experts' weight gradient dW_e = dY_e^T . X_e.  The result is, bit for bit, the pair of
// deepep_cast_fp4_mx / deepep_cast_fp6_mx for the transposed matrix; the same launch can also write that entry's pair
// for x itself (the row-wise pair) from the same read.  There is no counterpart in the reference.
//
// One kernel over the element type, the tiling of cast_fp8_mx_t_kernel (fp8_cast_t.hip).  The scale rules, the
// conversions and the row-wise group's cast are the definitions of fp4_cast_common.h and fp6_cast_common.h, shared with
// fp4_cast.hip and fp6_cast.hip; the amax steps and the exponent bytes are cast_common.h's.
#include "fp4_cast_common.h"
#include "fp6_cast_common.h"

namespace {

constexpr int kTile = 128;                                // tokens and columns of a tile
constexpr int kWaveTiles = 4;                             // tiles per wave: 512 tokens = 16 bytes of sf_t per column

enum class Mx { kFp4, kFp6 };

// Per element type: the bytes of one (column, block of 32 tokens) and the unit the LDS image is written in.
template <Mx kFmt> struct MxFormat;
template <> struct MxFormat<Mx::kFp4> {
    static constexpr int kBlockBytes = 16;                // 32 codes of 4 bits: one 16-byte unit
    using unit = u32x4;
};
template <> struct MxFormat<Mx::kFp6> {
    static constexpr int kBlockBytes = kGroupBytes;       // 32 codes of 6 bits: three 8-byte units
    using unit = u32x2;
};

// tokens (n, n + 1) of one column as the two bf16 of a dword, the lower token in the lower half -- the order both
// conversions take their sources in: a, b are the dwords of the two tokens that hold the column.  One v_perm_b32 (its
// selector bytes 0-3 name the bytes of the second operand, 4-7 those of the first): (a & 0xffff) | b << 16, or
// a >> 16 | (b & 0xffff0000) for the dword's high column.
__device__ __forceinline__ uint32_t pair_tokens(uint32_t a, uint32_t b, bool high) {
    return __builtin_amdgcn_perm(b, a, high ? 0x07060302u : 0x05040100u);
}

// One wave (a workgroup of its own) per run of up to kWaveTiles tiles of 128 tokens x 128 columns, the tiles
// consecutive along the token axis.
//
// Loads, as cast_fp8_mx_t_kernel: lane = 16 * g + cl holds columns [8 cl, 8 cl + 8) of the 32 tokens of the tile's
// group g (32 16-byte non-temporal loads in flight, each instruction four whole 256-byte row segments), so the
// token-axis amax is in-lane, on packed 16-bit magnitudes.
//
// Transposition: both conversions take their sources as pairs of bf16 in a dword, so the lane pairs tokens
// (2j, 2j + 1) of ONE column (pair_tokens) and the transposition inside the lane costs only that.  FP4: cvt8_fp4 over
// four pairs gives the dword of 8 tokens, four of them the block's 16 bytes.  FP6: the 16 pairs are one source of
// cvt32_fp6, which gives the block's 24 bytes.  What moves between lanes is codes, never bf16.
//
// The LDS image (8 KiB / 12 KiB) holds, per column, the 64 / 96 bytes of the tile's four blocks; the columns stand in
// the order p = 16 c + cl of column 8 cl + c, so that the lanes of one write instruction (one c) are 64 / 96 bytes
// apart and not 512 / 768.  FP4: a 16-byte slot 4 p + g, its low two bits XORed with (p >> 2) & 3: the 16 lanes of a
// write pass (one g) then hit 16 different slots mod 16.  FP6: 8-byte units 12 p + 3 g + j, unswizzled: 12 cl mod 32
// takes 8 values and the two groups of a pass are 3 units apart, so a 32-lane pass of 8-byte writes is 2-way
// conflicted (cl and cl + 8).  The image is read back linearly, lane l of instruction k the 16 bytes at 16 (64 k + l)
// (FP4: through the same XOR): no conflict, and 4 / 6 consecutive lanes hold the 64 / 96 contiguous bytes a tile adds
// to one row of q_t, which they store 16 bytes a lane.  No byte is ever stored to memory.
//
// Scale factors and the schedule of the work items: as cast_fp8_mx_t_kernel (a dword per column and tile, 16 bytes
// per column when sf16).
//
// The row-wise pair (kRowwise): the lane's 8 columns of a row are a quarter of a group of 32 columns, so each row is
// cast by cast_group_fp4<1> / cast_group_fp6<1> (the quad steps of group_max).  FP4: the lane's dword, 16 lanes a
// row's 64 bytes.  FP6: the lane's 8 codes are 48 bits; the quad's four pieces are the group's 24 bytes, which its
// first three lanes store 8 bytes each after one quad DPP read of the next lane's piece.  The first lane of 16 stores
// the dword of the tile's four column groups.
//
// Every tile lies inside the matrix (num_rows % 128 == 0, hidden % 128 == 0): no lane is ever out of range, and a
// block's output depends on its own 32 rows only.
template <Mx kFmt, bool kRowwise>
__global__ void __launch_bounds__(64)
cast_mx_t_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int64_t num_rows, int hidden,
                 uint8_t* __restrict__ q_t, uint8_t* __restrict__ sf_t, uint8_t* __restrict__ q,
                 uint32_t* __restrict__ sf, int col_blocks, int64_t num_items, int sf16) {
    using F = MxFormat<kFmt>;
    using Unit = typename F::unit;
    constexpr int kBlockBytes = F::kBlockBytes;
    constexpr int kColBytes = 4 * kBlockBytes;             // a column's bytes of one tile
    __shared__ __attribute__((aligned(16))) Unit image[kTile * kColBytes / sizeof(Unit)];
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
    const int64_t qt_pitch = num_rows / 32 * kBlockBytes;  // bytes per row of q_t
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
        // the transposed half: per column, the amax of the lane's 32 tokens, the scale rule, the codes
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
            const float amax = amax_floor(m[c >> 1][c & 1]);
            const int p = 16 * c + cl;                     // the image's place of column 8 cl + c
            uint32_t byte;
            if constexpr (kFmt == Mx::kFp4) {
                byte = fp4_exp_byte(amax);
                const float factor = deepep::ue8m0_factor(byte);
                u32x4 d;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    u32x4 pr;                              // tokens 8k .. 8k + 7 of column c
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        pr[j] = pair_tokens(raw[8 * k + 2 * j][c >> 1], raw[8 * k + 2 * j + 1][c >> 1], c & 1);
                    d[k] = cvt8_fp4(pr, factor);
                    __builtin_amdgcn_sched_barrier(0);     // 8 tokens' temporaries at a time beside raw[]
                }
                image[(4 * p + g) ^ ((cl >> 2) & 3)] = d;
            } else {
                byte = fp6_exp_byte(amax);
                const float factor = deepep::ue8m0_factor(byte);
                u32x16 v;                                  // the 32 tokens of column c
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = pair_tokens(raw[2 * j][c >> 1], raw[2 * j + 1][c >> 1], c & 1);
                const u32x6 d = cvt32_fp6(v, factor);
#pragma unroll
                for (int j = 0; j < 3; ++j) image[12 * p + 3 * g + j] = u32x2{d[2 * j], d[2 * j + 1]};
                __builtin_amdgcn_sched_barrier(0);         // one column's temporaries at a time beside raw[]
            }
            sf_bytes[(8 * cl + c) * 4 + g] = static_cast<uint8_t>(byte);
        }
        // (stores as loads: a descriptor over what the tile may write, a scalar offset per row and the lane's 32-bit
        // offset, so that no address pair per store lives across the tile loop; the launcher bounds hidden so that
        // the extents fit, and the descriptor's range check drops anything outside them)
        if constexpr (kRowwise) {
            const uint32_t h32 = static_cast<uint32_t>(hidden);
            const uint32_t q_pitch = h32 / 32 * kBlockBytes, sf_pitch = h32 / 32;    // bytes per row of q and of sf
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
                q + n0 * q_pitch + cb * (4 * kBlockBytes), 0, (kTile - 1) * q_pitch + 4 * kBlockBytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsf = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<uint8_t*>(sf) + n0 * sf_pitch + cb * 4, 0, (kTile - 1) * sf_pitch + 4, 0x00020000);
            const uint32_t sf_off = 32u * g * sf_pitch;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                // (the row's dwords through an empty asm: the compiler then works on them here, for this row alone)
                u32x4 row = raw[i];
                asm volatile("" : "+v"(row));
                uint32_t w;
                if constexpr (kFmt == Mx::kFp4) {
                    const Fp4Lane<1> r = cast_group_fp4<1>(&row);
                    w = ue8m0_or4<4>(r.byte, lane);
                    __builtin_amdgcn_raw_buffer_store_b32(r.q[0], rq, 32u * g * q_pitch + 4u * cl, i * q_pitch, 0);
                } else {
                    const Fp6Lane r = cast_group_fp6<1>(&row);
                    w = ue8m0_or4<4>(r.byte, lane);
                    // the lane's 48 bits: lo and the low half of hi; the next lane of the quad's (quad permute
                    // [1, 2, 3, 3]); piece j of the group's three 8-byte pieces from lanes j and j + 1
                    constexpr int kDppQuadNext = 0xF9;
                    const uint32_t lo = r.q[0], hi = r.q[1];
                    const uint32_t nlo = static_cast<uint32_t>(
                        __builtin_amdgcn_mov_dpp(static_cast<int>(lo), kDppQuadNext, 0xf, 0xf, true));
                    const uint32_t nhi = static_cast<uint32_t>(
                        __builtin_amdgcn_mov_dpp(static_cast<int>(hi), kDppQuadNext, 0xf, 0xf, true));
                    const int j = cl & 3;
                    const uint32_t mix = hi | (nlo << 16);               // own bytes 4-5, the next lane's 0-1
                    const u32x2 piece = j == 0 ? u32x2{lo, mix}
                                      : j == 1 ? u32x2{(lo >> 16) | (hi << 16), nlo}
                                               : u32x2{mix, (nlo >> 16) | (nhi << 16)};
                    if (j < 3)
                        __builtin_amdgcn_raw_buffer_store_b64(
                            piece, rq, 32u * g * q_pitch + kBlockBytes * (cl >> 2) + 8u * j, i * q_pitch, 0);
                }
                if (cl == 0) __builtin_amdgcn_raw_buffer_store_b32(w, rsf, sf_off, i * sf_pitch, 0);
                __builtin_amdgcn_sched_barrier(0);         // one row's temporaries at a time beside raw[]
            }
        }
        __syncthreads();
        // the tile's share of q_t: row c0 + column, bytes [n0 / 32 * kBlockBytes, + kColBytes) (64-bit addresses:
        // nothing else is live here)
        uint8_t* qt_tile = q_t + c0 * qt_pitch + n0 / 32 * kBlockBytes;
#pragma unroll
        for (int k = 0; k < kColBytes / 16 * 2; ++k) {
            const int i = 64 * k + lane;                   // the image's 16 bytes at 16 i: place p, 16-byte piece
            int p, piece;
            u32x4 v;
            if constexpr (kFmt == Mx::kFp4) {
                p = i >> 2;
                piece = i & 3;
                v = image[i ^ ((lane >> 4) & 3)];          // (p >> 2) & 3 == (lane >> 4) & 3
            } else {
                p = i / 6;
                piece = i - 6 * p;
                const u32x2 a = image[2 * i], b = image[2 * i + 1];
                v = u32x4{a[0], a[1], b[0], b[1]};
            }
            const int col = 8 * (p & 15) + (p >> 4);
            *reinterpret_cast<u32x4*>(qt_tile + col * qt_pitch + 16 * piece) = v;
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

// the checks and the launch of deepep_cast_fp8_mx_transposed, over the element type
template <Mx kFmt>
int cast_mx_t(const char* what, const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
              uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream) {
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
    // the kernel addresses a tile of x, q and sf through 32-bit offsets from the tile's own base (the bases are 64-bit)
    if (x_row_stride_bytes > (1 << 24) || hidden > (1 << 24) || num_rows >= (1 << 29))
        return invalid(what, "row stride or hidden above 2^24, or 2^29 rows or more");
    const int col_blocks = hidden / kTile;
    const int64_t runs = (static_cast<int64_t>(num_rows) + kTile * kWaveTiles - 1) / (kTile * kWaveTiles);
    const int64_t num_items = runs * col_blocks;
    const int64_t grid = (num_items + 7) / 8 * 8;
    if (grid > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    const int sf16 = num_rows % (kTile * kWaveTiles) == 0 && a16(sf_t);
    const auto kernel = q != nullptr ? cast_mx_t_kernel<kFmt, true> : cast_mx_t_kernel<kFmt, false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(x), x_row_stride_bytes, static_cast<int64_t>(num_rows), hidden,
                       static_cast<uint8_t*>(q_t), sf_t, static_cast<uint8_t*>(q), reinterpret_cast<uint32_t*>(sf),
                       col_blocks, num_items, sf16);
    return launch_status(what);
}

}  // namespace

extern "C" {

int deepep_cast_fp4_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream) {
    return cast_mx_t<Mx::kFp4>("cast_fp4_mx_transposed", x, x_row_stride_bytes, q_t, sf_t, q, sf, num_rows, hidden,
                               stream);
}

int deepep_cast_fp6_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream) {
    return cast_mx_t<Mx::kFp6>("cast_fp6_mx_transposed", x, x_row_stride_bytes, q_t, sf_t, q, sf, num_rows, hidden,
                               stream);
}

}  // extern "C"
