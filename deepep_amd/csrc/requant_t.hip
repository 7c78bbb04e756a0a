// requant_t.hip -- a row-wise quantised pair requantised along the TOKEN axis on MI355X
// (deepep_requant_fp8_mx_transposed, deepep_requant_fp4_mx_transposed, deepep_requant_fp6_mx_transposed): what a
// casting dispatch returns -- e4m3fn / e2m1 / e2m3 rows with their scale factors along hidden -- becomes the operand of
// the experts' weight gradient dW_e = dY_e^T . X_e, codes stored K-contiguous [hidden][num_rows ...] with one UE8M0
// exponent byte per 32 TOKENS, in one read of the pair and without the bf16 [num_rows][hidden] buffer between.  The
// result is, bit for bit, the transposed cast (fp8_cast_t.hip, fp46_cast_t.hip) of the cast back (fp8_cast.hip,
// fp4_cast.hip, fp6_cast.hip) of the pair.  There is no counterpart in the reference.
//
// Nothing here is new arithmetic.  The load stage dequantises with the cast backs' own definitions (fp8_dequant.h,
// fp4_dequant.h, fp6_dequant.h: exact code -> fp32, one fp32 multiply by the group's factor, one round to nearest even
// to bf16 -- the rounding is part of the contract) into the packed bf16 dwords a bf16 load would have given; from
// there the tile is that of cast_fp8_mx_t_kernel / cast_mx_t_kernel without the row-wise pair, restated here (those
// two files stay as they are, to the instruction), over the definitions of fp8_cast_common.h, fp4_cast_common.h and
// fp6_cast_common.h.  Their comments give the reasons for the shapes below.
#include "fp4_cast_common.h"
#include "fp4_dequant.h"
#include "fp6_cast_common.h"
#include "fp6_dequant.h"
#include "fp8_cast_common.h"

namespace {

constexpr int kTile = 128;                                // tokens and columns of a tile
constexpr int kWaveTiles = 4;                             // tiles per wave: 512 tokens = 16 bytes of sf_t per column

// ---------------------------------------------------------------- the load stages
// As in the transposed casts, lane = 16 * g + cl holds columns [8 cl, 8 cl + 8) of the 32 tokens n0 + 32 g + i of the
// tile's group g.  A load stage is  load(n0, cb, g, cl, raw): it leaves in raw[i] the 8 bf16 of the lane's columns of
// token i as one 16-byte vector (column 2j in the low half of dword j), exactly the cast back's bf16.
//
// Codes: one load per token through the tile's buffer descriptor (a scalar row offset and the lane's 32-bit offset;
// the launcher bounds the row stride so that the tile's extent fits), all 32 in flight, non-temporal.
// Factors: one per token and lane, read in place through the tensor's own strides (in bytes here).  The lane's 8
// columns lie in one group of 32 and in one group of 128, so a lane needs one factor a token: the exponent byte of
// column group 4 cb + (cl >> 2) (per-32 forms), byte cb & 3 of element cb >> 2 (packed UE8M0) or the float of
// column group cb (fp32).  16 lanes (4 with per-32 factors) read the same address.

// where the lane's factor of the tile's first token of group g stands
template <Sf kSf>
__device__ __forceinline__ const uint8_t* sf_of(const uint8_t* sf, int64_t row_bytes, int64_t col_bytes, int64_t n0,
                                                int cb, int g, int cl) {
    const uint8_t* p = sf + (n0 + 32 * g) * row_bytes;
    if constexpr (kSf == Sf::kExp32) return p + (4 * cb + (cl >> 2)) * col_bytes;
    else if constexpr (kSf == Sf::kExp128) return p + (cb >> 2) * col_bytes + (cb & 3);
    else return p + cb * col_bytes;
}

template <Sf kSf>
__device__ __forceinline__ float load_factor(const uint8_t* p) {
    if constexpr (kSf == Sf::kFp32) return *reinterpret_cast<const float*>(p);
    else return deepep::ue8m0_factor(*p);                  // byte 0: +0.0f
}

struct CodeRows {
    const uint8_t* __restrict__ q;
    int64_t q_stride;
    const uint8_t* __restrict__ sf;
    int64_t sf_row_bytes, sf_col_bytes;
};

// e4m3fn: 8 bytes a token, 16 lanes a row's 128 bytes (a whole line)
template <Sf kSf>
struct LoadFp8 : CodeRows {
    __device__ __forceinline__ void operator()(int64_t n0, int cb, int g, int cl, u32x4* raw) const {
        const uint32_t stride32 = static_cast<uint32_t>(q_stride);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(q + n0 * q_stride + cb * kTile), 0, (kTile - 1) * stride32 + kTile, 0x00020000);
        const uint32_t lane_off = 32u * g * stride32 + 8u * cl;
        u32x2 code[32];
#pragma unroll
        for (int i = 0; i < 32; ++i)
            code[i] = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, i * stride32, 2);     // nt: read once
        const uint8_t* sfp = sf_of<kSf>(sf, sf_row_bytes, sf_col_bytes, n0, cb, g, cl);
        float s[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) s[i] = load_factor<kSf>(sfp + i * sf_row_bytes);
#pragma unroll
        for (int i = 0; i < 32; ++i) raw[i] = deepep::dequant8(code[i][0], code[i][1], s[i]);
    }
};

// e2m1: 4 bytes a token, 16 lanes a row's 64 bytes
struct LoadFp4 : CodeRows {
    __device__ __forceinline__ void operator()(int64_t n0, int cb, int g, int cl, u32x4* raw) const {
        const uint32_t stride32 = static_cast<uint32_t>(q_stride);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(q + n0 * q_stride + cb * (kTile / 2)), 0, (kTile - 1) * stride32 + kTile / 2,
            0x00020000);
        const uint32_t lane_off = 32u * g * stride32 + 4u * cl;
        uint32_t code[32];
#pragma unroll
        for (int i = 0; i < 32; ++i)
            code[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, lane_off, i * stride32, 2);     // nt: read once
        const uint8_t* sfp = sf_of<Sf::kExp32>(sf, sf_row_bytes, sf_col_bytes, n0, cb, g, cl);
        float s[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) s[i] = load_factor<Sf::kExp32>(sfp + i * sf_row_bytes);
#pragma unroll
        for (int i = 0; i < 32; ++i) raw[i] = deepep::dequant8_fp4(code[i], s[i]);
    }
};

// e2m3: 6 bytes a token, bits [48 j, 48 j + 48) of the 24-byte group of the lane's quad, j = cl & 3.  The quad's 24
// bytes are dword-aligned, a lane's 6 are not: the lane loads the 8 bytes at 0 / 4 / 12 / 16 of the group, which hold
// its 6 from byte 0 (j even) or byte 2 (j odd) on, and shifts.  The 8 codes go through the group's conversion as the
// low 48 bits of a group whose other codes are zero (dequant32_fp6: v_cvt_scalef32_pk32_f32_fp6 converts a whole
// group); its first vector is the lane's 8 bf16.
struct LoadFp6 : CodeRows {
    __device__ __forceinline__ void operator()(int64_t n0, int cb, int g, int cl, u32x4* raw) const {
        constexpr int kTileBytes = 4 * kGroupBytes;        // a row's bytes of one tile
        const uint32_t stride32 = static_cast<uint32_t>(q_stride);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(q + n0 * q_stride + cb * kTileBytes), 0, (kTile - 1) * stride32 + kTileBytes,
            0x00020000);
        const int j = cl & 3;
        const uint32_t lane_off = 32u * g * stride32 + kGroupBytes * (cl >> 2) + 4u * j + (j >= 2 ? 4u : 0u);
        u32x2 code[32];
#pragma unroll
        for (int i = 0; i < 32; ++i)
            code[i] = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_off, i * stride32, 2);     // nt: read once
        const uint8_t* sfp = sf_of<Sf::kExp32>(sf, sf_row_bytes, sf_col_bytes, n0, cb, g, cl);
        float s[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) s[i] = load_factor<Sf::kExp32>(sfp + i * sf_row_bytes);
        const bool odd = j & 1;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t lo = odd ? (code[i][0] >> 16) | (code[i][1] << 16) : code[i][0];
            const uint32_t hi = odd ? code[i][1] >> 16 : code[i][1] & 0xffffu;
            u32x4 out[4];
            deepep::dequant32_fp6(u32x6{lo, hi, 0u, 0u, 0u, 0u}, s[i], out);
            raw[i] = out[0];
        }
    }
};

// ---------------------------------------------------------------- the tile, after the load
// the work item of a workgroup: workgroups w = x (mod 8) share an XCD (observed, for speed only) and take consecutive
// items, column blocks fastest
__device__ __forceinline__ int64_t tile_item() {
    const int64_t per_xcd = gridDim.x / 8;
    return (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
}

// the packed 16-bit magnitudes' maximum over the lane's 32 tokens, per pair of columns
__device__ __forceinline__ void token_amax(const u32x4* raw, u16x2* m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = u16x2{0, 0};
#pragma unroll
    for (int i = 0; i < 32; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[j] = __builtin_elementwise_max(m[j], __builtin_bit_cast(u16x2, raw[i][j] & 0x7fff7fffu));
    }
}

// the tile's exponent dwords (lane l: columns 2l and 2l + 1) into the run's
__device__ __forceinline__ void keep_sf(u32x4* acc, const uint32_t* sf_image, int t, int lane) {
    const u32x2 s = reinterpret_cast<const u32x2*>(sf_image)[lane];
#pragma unroll
    for (int k = 0; k < kWaveTiles; ++k) {
        acc[0][k] = t == k ? s[0] : acc[0][k];
        acc[1][k] = t == k ? s[1] : acc[1][k];
    }
}

// a column's exponent dwords of the run: one 16-byte store per column (sf16: num_rows % 512 == 0 and a 16-byte aligned
// sf_t) or dwords (the tail)
__device__ __forceinline__ void store_sf(const u32x4* acc, uint8_t* __restrict__ sf_t, int64_t num_rows, int c0,
                                         int64_t n_base, int ntile, int sf16, int lane) {
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

// One wave (a workgroup of its own) per run of up to kWaveTiles tiles of 128 tokens x 128 columns, the tiles
// consecutive along the token axis: cast_fp8_mx_t_kernel<false> behind the load stage kLoad.  Every tile lies inside
// the matrix (num_rows % 128 == 0, hidden % 128 == 0), and a block's output depends on its own 32 rows only.
template <typename Load>
__global__ void __launch_bounds__(64)
requant_fp8_mx_t_kernel(Load load, int64_t num_rows, uint8_t* __restrict__ q_t, uint8_t* __restrict__ sf_t,
                        int col_blocks, int64_t num_items, int sf16) {
    __shared__ u32x4 image[kTile * kTile / 16];            // [column][8 slots of 16 bytes], slot ^ ((column >> 3) & 7)
    // [column]: byte g the exponent byte of the tile's group g
    __shared__ __attribute__((aligned(16))) uint32_t sf_image[kTile];
    const int lane = threadIdx.x, g = lane >> 4, cl = lane & 15;
    const int64_t item = tile_item();
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
        u32x4 raw[32];
        load(n0, cb, g, cl, raw);
        // per column, the amax of the lane's 32 tokens, the scale rule, the bytes
        u16x2 m[4];
        token_amax(raw, m);
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
        __syncthreads();
        // (a descriptor over what the tile may write and the lane's 32-bit offset; the launcher bounds num_rows so
        // that the extents fit, and the descriptor's range check drops anything outside them)
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
        keep_sf(acc, sf_image, t, lane);
        __syncthreads();                                   // the image is free for the next tile
    }
    store_sf(acc, sf_t, num_rows, c0, n_base, ntile, sf16, lane);
}

enum class Mx { kFp4, kFp6 };

// Per element type: the bytes of one (column, block of 32 tokens), the unit the LDS image is written in, a row's
// bytes of 32 columns and the load stage.
template <Mx kFmt> struct MxFormat;
template <> struct MxFormat<Mx::kFp4> {
    static constexpr int kBlockBytes = 16;                // 32 codes of 4 bits: one 16-byte unit
    using unit = u32x4;
    using load = LoadFp4;
};
template <> struct MxFormat<Mx::kFp6> {
    static constexpr int kBlockBytes = kGroupBytes;       // 32 codes of 6 bits: three 8-byte units
    using unit = u32x2;
    using load = LoadFp6;
};

// tokens (n, n + 1) of one column as the two bf16 of a dword, the lower token in the lower half (one v_perm_b32, as
// in fp46_cast_t.hip): a, b are the dwords of the two tokens that hold the column
__device__ __forceinline__ uint32_t pair_tokens(uint32_t a, uint32_t b, bool high) {
    return __builtin_amdgcn_perm(b, a, high ? 0x07060302u : 0x05040100u);
}

// cast_mx_t_kernel<kFmt, false> behind the element type's load stage.
template <Mx kFmt>
__global__ void __launch_bounds__(64)
requant_mx_t_kernel(typename MxFormat<kFmt>::load load, int64_t num_rows, uint8_t* __restrict__ q_t,
                    uint8_t* __restrict__ sf_t, int col_blocks, int64_t num_items, int sf16) {
    using F = MxFormat<kFmt>;
    using Unit = typename F::unit;
    constexpr int kBlockBytes = F::kBlockBytes;
    constexpr int kColBytes = 4 * kBlockBytes;             // a column's bytes of one tile
    __shared__ __attribute__((aligned(16))) Unit image[kTile * kColBytes / sizeof(Unit)];
    // [column]: byte g the exponent byte of the tile's group g
    __shared__ __attribute__((aligned(16))) uint32_t sf_image[kTile];
    const int lane = threadIdx.x, g = lane >> 4, cl = lane & 15;
    const int64_t item = tile_item();
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
        u32x4 raw[32];
        load(n0, cb, g, cl, raw);
        // per column, the amax of the lane's 32 tokens, the scale rule, the codes
        u16x2 m[4];
        token_amax(raw, m);
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
        keep_sf(acc, sf_image, t, lane);
        __syncthreads();                                   // the image is free for the next tile
    }
    store_sf(acc, sf_t, num_rows, c0, n_base, ntile, sf16, lane);
}

// ---------------------------------------------------------------- the checks and the launch, over the element type
// row_bytes: the code bytes of a row of `hidden` columns; sf_elem: the bytes of a scale-factor element (its alignment)
struct Launch {
    int col_blocks;
    int64_t num_items;
    unsigned grid;
    int sf16;
};

int requant_checks(const char* what, const void* q, int64_t q_row_stride_bytes, int64_t row_bytes, const void* sf,
                   int sf_elem, int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t, int num_rows,
                   int hidden, Launch& l) {
    if (hidden < kTile || hidden % kTile != 0) return invalid(what, "hidden must be a positive multiple of 128");
    if (num_rows < 0 || num_rows % kTile != 0)
        return invalid(what, "num_rows must be a multiple of 128 (four groups of 32 tokens to a scale-factor dword)");
    if (q == nullptr || sf == nullptr || q_t == nullptr || sf_t == nullptr || !a16(q) || !a16(q_t) ||
        reinterpret_cast<uintptr_t>(sf) % sf_elem != 0 || (reinterpret_cast<uintptr_t>(sf_t) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows, 4-byte aligned sf_t, aligned sf)");
    if (q_row_stride_bytes < row_bytes || q_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below a row's bytes or not 16-byte aligned");
    if (sf_row_stride < 0 || sf_col_stride < 0) return invalid(what, "negative scale-factor stride");
    // the kernel addresses a tile of q and of q_t through 32-bit offsets from the tile's own base (the bases are 64-bit)
    if (q_row_stride_bytes > (1 << 24) || hidden > (1 << 24) || num_rows >= (1 << 29))
        return invalid(what, "row stride or hidden above 2^24, or 2^29 rows or more");
    l.col_blocks = hidden / kTile;
    const int64_t runs = (static_cast<int64_t>(num_rows) + kTile * kWaveTiles - 1) / (kTile * kWaveTiles);
    l.num_items = runs * l.col_blocks;
    const int64_t grid = (l.num_items + 7) / 8 * 8;
    if (grid > 0x7fffffff) return invalid(what, "too many tiles for one launch");
    l.grid = static_cast<unsigned>(grid);
    l.sf16 = num_rows % (kTile * kWaveTiles) == 0 && a16(sf_t);
    return DEEPEP_OK;
}

template <typename Kernel, typename Load>
int requant_launch(const char* what, Kernel kernel, const Load& load, const Launch& l, int num_rows, void* q_t,
                   uint8_t* sf_t, deepep_stream_t stream) {
    hipLaunchKernelGGL(kernel, dim3(l.grid), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), load,
                       static_cast<int64_t>(num_rows), static_cast<uint8_t*>(q_t), sf_t, l.col_blocks, l.num_items,
                       l.sf16);
    return launch_status(what);
}

template <Mx kFmt>
int requant_mx_t(const char* what, int64_t row_bytes, const void* q, int64_t q_row_stride_bytes, const uint8_t* sf,
                 int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t, int num_rows, int hidden,
                 deepep_stream_t stream) {
    if (num_rows == 0) return DEEPEP_OK;
    Launch l;
    if (const int rc = requant_checks(what, q, q_row_stride_bytes, row_bytes, sf, 1, sf_row_stride, sf_col_stride,
                                      q_t, sf_t, num_rows, hidden, l))
        return rc;
    typename MxFormat<kFmt>::load load{{static_cast<const uint8_t*>(q), q_row_stride_bytes, sf, sf_row_stride,
                                        sf_col_stride}};
    return requant_launch(what, requant_mx_t_kernel<kFmt>, load, l, num_rows, q_t, sf_t, stream);
}

}  // namespace

extern "C" {

int deepep_requant_fp8_mx_transposed(const void* q, int64_t q_row_stride_bytes, const void* sf, int64_t sf_row_stride,
                                     int64_t sf_col_stride, int sf_form, void* q_t, uint8_t* sf_t, int num_rows,
                                     int hidden, deepep_stream_t stream) {
    const char* what = "requant_fp8_mx_transposed";
    if (num_rows == 0) return DEEPEP_OK;
    if (sf_form != DEEPEP_SF_FORM_FP32 && sf_form != DEEPEP_SF_FORM_UE8M0_PACKED && sf_form != DEEPEP_SF_FORM_MX)
        return invalid(what, "sf_form is DEEPEP_SF_FORM_FP32, DEEPEP_SF_FORM_UE8M0_PACKED or DEEPEP_SF_FORM_MX");
    if (sf_form == DEEPEP_SF_FORM_UE8M0_PACKED && hidden % 512 != 0)
        return invalid(what, "packed UE8M0 scale factors need hidden % 512 == 0");
    const int elem = sf_form == DEEPEP_SF_FORM_MX ? 1 : 4;                // the strides count elements
    Launch l;
    if (const int rc = requant_checks(what, q, q_row_stride_bytes, hidden, sf, elem, sf_row_stride, sf_col_stride, q_t,
                                      sf_t, num_rows, hidden, l))
        return rc;
    const CodeRows rows{static_cast<const uint8_t*>(q), q_row_stride_bytes, static_cast<const uint8_t*>(sf),
                        sf_row_stride * elem, sf_col_stride * elem};
    if (sf_form == DEEPEP_SF_FORM_FP32)
        return requant_launch(what, requant_fp8_mx_t_kernel<LoadFp8<Sf::kFp32>>, LoadFp8<Sf::kFp32>{rows}, l, num_rows,
                              q_t, sf_t, stream);
    if (sf_form == DEEPEP_SF_FORM_UE8M0_PACKED)
        return requant_launch(what, requant_fp8_mx_t_kernel<LoadFp8<Sf::kExp128>>, LoadFp8<Sf::kExp128>{rows}, l,
                              num_rows, q_t, sf_t, stream);
    return requant_launch(what, requant_fp8_mx_t_kernel<LoadFp8<Sf::kExp32>>, LoadFp8<Sf::kExp32>{rows}, l, num_rows,
                          q_t, sf_t, stream);
}

int deepep_requant_fp4_mx_transposed(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf,
                                     int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t,
                                     int num_rows, int hidden, deepep_stream_t stream) {
    return requant_mx_t<Mx::kFp4>("requant_fp4_mx_transposed", static_cast<int64_t>(hidden) / 2, q, q_row_stride_bytes,
                                  sf, sf_row_stride, sf_col_stride, q_t, sf_t, num_rows, hidden, stream);
}

int deepep_requant_fp6_mx_transposed(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf,
                                     int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t,
                                     int num_rows, int hidden, deepep_stream_t stream) {
    return requant_mx_t<Mx::kFp6>("requant_fp6_mx_transposed", static_cast<int64_t>(hidden) / 4 * 3, q,
                                  q_row_stride_bytes, sf, sf_row_stride, sf_col_stride, q_t, sf_t, num_rows, hidden,
                                  stream);
}

}  // extern "C"
