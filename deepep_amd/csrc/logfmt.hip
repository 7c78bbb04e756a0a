// logfmt.hip -- the LogFMT-10 codec kernels (the format and its arithmetic: logfmt_codec.h):
//   deepep_cast_logfmt        bf16 rows -> planes [low | high] and meta        (reference: internode_ll.cu:557-638)
//   deepep_cast_back_logfmt   planes and meta -> bf16 rows                      (reference: internode_ll.cu:672-712)
//   deepep_logfmt_pack_rows   packed bf16 exchange rows [bf16 | weight tail] -> wire rows
//                             [low | high | meta, padded to a 128-byte line | weight tail]
// One wave per row, a lane takes 8 columns (one 16-byte load of bf16, one 8-byte store into the low plane, one 2-byte
// store into the high plane); the 16 lanes of a 128-column group find its amax and amin with a four-step butterfly on
// the magnitude bits.  Plain and vector stores with the default cache policy: the exchange and the combine read the
// rows right back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/deepep_amd.h"
#include "logfmt_codec.h"

extern "C" __attribute__((visibility("hidden"))) int deepep_amd_set_error(int code, const char* msg);

namespace {

using deepep::lf_u32x2;
using deepep::lf_u32x4;

constexpr int kRowsPerBlock = 4;                         // one wave each

// The encode of one row by one wave: x (hidden bf16) -> low (hidden bytes), high (hidden / 4 bytes), meta
// (hidden / 128 dwords).  A lane past the row holds zeros and still runs the butterfly (hidden % 128 == 0: a 16-lane
// group is inside the row or outside).
__device__ __forceinline__ void encode_row(const lf_u32x4* __restrict__ xs, int hidden, uint8_t* __restrict__ low,
                                           uint8_t* __restrict__ high, uint32_t* __restrict__ meta, int lane) {
    const int nvec = hidden / 8;
    auto load = [&](int v) { return v < nvec ? __builtin_nontemporal_load(xs + v) : lf_u32x4{0u, 0u, 0u, 0u}; };
    lf_u32x4 next = load(lane);
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        const lf_u32x4 raw = next;
        next = load(v + 64);                             // in flight while this vector is reduced and encoded
        uint32_t amax = 0u, amin = 0x7fffu;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t m = deepep::lf_magnitude((raw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
            amax = max(amax, m);
            amin = min(amin, m);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), off, 64)));
            amin = min(amin, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amin), off, 64)));
        }
        const uint32_t word = amax | amin << 16;
        lf_u32x2 lo;
        uint32_t hi;
        deepep::lf_encode8(raw, deepep::lf_group(word), lo, hi);
        if (v < nvec) {
            reinterpret_cast<lf_u32x2*>(low)[v] = lo;
            reinterpret_cast<uint16_t*>(high)[v] = static_cast<uint16_t>(hi);
            if ((lane & 15) == 0) meta[v >> 4] = word;
        }
    }
}

__global__ void __launch_bounds__(64 * kRowsPerBlock)
cast_logfmt_kernel(const uint8_t* __restrict__ x, int64_t x_stride, int num_rows, int hidden,
                   uint8_t* __restrict__ planes, uint32_t* __restrict__ meta) {
    const int lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= num_rows) return;
    uint8_t* row = planes + t * (hidden + hidden / 4);
    encode_row(reinterpret_cast<const lf_u32x4*>(x + t * x_stride), hidden, row, row + hidden,
               meta + t * (hidden / 128), lane);
}

__global__ void __launch_bounds__(64 * kRowsPerBlock)
cast_back_logfmt_kernel(const uint8_t* __restrict__ planes, int64_t planes_stride, const uint32_t* __restrict__ meta,
                        int64_t meta_stride, int num_rows, int hidden, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= num_rows) return;
    const uint8_t* row = planes + t * planes_stride;
    const lf_u32x2* low = reinterpret_cast<const lf_u32x2*>(row);
    const uint16_t* high = reinterpret_cast<const uint16_t*>(row + hidden);
    const uint32_t* ms = meta + t * meta_stride;
    lf_u32x4* os = reinterpret_cast<lf_u32x4*>(out + t * hidden * 2);
    const int nvec = hidden / 8;
    for (int v = lane; v < nvec; v += 64) {
        const lf_u32x2 lo = __builtin_nontemporal_load(low + v);
        os[v] = deepep::lf_decode8(lo[0], lo[1], high[v], ms[v >> 4]);
    }
}

// Row t of the first num_rows packed rows: the bf16 part encoded, the weight tail (tail_bytes, whole 16-byte vectors)
// copied.
__global__ void __launch_bounds__(64 * kRowsPerBlock)
logfmt_pack_rows_kernel(const uint8_t* __restrict__ src, int64_t src_row_bytes, int src_tail_off, int num_rows,
                        int hidden, int tail_bytes, uint8_t* __restrict__ dst, int64_t dst_row_bytes, int dst_tail_off) {
    const int lane = threadIdx.x & 63;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= num_rows) return;
    const uint8_t* s = src + t * src_row_bytes;
    uint8_t* d = dst + t * dst_row_bytes;
    encode_row(reinterpret_cast<const lf_u32x4*>(s), hidden, d, d + hidden,
               reinterpret_cast<uint32_t*>(d + hidden + hidden / 4), lane);
    const lf_u32x4* ts = reinterpret_cast<const lf_u32x4*>(s + src_tail_off);
    lf_u32x4* td = reinterpret_cast<lf_u32x4*>(d + dst_tail_off);
    for (int i = lane; i < tail_bytes / 16; i += 64) td[i] = ts[i];
}

int invalid(const char* what, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, msg);
    return deepep_amd_set_error(DEEPEP_ERR_INVALID_ARG, buf);
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

unsigned grid_of(int num_rows) { return static_cast<unsigned>((static_cast<int64_t>(num_rows) + kRowsPerBlock - 1) / kRowsPerBlock); }

}  // namespace

extern "C" {

int deepep_cast_logfmt(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* planes, int32_t* meta,
                       deepep_stream_t stream) {
    const char* what = "cast_logfmt";
    if (num_rows == 0) return DEEPEP_OK;
    if (num_rows < 0 || hidden < 128 || hidden % 128 != 0) return invalid(what, "hidden must be a positive multiple of 128");
    if (x == nullptr || planes == nullptr || meta == nullptr || !a16(x) || !a16(planes) ||
        (reinterpret_cast<uintptr_t>(meta) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (x_row_stride_bytes < static_cast<int64_t>(hidden) * 2 || x_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden * 2 bytes or not 16-byte aligned");
    hipLaunchKernelGGL(cast_logfmt_kernel, dim3(grid_of(num_rows)), dim3(64 * kRowsPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(x), x_row_stride_bytes,
                       num_rows, hidden, static_cast<uint8_t*>(planes), reinterpret_cast<uint32_t*>(meta));
    return launch_status(what);
}

int deepep_cast_back_logfmt(const void* planes, int64_t planes_row_stride_bytes, const int32_t* meta,
                            int64_t meta_row_stride, int num_rows, int hidden, void* out, deepep_stream_t stream) {
    const char* what = "cast_back_logfmt";
    if (num_rows == 0) return DEEPEP_OK;
    if (num_rows < 0 || hidden < 128 || hidden % 128 != 0) return invalid(what, "hidden must be a positive multiple of 128");
    if (planes == nullptr || meta == nullptr || out == nullptr || !a16(planes) || !a16(out) ||
        (reinterpret_cast<uintptr_t>(meta) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned rows)");
    if (planes_row_stride_bytes < static_cast<int64_t>(hidden) + hidden / 4 || planes_row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below hidden * 5 / 4 bytes or not 16-byte aligned");
    if (meta_row_stride < hidden / 128) return invalid(what, "meta row stride below hidden / 128");
    hipLaunchKernelGGL(cast_back_logfmt_kernel, dim3(grid_of(num_rows)), dim3(64 * kRowsPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(planes),
                       planes_row_stride_bytes, reinterpret_cast<const uint32_t*>(meta), meta_row_stride, num_rows,
                       hidden, static_cast<uint8_t*>(out));
    return launch_status(what);
}

int deepep_logfmt_pack_rows(const void* src, int64_t src_row_bytes, int src_tail_offset, int num_rows, int hidden,
                            int tail_bytes, void* dst, int64_t dst_row_bytes, int dst_tail_offset,
                            deepep_stream_t stream) {
    const char* what = "logfmt_pack_rows";
    if (num_rows == 0) return DEEPEP_OK;
    if (num_rows < 0 || hidden < 128 || hidden % 128 != 0) return invalid(what, "hidden must be a positive multiple of 128");
    if (src == nullptr || dst == nullptr || !a16(src) || !a16(dst) || src_row_bytes % 16 != 0 || dst_row_bytes % 16 != 0)
        return invalid(what, "null pointers or rows not 16-byte aligned");
    const int64_t coded = static_cast<int64_t>(hidden) + hidden / 4 + hidden / 128 * 4;
    if (tail_bytes < 0 || tail_bytes % 16 != 0 || src_tail_offset % 16 != 0 || dst_tail_offset % 16 != 0 ||
        src_tail_offset < static_cast<int64_t>(hidden) * 2 || dst_tail_offset < coded ||
        src_row_bytes < static_cast<int64_t>(src_tail_offset) + tail_bytes ||
        dst_row_bytes < static_cast<int64_t>(dst_tail_offset) + tail_bytes)
        return invalid(what, "the weight tail does not lie behind the row's data and inside the row");
    hipLaunchKernelGGL(logfmt_pack_rows_kernel, dim3(grid_of(num_rows)), dim3(64 * kRowsPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(src), src_row_bytes,
                       src_tail_offset, num_rows, hidden, tail_bytes, static_cast<uint8_t*>(dst), dst_row_bytes,
                       dst_tail_offset);
    return launch_status(what);
}

}  // extern "C"
