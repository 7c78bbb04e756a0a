// router.hip -- the MoE gate's scoring and group-limited top-k on MI355X (deepep_route_topk): logits [T][E] from the
// gate's linear layer become topk_idx [T][K] and topk_weights [T][K], what ElasticBuffer.dispatch takes, in one kernel
// that reads each logit once and keeps no [T][E] temporary.  There is no counterpart in the reference, which takes the
// two tensors from its caller.  The definition is in include/deepep_amd.h; in short, per token and in fp32:
// s = sigmoid(x) or softmax(x), sel = s + bias, the num_topk_groups groups with the largest group score (the sum of a
// group's two largest sel, or its largest) stay, the K largest sel among them are chosen in descending order, an exact
// tie goes to the lower index, and w = s[chosen] / sum * routed_scaling_factor.
//
// Work split.  One wave owns a token; a workgroup is kWaves waves, each striding over the tokens (no count has to
// divide another).  Lane l holds the V = kUnits * (16 / sizeof(logit)) consecutive experts [l V, l V + V) of the row in
// registers -- V is 4, 8 or 16 for fp32 logits and 8 or 16 for bf16, the smallest with 64 V >= E -- loaded with kUnits
// 16-byte loads; lanes past E / V hold nothing.  A lane keeps two registers an expert: s, which becomes the weight, and
// `hi`, the order-preserving bits of sel (a float's bits with the sign bit flipped, or all bits when negative: unsigned
// order is then the floats' order, and 0 is below every number).  hi == 0 marks what cannot be chosen: padding, the
// experts of dropped groups, and winners already taken.
//
// The top-k is K rounds of a wave arg-max over one 64-bit key a lane, (hi, ~index): the lane's best is a strict `>`
// scan of its V registers in ascending index, the wave's a six-step butterfly of 64-bit maxima -- xor 1 and 2 as quad
// permutes, 4 and 8 as the row's half mirror and mirror (DPP; after the steps before, any pairing of the halves will
// do), 16 and 32 as __shfl_xor -- so every lane ends with the same key and the lower index wins a tie at no cost.  The
// winner's owner clears its hi; its s goes to lane k with one v_readlane.  After K rounds lane k holds result k: the
// normalising sum is one more butterfly, the division is IEEE, and both stores of a row are one coalesced run.
//
// The group stage (compiled out without groups) takes the groups one at a time: a lane's top two of its registers that
// lie in the group (a group need not be whole lanes: E = 160 in 8 groups of 20 on 8-expert lanes), merged over the
// wave by the same butterfly on (largest, second) pairs; lane g keeps group g's score.  A lane's rank is then the
// number of groups that beat its own under (score, lower index first), counted over v_readlane of the G scores, and
// the ballot of rank < num_topk_groups is the mask that clears the dropped groups' hi.
//
// The exponentials.  v_exp_f32 is good to 1 ulp, but rounding its argument x log2(e) to fp32 costs |x log2(e)| 2^-24
// relative, some 5 ulp at |x| = 7.  exp_neg() therefore carries the product's rounding error and the low part of
// log2(e) into a first-order correction, and the softmax subtracts the row maximum with an exact two-term difference.
//
// counts: a workgroup adds its waves' choices into an LDS histogram and flushes the non-zero bins with one vector
// atomicAdd each; the entry clears counts with a small kernel first (no memset node: the call captures into a graph).
// Integer adds: the result does not depend on timing.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): DESIGN.md section 3.
#include "cast_common.h"

namespace {

constexpr int kWaves = 4;                  // waves (tokens in flight) a workgroup
constexpr int kMaxExperts = 1024;          // 64 lanes x 16 registers; the LDS histogram's bins
constexpr int kMaxGrid = 2048;             // workgroups: 8 waves a SIMD on 256 CUs; more tokens are strided over

struct RouteArgs {
    const uint8_t* logits;
    int64_t row_stride;                    // bytes
    const float* bias;                     // or nullptr
    int num_tokens, num_experts, num_topk;
    int num_groups, num_topk_groups, group_max;
    uint32_t group_magic;                  // ceil(2^20 / group size): expert * magic >> 20 is its group, below 1024
    int norm;
    float scale;
    void* topk_idx;
    int idx32;
    float* topk_weights;
    int32_t* counts;                       // or nullptr
};

// ---------------------------------------------------------------- cross-lane steps (the controls: cast_common.h)

template <int kStep>
__device__ __forceinline__ uint32_t partner(uint32_t v) {
    if constexpr (kStep < 4) {
        constexpr int kCtrl = kStep == 0 ? kDppXor1 : kStep == 1 ? kDppXor2 : kStep == 2 ? kDppHalfMirror : kDppRowMirror;
        return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), kCtrl, 0xf, 0xf, true));
    } else {
        return static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), kStep == 4 ? 16 : 32));
    }
}

template <int kStep>
__device__ __forceinline__ float partner(float v) {
    return __builtin_bit_cast(float, partner<kStep>(__builtin_bit_cast(uint32_t, v)));
}

// every step pairs lane a with lane b both ways, and + and max commute: all 64 lanes end with the same bits
template <bool kMax, int kStep = 0>
__device__ __forceinline__ float wave_reduce(float v) {
    if constexpr (kStep == 6) return v;
    else {
        const float o = partner<kStep>(v);
        return wave_reduce<kMax, kStep + 1>(kMax ? fmaxf(v, o) : v + o);
    }
}

// the wave's largest (hi, lo) as a 64-bit number, in every lane
template <int kStep = 0>
__device__ __forceinline__ void wave_argmax(uint32_t& hi, uint32_t& lo) {
    if constexpr (kStep < 6) {
        const uint32_t oh = partner<kStep>(hi), ol = partner<kStep>(lo);
        const bool take = oh > hi || (oh == hi && ol > lo);
        hi = take ? oh : hi;
        lo = take ? ol : lo;
        wave_argmax<kStep + 1>(hi, lo);
    }
}

// the wave's two largest of every lane's (m1 >= m2), in every lane
template <int kStep = 0>
__device__ __forceinline__ void wave_top2(uint32_t& m1, uint32_t& m2) {
    if constexpr (kStep < 6) {
        const uint32_t o1 = partner<kStep>(m1), o2 = partner<kStep>(m2);
        const uint32_t second = max(min(m1, o1), max(m2, o2));
        m1 = max(m1, o1);
        m2 = second;
        wave_top2<kStep + 1>(m1, m2);
    }
}

// ---------------------------------------------------------------- the numbers
// a float's bits in unsigned order (no NaN): negative numbers below positive ones, every number above 0
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return u ^ (static_cast<uint32_t>(static_cast<int32_t>(u) >> 31) | 0x80000000u);
}

__device__ __forceinline__ float unordered(uint32_t o) {
    return __builtin_bit_cast(float, o ^ (static_cast<uint32_t>(static_cast<int32_t>(~o) >> 31) | 0x80000000u));
}

constexpr float kLog2eHi = 1.44269502162933349609375f;     // fp32(log2(e))
constexpr float kLog2eLo = 1.92596299e-8f;                 // log2(e) - kLog2eHi
constexpr float kLn2 = 0.693147182f;

// exp(d + d_lo) for d <= 0, |d_lo| below an ulp of d: v_exp_f32 of the rounded product, times 2^(what the rounding
// dropped) to first order.  Results below 2^-126 are flushed to 0, so an argument below kExpFloor -- or one that is no
// number at all, the difference of two infinities or of two numbers whose difference overflows -- is taken as
// kExpFloor: every product below stays finite, and the result is the same 0.
constexpr float kExpFloor = -128.0f;

__device__ __forceinline__ float exp_neg(float d, float d_lo) {
    const bool far = !(d >= kExpFloor);
    d = far ? kExpFloor : d;
    d_lo = far ? 0.0f : d_lo;
    const float p = d * kLog2eHi;
    const float dropped = __builtin_fmaf(d, kLog2eLo, __builtin_fmaf(d, kLog2eHi, -p)) + d_lo * kLog2eHi;
    const float t = __builtin_amdgcn_exp2f(p);
    return __builtin_fmaf(t, dropped * kLn2, t);
}

// 1 / (1 + exp(-x)) with t = exp(-|x|) in [0, 1]: 1 + t stays in [1, 2], and exp_neg takes any |x|, infinite too:
// sigmoid(-inf) = 0, sigmoid(+inf) = 1
__device__ __forceinline__ float sigmoid(float x) {
    const float t = exp_neg(-fabsf(x), 0.0f);
    const float r = __builtin_amdgcn_rcpf(1.0f + t);
    return x < 0.0f ? t * r : r;
}

// ---------------------------------------------------------------- the kernel
__global__ void zero_counts_kernel(int32_t* __restrict__ counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// In: float or uint16_t (bf16 bits).  kSoftmax: the score function.  kGroups: the group stage.  kUnits: 16-byte loads
// a lane.  K, the group sizes and every other scalar are arguments.
template <typename In, bool kSoftmax, bool kGroups, int kUnits>
__global__ void __launch_bounds__(64 * kWaves) route_topk_kernel(const RouteArgs a) {
    constexpr int kUnitVals = 16 / static_cast<int>(sizeof(In));
    constexpr int V = kUnits * kUnitVals;
    __shared__ int32_t hist[kMaxExperts];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int E = a.num_experts, K = a.num_topk;
    const bool counting = a.counts != nullptr;             // uniform over the grid
    if (counting) {
        for (int e = threadIdx.x; e < E; e += 64 * kWaves) hist[e] = 0;
        __syncthreads();
    }

    const int base = lane * V;                             // the lane's first expert
    const int held = min(max(E - base, 0), V);             // its experts: a multiple of kUnitVals (E % 8 == 0)
    float bias[V];
#pragma unroll
    for (int i = 0; i < V; ++i) bias[i] = (a.bias != nullptr && i < held) ? a.bias[base + i] : 0.0f;
    [[maybe_unused]] uint32_t group[V];                    // the group of each register
    if constexpr (kGroups) {
#pragma unroll
        for (int i = 0; i < V; ++i) group[i] = (static_cast<uint32_t>(base + i) * a.group_magic) >> 20;
    }

    for (int64_t t = static_cast<int64_t>(blockIdx.x) * kWaves + wave; t < a.num_tokens;
         t += static_cast<int64_t>(gridDim.x) * kWaves) {  // wave-uniform: every lane of a wave is in every round
        // ---- the row: each logit once, 16 bytes a load
        const uint8_t* row = a.logits + t * a.row_stride + static_cast<int64_t>(base) * sizeof(In);
        float x[V];
#pragma unroll
        for (int j = 0; j < kUnits; ++j) {
            u32x4 v{0u, 0u, 0u, 0u};
            if (j * kUnitVals < held) v = *reinterpret_cast<const u32x4*>(row + 16 * j);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint32_t word = v[m];
                if constexpr (sizeof(In) == 4) {
                    x[4 * j + m] = __builtin_bit_cast(float, word);
                } else {
                    x[8 * j + 2 * m] = __builtin_bit_cast(float, word << 16);
                    x[8 * j + 2 * m + 1] = __builtin_bit_cast(float, word & 0xffff0000u);
                }
            }
        }

        // ---- s and the order-preserving bits of sel = s + bias
        float s[V];
        if constexpr (kSoftmax) {
            float top = -INFINITY;
#pragma unroll
            for (int i = 0; i < V; ++i) top = fmaxf(top, i < held ? x[i] : -INFINITY);
            top = wave_reduce<true>(top);
            float sum = 0.0f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                // x - top = d + d_lo exactly (the two-term sum of x and -top); x = -inf, or a difference that
                // overflows, makes both no numbers, which exp_neg takes as its floor: s = 0
                const float d = x[i] - top, back = d - x[i];
                const float d_lo = (x[i] - (d - back)) + (-top - back);
                s[i] = i < held ? exp_neg(d, d_lo) : 0.0f;
                sum += s[i];
            }
            const float inv = 1.0f / wave_reduce<false>(sum);
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] *= inv;
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = sigmoid(x[i]);
        }
        uint32_t hi[V];
#pragma unroll
        for (int i = 0; i < V; ++i) hi[i] = i < held ? ordered(s[i] + bias[i]) : 0u;

        // ---- the group stage: group g's score to lane g, the lanes' ranks, the dropped groups cleared
        if constexpr (kGroups) {
            uint32_t score = 0u;
            for (int g = 0; g < a.num_groups; ++g) {
                uint32_t m1 = 0u, m2 = 0u;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t v = group[i] == static_cast<uint32_t>(g) ? hi[i] : 0u;
                    m2 = max(m2, min(m1, v));
                    m1 = max(m1, v);
                }
                wave_top2(m1, m2);
                const float largest = unordered(m1);
                const uint32_t of_group = ordered(a.group_max ? largest : largest + unordered(m2));
                score = lane == g ? of_group : score;
            }
            int rank = 0;
            for (int g = 0; g < a.num_groups; ++g) {
                const uint32_t other = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(score), g));
                rank += (other > score || (other == score && g < lane)) ? 1 : 0;
            }
            const uint64_t kept = __ballot(lane < a.num_groups && rank < a.num_topk_groups);
#pragma unroll
            for (int i = 0; i < V; ++i) hi[i] = ((kept >> (group[i] & 63u)) & 1u) != 0 ? hi[i] : 0u;
        }

        // ---- K rounds of the wave arg-max; result k stays in lane k
        uint32_t my_idx = 0u;
        float my_s = 0.0f;
        for (int k = 0; k < K; ++k) {
            uint32_t kh = hi[0], at = 0u;
#pragma unroll
            for (int i = 1; i < V; ++i) {
                const bool better = hi[i] > kh;
                kh = better ? hi[i] : kh;
                at = better ? static_cast<uint32_t>(i) : at;
            }
            uint32_t kl = ~(static_cast<uint32_t>(base) + at);
            wave_argmax(kh, kl);
            const uint32_t winner = ~static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(kl)));
            const uint32_t mine = winner - static_cast<uint32_t>(base);        // below V in the owner alone
            float chosen = s[0];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                hi[i] = mine == static_cast<uint32_t>(i) ? 0u : hi[i];
                chosen = mine == static_cast<uint32_t>(i) ? s[i] : chosen;
            }
            const float s_winner = __builtin_bit_cast(
                float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, chosen), static_cast<int>(winner / V)));
            my_idx = lane == k ? winner : my_idx;
            my_s = lane == k ? s_winner : my_s;
        }

        // ---- the weights and the two stores of the row
        const float sum = wave_reduce<false>(lane < K ? my_s : 0.0f);
        const float w = (a.norm ? my_s / sum : my_s) * a.scale;
        if (lane < K) {
            const int64_t o = t * K + lane;
            if (a.idx32) static_cast<int32_t*>(a.topk_idx)[o] = static_cast<int32_t>(my_idx);
            else static_cast<int64_t*>(a.topk_idx)[o] = static_cast<int64_t>(my_idx);
            a.topk_weights[o] = w;
            if (counting && my_idx < static_cast<uint32_t>(E)) atomicAdd(&hist[my_idx], 1);
        }
    }

    if (counting) {
        __syncthreads();
        for (int e = threadIdx.x; e < E; e += 64 * kWaves) {
            const int32_t c = hist[e];
            if (c != 0) atomicAdd(a.counts + e, c);
        }
    }
}

// ---------------------------------------------------------------- the launches, over what changes the instructions
template <typename In, bool kSoftmax, bool kGroups, int kUnits>
void launch(const RouteArgs& a, hipStream_t stream) {
    const int blocks = (a.num_tokens + kWaves - 1) / kWaves, grid = blocks < kMaxGrid ? blocks : kMaxGrid;
    hipLaunchKernelGGL((route_topk_kernel<In, kSoftmax, kGroups, kUnits>), dim3(grid), dim3(64 * kWaves), 0, stream, a);
}

template <typename In, int kUnits>
void launch_units(const RouteArgs& a, bool softmax, hipStream_t stream) {
    const bool groups = a.num_groups > 1;
    if (softmax) groups ? launch<In, true, true, kUnits>(a, stream) : launch<In, true, false, kUnits>(a, stream);
    else groups ? launch<In, false, true, kUnits>(a, stream) : launch<In, false, false, kUnits>(a, stream);
}

}  // namespace

extern "C" {

int deepep_route_topk(const void* logits, int logits_bf16, int64_t row_stride_bytes, const float* bias, int num_tokens,
                      int num_experts, int num_topk, int score_func, int num_groups, int num_topk_groups,
                      int group_score, int norm_topk_prob, float routed_scaling_factor, void* topk_idx, int idx_bits,
                      float* topk_weights, int32_t* counts, deepep_stream_t stream) {
    const char* what = "route_topk";
    if (num_tokens == 0) return DEEPEP_OK;
    if (num_tokens < 0) return invalid(what, "num_tokens must not be negative");
    if (num_experts < 8 || num_experts > kMaxExperts || num_experts % 8 != 0)
        return invalid(what, "num_experts must be a multiple of 8 from 8 to 1024");
    if (score_func != DEEPEP_ROUTE_SIGMOID && score_func != DEEPEP_ROUTE_SOFTMAX)
        return invalid(what, "score_func is DEEPEP_ROUTE_SIGMOID or DEEPEP_ROUTE_SOFTMAX");
    if (group_score != DEEPEP_ROUTE_GROUP_TOP2_SUM && group_score != DEEPEP_ROUTE_GROUP_MAX)
        return invalid(what, "group_score is DEEPEP_ROUTE_GROUP_TOP2_SUM or DEEPEP_ROUTE_GROUP_MAX");
    if (num_groups < 1 || num_groups > 64 || num_experts % num_groups != 0)
        return invalid(what, "num_groups must be from 1 to 64 and divide num_experts");
    const int group_size = num_experts / num_groups;
    if (num_topk_groups < 1 || num_topk_groups > num_groups)
        return invalid(what, "num_topk_groups must be from 1 to num_groups");
    if (num_groups > 1 && group_score == DEEPEP_ROUTE_GROUP_TOP2_SUM && group_size < 2)
        return invalid(what, "DEEPEP_ROUTE_GROUP_TOP2_SUM needs at least 2 experts a group");
    if (num_topk < 1 || num_topk > 64 || num_topk > num_topk_groups * group_size)
        return invalid(what, "num_topk must be from 1 to 64 and at most the experts of the kept groups");
    if (idx_bits != 32 && idx_bits != 64) return invalid(what, "idx_bits is 32 or 64");
    if (logits == nullptr || topk_idx == nullptr || topk_weights == nullptr || !a16(logits) ||
        (reinterpret_cast<uintptr_t>(topk_idx) & (idx_bits / 8 - 1)) != 0 ||
        (reinterpret_cast<uintptr_t>(topk_weights) & 3u) != 0 || (reinterpret_cast<uintptr_t>(bias) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(counts) & 3u) != 0)
        return invalid(what, "null or misaligned pointers (16-byte aligned logits rows)");
    if (row_stride_bytes < static_cast<int64_t>(num_experts) * (logits_bf16 ? 2 : 4) || row_stride_bytes % 16 != 0)
        return invalid(what, "row stride below a row's bytes or not 16-byte aligned");

    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (counts != nullptr) hipLaunchKernelGGL(zero_counts_kernel, dim3((num_experts + 255) / 256), dim3(256), 0, s,
                                              counts, num_experts);
    const RouteArgs a{static_cast<const uint8_t*>(logits), row_stride_bytes, bias, num_tokens, num_experts, num_topk,
                      num_groups, num_topk_groups, group_score == DEEPEP_ROUTE_GROUP_MAX,
                      static_cast<uint32_t>(((1 << 20) + group_size - 1) / group_size), norm_topk_prob != 0,
                      routed_scaling_factor, topk_idx, idx_bits == 32, topk_weights, counts};
    const bool softmax = score_func == DEEPEP_ROUTE_SOFTMAX;
    if (logits_bf16) {                                     // 8 experts a load
        if (num_experts <= 512) launch_units<uint16_t, 1>(a, softmax, s);
        else launch_units<uint16_t, 2>(a, softmax, s);
    } else {                                               // 4 experts a load
        if (num_experts <= 256) launch_units<float, 1>(a, softmax, s);
        else if (num_experts <= 512) launch_units<float, 2>(a, softmax, s);
        else launch_units<float, 4>(a, softmax, s);
    }
    return launch_status(what);
}

}  // extern "C"
