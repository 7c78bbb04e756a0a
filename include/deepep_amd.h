/*
 * deepep_amd.h -- C-ABI of libdeepep_amd.so, the MI355X (gfx950) combine reduction.
 *
 * Plain C: raw device pointers, sizes and a hipStream_t; no torch types.  Every
 * entry point returns DEEPEP_OK (0) or a negative DEEPEP_ERR_* code; the message
 * of the last failure on the calling thread is available from
 * deepep_amd_last_error().  The Python host layer (deepep_amd/_lib.py) turns a
 * non-zero code into RuntimeError, which is what the reference raises for a
 * failed EP_HOST_ASSERT (EPException -> RuntimeError,
 * deep_ep/include/deep_ep/common/exception.cuh:11-37 in /root/reference).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   deepep_combine_reduce(mode = DEEPEP_MODE_LOCAL)
 *       launch_combine / combine_impl, the per-received-token local reduce
 *       (csrc/kernels/elastic/combine.hpp:114-193,
 *        deep_ep/include/deep_ep/impls/combine.cuh:28-243)
 *   deepep_combine_reduce(mode = DEEPEP_MODE_EPILOGUE)
 *       launch_combine_reduce_epilogue / combine_reduce_epilogue_impl
 *       (csrc/kernels/elastic/combine.hpp:248-287,
 *        deep_ep/include/deep_ep/impls/combine_reduce_epilogue.cuh:24-143)
 *   deepep_combine_reduce(mode = DEEPEP_MODE_FUSED)
 *       both of the above at EP = 1, fused into one pass (no receive buffer)
 *   deepep_build_local_plan
 *       the token -> slot lookup that combine_reduce_epilogue_impl performs per
 *       token through the symmetric receive buffer (combine_reduce_epilogue.cuh:62-95),
 *       materialised once per handle
 *   deepep_combine_buffer_size
 *       ElasticBuffer::get_combine_buffer_size (csrc/elastic/buffer.hpp:616-650)
 *   deepep_dispatch_notify (or _route / _expert_counts) / _pack   (the handle producer, send side)
 *       dispatch_impl's notify, slot assignment and token push
 *       (deep_ep/include/deep_ep/impls/dispatch.cuh:79-258, 336-392)
 *   deepep_cast_fp8 / deepep_dispatch_pack_cast / deepep_dispatch_copy_cast   (the per-token FP8 cast, alone,
 *       fused into the push and, at one rank, into the receive-side copy)
 *       per_token_cast_to_fp8 (deep_ep/utils/math.py:30-39); the use_fp8 / round_scale branch of the legacy
 *       low-latency send kernel (csrc/kernels/legacy/internode_ll.cu:220-245, utils.cuh:494-503)
 *   deepep_cast_back_fp8   (the inverse, for the received pair)
 *       per_token_cast_back (deep_ep/utils/math.py:42-56)
 *   deepep_cast_fp8_ue8m0 / deepep_cast_back_fp8_ue8m0 / deepep_dispatch_pack_cast_ue8m0 /
 *   deepep_dispatch_copy_cast_ue8m0   (the four above with packed UE8M0 scale factors)
 *       the use_ue8m0 form of the legacy low-latency dispatch (csrc/kernels/legacy/internode_ll.cu:439-459,
 *       utils.cuh:505-512) and the torch.int branch of per_token_cast_back (deep_ep/utils/math.py:51-53)
 *   deepep_cast_fp8_mx / deepep_cast_back_fp8_mx / deepep_dispatch_pack_cast_mx / deepep_dispatch_copy_cast_mx
 *       (the same four as MXFP8: one UE8M0 exponent byte per 32 columns, the operand of gfx950's block-scaled
 *       MFMA; no counterpart in the reference, whose groups are 128 columns)
 *   deepep_cast_fp8_mx_transposed   (the MXFP8 cast with the groups of 32 along the token axis, stored
 *       [hidden][rows]: the weight-gradient operand of the same MFMA; optionally the row-wise pair from the same read)
 *       (none: the wgrad operand of v_mfma_scale_f32_*_f8f6f4; the reference has no transposed cast)
 *   deepep_cast_fp4_mx / deepep_cast_back_fp4_mx / deepep_dispatch_pack_cast_fp4_mx /
 *   deepep_dispatch_copy_cast_fp4_mx
 *       (the same four as MXFP4: e2m1 rows, two codes to a byte, with the MXFP8 exponent bytes; no counterpart in
 *       the reference)
 *   deepep_cast_fp6_mx / deepep_cast_back_fp6_mx / deepep_dispatch_pack_cast_fp6_mx /
 *   deepep_dispatch_copy_cast_fp6_mx   (and deepep_cast_fp6_mx_stores, the cast with its store width chosen)
 *       (the same four as MXFP6: e2m3 rows, 32 codes to 24 bytes, with the MXFP8 exponent bytes; no counterpart in
 *       the reference)
 *   deepep_cast_fp4_mx_transposed / deepep_cast_fp6_mx_transposed   (deepep_cast_fp8_mx_transposed over e2m1 and e2m3)
 *       (none: the FP4 / FP6 wgrad operand of v_mfma_scale_f32_*_f8f6f4)
 *   deepep_requant_fp8_mx_transposed / deepep_requant_fp4_mx_transposed / deepep_requant_fp6_mx_transposed
 *       (the transposed casts from a row-wise quantised pair: the cast back fused into their load)
 *       (none: the wgrad operand from what a casting dispatch returns)
 *   deepep_cast_logfmt / deepep_cast_back_logfmt / deepep_logfmt_pack_rows / deepep_combine_reduce_logfmt /
 *   deepep_combine_reduce_scatter_logfmt
 *       the use_logfmt rows of the legacy low-latency combine (csrc/kernels/legacy/internode_ll.cu:557-638 encode,
 *       :672-712 decode)
 *   deepep_dispatch_count / _scan / _slots / _copy   (receive side)
 *       dispatch_copy_epilogue_impl (deep_ep/include/deep_ep/impls/dispatch_copy_epilogue.cuh:11-323)
 *   deepep_route_block_counts / deepep_plan_expert / deepep_plan_source   (EP > 1 combine plan)
 *       the addressing combine_impl and combine_reduce_epilogue_impl derive inside every launch
 *       (combine.cuh:96-106, combine_reduce_epilogue.cuh:62-95), built once per handle on the device
 * The Python-facing runtime call these serve is _C.ElasticBuffer.combine
 * (csrc/elastic/buffer.hpp:1179-1343), re-implemented in deepep_amd/buffer.py.
 */
#ifndef DEEPEP_AMD_H
#define DEEPEP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* deepep_stream_t;   /* == hipStream_t */

#define DEEPEP_AMD_ABI_VERSION 14

#define DEEPEP_OK               0
#define DEEPEP_ERR_INVALID_ARG  (-1)
#define DEEPEP_ERR_UNSUPPORTED  (-2)
#define DEEPEP_ERR_HIP          (-3)

/* Error record: the error_flag of the window paths (the scatter, plan_expert, the xGMI dispatch pack)
 * points at DEEPEP_ERROR_RECORD_INTS device ints.  [0] = flag bits: 1 = a slot / unit was rejected
 * (skipped, never dereferenced), 2 = a window barrier timed out, 4 = a computed window address fell
 * outside every window (nothing stored there).  [1..7] = the first fault with bit 4 or a rejected plan
 * entry: [1] kind (DEEPEP_FAULT_*), [2] unit / token / row, [3] rank / lane, [4] address low 32 bits,
 * [5] address high 32 bits, [6] an extra value (the extent it exceeded, in 16-byte units).  The host
 * layer raises RuntimeError with this record at the next call.  The other entry points that take an
 * error_flag use [0] only. */
#define DEEPEP_ERROR_RECORD_INTS 8
#define DEEPEP_FLAG_BAD_SLOT     1
#define DEEPEP_FLAG_TIMEOUT      2
#define DEEPEP_FLAG_BAD_ADDRESS  4
#define DEEPEP_FAULT_SCATTER_ROW 1   /* deepep_combine_reduce_scatter: out_rows[u] outside every window  */
#define DEEPEP_FAULT_PLAN_ROW    2   /* deepep_plan_expert: window row past the window's data extent     */
#define DEEPEP_FAULT_PLAN_UNIT   3   /* deepep_plan_expert: unit position / received row out of range     */
#define DEEPEP_FAULT_PACK_ROW    4   /* deepep_dispatch_pack: destination row past the destination buffer */

/* Reduction modes of deepep_combine_reduce. */
#define DEEPEP_MODE_LOCAL     0   /* phase A: copy if 1 valid slot, hadd if 2, else fp32 sum   */
#define DEEPEP_MODE_EPILOGUE  1   /* phase B: bias0 + bias1 + partials (hadd bypass w/o bias)    */
#define DEEPEP_MODE_FUSED     2   /* phase A then phase B over the single partial (EP = 1)       */

int deepep_amd_abi_version(void);
const char* deepep_amd_last_error(void);
/* 16 hex digits: sha256 of the sources, this header and the compile flags the library was built
 * from (deepep_amd/_lib.py source_build_id); the Python loader refuses a binary whose id does not
 * match the sources next to it. */
const char* deepep_amd_build_id(void);

/*
 * Per unit u in [0, num_units): gather the source rows listed in
 * table[u * table_stride + j] (j < table_width, entries < 0 are skipped; a NULL
 * table means the single row u), reduce them in ascending j in fp32 with the
 * reference's rounding rules for `mode`, and write one bf16 row to
 * out + u * out_row_stride.
 *
 *   src            bf16 [num_src_rows][src_row_stride], rows 16-byte aligned
 *   hidden         elements per row; hidden % 8 == 0
 *   weighted       0: plain sum (ElasticBuffer semantics);
 *                  1: row j scaled by row_weights[slot_j] with an fp32 fma chain
 *                     (legacy low_latency_combine semantics, csrc/kernels/legacy/
 *                     internode_ll.cu:1072-1135); in mode EPILOGUE (the single-reduction
 *                     combine) the chain starts from +0 + bias0 + bias1
 *   bias0, bias1   bf16 [num_units][hidden] or NULL (modes EPILOGUE and FUSED)
 *   out_weights    fp32 rows of out_weights_stride floats (0 = num_weights) or NULL: top-k
 *                  weight pass-through, written once per unit:
 *                  out_weights[u*out_weights_stride + k] = (i = wtable ? wtable[u*wtable_stride + k]
 *                                                             : u*num_weights + k) >= 0 ? wsrc[i] : 0
 *                  (a stride lets the weights ride in the tail of packed exchange rows)
 *   weights_pad    floats written per weight row (<= 64; values below num_weights mean num_weights):
 *                  the entries past num_weights are zeros.  32 writes a packed row's whole 128-byte
 *                  tail line at once: a partial-line store costs the memory side a read-modify-write
 *   units_per_block  workgroup shape: 4 = 4 (row, column-chunk) items per 256-thread workgroup,
 *                  8 = 8 items per 512-thread workgroup, 0 = automatic (4 for LOCAL, else 8)
 *   error_flag     device int or NULL; bit 1 is set when a slot is >= num_src_rows (such slots are
 *                  skipped, never dereferenced).  When bit 2 is already set (a symmetric-window
 *                  barrier timed out, deepep_sym_barrier) the launch stores NaN rows instead of sums
 *                  (and deepep_combine_reduce_scatter stores nothing into the peers' windows)
 */
int deepep_combine_reduce(int mode, int weighted,
                          const void* src, int64_t num_src_rows, int64_t src_row_stride,
                          const int32_t* table, int64_t table_stride, int table_width,
                          const float* row_weights,
                          const void* bias0, const void* bias1,
                          void* out, int64_t out_row_stride,
                          int num_units, int hidden,
                          const int32_t* wtable, int64_t wtable_stride,
                          const float* wsrc, float* out_weights, int num_weights,
                          int64_t out_weights_stride, int weights_pad,
                          int units_per_block, int32_t* error_flag,
                          deepep_stream_t stream);

/*
 * deepep_combine_reduce over FP8 source rows: the same reduction with every source element cast back in
 * registers, bf16_rne(fp32(e4m3fn) * sf), before it enters the sum -- bit for bit the result of
 * deepep_cast_back_fp8 (or _ue8m0) into a bf16 buffer followed by deepep_combine_reduce over that buffer,
 * without the buffer.  Replaces per_token_cast_back (deep_ep/utils/math.py:42-56) in front of
 * ElasticBuffer.combine (deep_ep/buffers/elastic.py:1046-1107) for expert rows held as an FP8 pair.
 * The arguments are deepep_combine_reduce's, with the scale factors after the source:
 *   src            e4m3fn [num_src_rows][src_row_stride], 16-byte aligned; src_row_stride counts e4m3fn
 *                  elements, is a multiple of 16 and >= hidden
 *   hidden         hidden % 128 == 0 (% 512 == 0 when sf_packed)
 *   sf             sf_packed == 0: fp32 [num_src_rows][hidden / 128], one factor per 128 columns;
 *                  sf_packed != 0: int32 [num_src_rows][hidden / 512], four UE8M0 exponent bytes each (byte j,
 *                  little-endian, of element p is column group 4p + j; the factor is float_from_bits(byte << 23)).
 *                  4-byte aligned, not NULL.  Element (r, c) is at sf[r * sf_row_stride + c * sf_col_stride], so a
 *                  column-major tensor is read in place.  Only rows named by a valid slot are read
 *   units_per_block  honoured by modes LOCAL and FUSED; the epilogue keeps 8 items per workgroup
 * Everything else (table, weights, bias, out, pass-through, error_flag, modes) as deepep_combine_reduce; out and
 * the bias rows are bf16.  Finite bytes and positive finite normal factors are the contract, as for the cast back.
 */
int deepep_combine_reduce_fp8(int mode, int weighted,
                              const void* src, int64_t num_src_rows, int64_t src_row_stride,
                              const void* sf, int64_t sf_row_stride, int64_t sf_col_stride, int sf_packed,
                              const int32_t* table, int64_t table_stride, int table_width,
                              const float* row_weights,
                              const void* bias0, const void* bias1,
                              void* out, int64_t out_row_stride,
                              int num_units, int hidden,
                              const int32_t* wtable, int64_t wtable_stride,
                              const float* wsrc, float* out_weights, int num_weights,
                              int64_t out_weights_stride, int weights_pad,
                              int units_per_block, int32_t* error_flag,
                              deepep_stream_t stream);

/*
 * Token-major slot table for the EP = 1 fused path, from the handle's
 * recv_src_metadata ([num_recv_tokens][num_topk + 2] int32, column 0 =
 * src_rank * num_max_tokens_per_rank + src_token, columns 2.. = expanded slots).
 *   expanded = 1: plan[t][k] = metadata slot k of the token received from t, else -1
 *   expanded = 0: plan[t][0] = i (the received row of t), else -1
 * plan is [num_tokens][plan_width] int32 (plan_width = num_topk or 1) and is fully
 * written.  When wtable is not NULL ([num_tokens][num_topk]) it receives the
 * weight-source index of the non-expanded pass-through: i*num_topk + k where
 * topk_idx[t][k] >= 0, else -1 (topk_idx is int64 [num_tokens][num_topk]).
 */
int deepep_build_local_plan(const int32_t* src_metadata, int num_recv_tokens, int num_topk,
                            int num_max_tokens_per_rank, int expanded,
                            int32_t* plan, int plan_width, int num_tokens,
                            const int64_t* topk_idx, int32_t* wtable,
                            deepep_stream_t stream);

/*
 * Tuning / diagnostics: vec_per_lane = 16-byte vectors each lane loads per source row and item (1 or 2),
 * rows_in_flight = source rows each lane loads before accumulating them (2, 4 or 8); 0 = automatic, the
 * default.  Process-wide, stored as one atomic word that every launch reads once.  Automatic shape: 2 KiB
 * chunks (1 KiB for rows under 128 vectors); rows in flight at most the slot table's width rounded up to
 * 2 / 4 / 8, and 2 (with 1 KiB chunks and 4-wave workgroups) for the fused reduce over top-k >= 5, 8 for
 * the epilogue, 4 for phase A (DEEPEP_MODE_LOCAL) and for every launch on a CU-budget stream.  The store
 * policy follows the output: sc1 nt for phase A's send rows, system scope for peer windows
 * (deepep_combine_reduce_scatter), sc1 otherwise.  The results are identical for every configuration;
 * only the speed changes.
 */
int deepep_set_launch_config(int vec_per_lane, int rows_in_flight);

/* ------------------------------------------------------------------ dispatch
 * Packed token row exchanged between ranks (byte offsets, all 16-byte aligned except as noted):
 *   [x: x_bytes | sf @sf_off: sf_bytes | topk_idx int64[K] @idx_off | weights fp32[K] @w_off |
 *    src_global_idx int32 @src_off], row_bytes % 16 == 0.
 * Receive order: grouped by source rank, ascending source token (deterministic).
 */

/* dst_slot[t][r] = #{t' < t routed to rank r} or -1 (int32 [num_tokens][num_ranks]);
 * send_counts[r] = tokens routed to rank r.  A token is routed to r when one of its top-k experts
 * lives on r (experts_per_rank = num_experts / num_ranks).  block_counts: int32 scratch of
 * ceil(num_tokens / 256) * num_ranks entries. */
int deepep_dispatch_route(const int64_t* topk_idx, int num_tokens, int num_topk, int num_experts, int num_ranks,
                          int32_t* dst_slot, int32_t* send_counts, int32_t* block_counts, deepep_stream_t stream);

/* counts[e] = #{(t, k) : topk_idx[t][k] == e} (int32 [num_experts], zeroed first; entries < 0 are
 * masked slots).  The per-expert half of dispatch_impl's notify (dispatch.cuh:79-258): each sender
 * sends slice [r * experts_per_rank, (r + 1) * experts_per_rank) to rank r with its per-rank count, so
 * one exchange and one host sync give the receiver both its row count per source rank and its
 * rows per local expert. */
int deepep_dispatch_expert_counts(const int64_t* topk_idx, int num_tokens, int num_topk, int num_experts,
                                  int32_t* counts, deepep_stream_t stream);

/* The send side of a fresh dispatch in two launches: dst_slot as deepep_dispatch_route; notify int32
 * [num_ranks][W], W = 1 + experts_per_rank + 2 * num_blocks, row d = [tokens routed to d |
 * deepep_dispatch_expert_counts' slice of d's experts | per-64-token-block tokens routed to d
 * (deepep_route_block_counts' tok) | per-block (token, lane) pairs routed to d (its pairs)] -- the record
 * dispatch_impl's notify sends to d (dispatch.cuh:79-258); send_offsets int32 [num_ranks] = the exclusive
 * prefix of the per-rank token counts.  num_blocks may be 0 (no block counts, one rank) or >=
 * ceil(num_tokens / 64); blocks past the tokens hold 0.  No output needs zeroing.  workspace: device
 * scratch of at least deepep_dispatch_notify_workspace(...) bytes. */
int64_t deepep_dispatch_notify_workspace(int num_tokens, int num_experts, int num_ranks);
int deepep_dispatch_notify(const int64_t* topk_idx, int num_tokens, int num_topk, int num_experts, int num_ranks,
                           int num_blocks, int32_t* dst_slot, int32_t* notify, int32_t* send_offsets,
                           void* workspace, int64_t workspace_bytes, deepep_stream_t stream);

/* Write packed row send_offsets[r] + dst_slot[t][r] for every (token t, destination r), in `packed`
 * (dest_bases NULL: one local buffer for an all-to-all) or in rank r's buffer at dest_bases[r] (device
 * uint64 [num_ranks]: the peers' symmetric windows, system-scope stores -- the xGMI push of
 * dispatch.cuh:373-392); src_global_idx = src_base + t.  topk_weights may be NULL (zeros are sent).
 * dest_rows: rows every destination buffer holds (`packed`, or each peer window); a row index
 * send_offsets[r] + dst_slot[t][r] outside [0, dest_rows) is not stored: bit 4 of error_flag is set and
 * the fault recorded (DEEPEP_FAULT_PACK_ROW).  error_flag (device, DEEPEP_ERROR_RECORD_INTS ints, or
 * NULL): with dest_bases, nothing is stored once bit 2 is set (the window barrier before the push timed
 * out). */
int deepep_dispatch_pack(const void* x, int64_t x_row_stride_bytes, int x_bytes,
                         const void* sf, int64_t sf_row_stride_bytes, int sf_bytes,
                         const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                         int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks,
                         void* packed, const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows,
                         int sf_off, int idx_off, int w_off, int src_off, int32_t* error_flag,
                         deepep_stream_t stream);

/* Per-token FP8 cast, one scale factor per 128 columns: x bf16 [num_rows][hidden] (rows
 * x_row_stride_bytes apart) -> q OCP e4m3fn [num_rows][hidden] and sf fp32 [num_rows][hidden / 128], both
 * contiguous.  Replaces per_token_cast_to_fp8 (deep_ep/utils/math.py:30-39) bit for bit, per group:
 * amax = max(max|x|, 1e-4f), sf = amax / 448.0f, q = e4m3fn_rne(fp32(x) * ((1.0f / amax) * 448.0f)) -- torch
 * evaluates that function's `448.0 / amax` as reciprocal(amax) * 448, two roundings, and so does this; with
 * round_scale != 0 the scale is a power of two (calculate_fp8_scales(round_scale = true),
 * csrc/kernels/legacy/utils.cuh:494-503): v = amax * fp32(1 / 448), e = exponent(v) + (mantissa(v) != 0),
 * sf = 2^e, q = e4m3fn_rne(fp32(x) * 2^-e).  Inputs must be finite (NaN / Inf: unspecified).  Every input
 * row is read once.  hidden % 128 != 0, null or misaligned pointers (x, q: 16 bytes; sf: 4), a row stride
 * below hidden * 2 or not a multiple of 16 are rejected; num_rows == 0 is a no-op. */
int deepep_cast_fp8(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, int round_scale,
                    void* q, float* sf, deepep_stream_t stream);

/* The inverse of deepep_cast_fp8 for the pair an FP8 dispatch returns (per_token_cast_back,
 * deep_ep/utils/math.py:42-56, bit for bit): q OCP e4m3fn [num_rows][hidden] (rows q_row_stride_bytes apart),
 * sf fp32 [num_rows][hidden / 128] addressed as sf[row * sf_row_stride + group * sf_col_stride] (strides in
 * elements, so a column-major tensor is read in place) -> out bf16 [num_rows][hidden], contiguous:
 * out = bf16_rne(fp32(q) * sf) -- an exact conversion, one fp32 multiply, one round-to-nearest-even.  Covers
 * finite bytes and positive, finite, normal scale factors; the NaN bytes 0x7f / 0xff give a NaN (payload
 * unspecified).  hidden % 128 != 0, null or misaligned pointers (q, out: 16 bytes; sf: 4), a row stride below
 * hidden or not a multiple of 16 and negative scale-factor strides are rejected; num_rows == 0 is a no-op. */
int deepep_cast_back_fp8(const void* q, int64_t q_row_stride_bytes, const float* sf, int64_t sf_row_stride,
                         int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_dispatch_pack with the cast of deepep_cast_fp8 fused in (the reference fuses it into its
 * low-latency send kernel: use_fp8 / round_scale, csrc/kernels/legacy/internode_ll.cu:220-245): x is the
 * tokens' bf16 rows [num_tokens][hidden], each read once and quantised in registers; the packed row of
 * every destination gets [hidden e4m3fn bytes | hidden / 128 fp32 scale factors @sf_off | ...], i.e. what
 * deepep_dispatch_pack writes for x_bytes = hidden, sf_bytes = hidden / 128 * 4 and the cast (q, sf).
 * Everything else (destinations, dest_rows bound, error_flag, the timed-out-barrier early return) as
 * deepep_dispatch_pack.  The offsets must describe non-overlapping fields inside row_bytes. */
int deepep_dispatch_pack_cast(const void* x, int64_t x_row_stride_bytes, int hidden, int round_scale,
                              const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                              int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks,
                              void* packed, const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows,
                              int sf_off, int idx_off, int w_off, int src_off, int32_t* error_flag,
                              deepep_stream_t stream);

/* The FP8 entries with packed UE8M0 scale factors (additive: the ABI version stays).  The packed form needs
 * hidden % 512 == 0: the scale factors are int32 [rows][hidden / 512], byte j (little-endian) of element p the biased
 * exponent (bits(sf) >> 23) & 0xff of column group 4p + j, sf the power-of-two factor deepep_cast_fp8 gives with
 * round_scale != 0 -- what the reference's low-latency dispatch produces with use_ue8m0
 * (csrc/kernels/legacy/internode_ll.cu:439-459, extract_required_scale_format, legacy/utils.cuh:505-512) and its
 * per_token_cast_back accepts (deep_ep/utils/math.py:51-53).  The e4m3fn bytes are the round_scale != 0 bytes of the
 * sibling entry, and every other argument, bound and rejection is the sibling's (a pointer to scale factors: 4-byte
 * aligned); hidden % 512 != 0 is rejected before any launch.  Finite bf16 input keeps every byte inside 105..247.
 *
 * deepep_cast_fp8_ue8m0: deepep_cast_fp8(round_scale = 1) with sf int32 [num_rows][hidden / 512], contiguous. */
int deepep_cast_fp8_ue8m0(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, int32_t* sf,
                          deepep_stream_t stream);

/* deepep_cast_back_fp8 for packed scale factors: sf int32 [num_rows][hidden / 512], element p of a row at
 * sf[row * sf_row_stride + p * sf_col_stride] (strides in int32 elements: a column-major tensor is read in place);
 * out = bf16_rne(fp32(q) * float_from_bits(byte << 23)).  For bytes 1..254 this is deepep_cast_back_fp8 of the
 * factors 2^(byte - 127); byte 0 multiplies by +0.0f (signed zeros), byte 255 is unspecified. */
int deepep_cast_back_fp8_ue8m0(const void* q, int64_t q_row_stride_bytes, const int32_t* sf, int64_t sf_row_stride,
                               int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_dispatch_pack_cast(round_scale = 1) with the packed row [hidden e4m3fn bytes | hidden / 128 exponent
 * bytes @sf_off | ...]: what deepep_dispatch_pack writes for x_bytes = hidden, sf_bytes = hidden / 128 and the pair
 * of deepep_cast_fp8_ue8m0. */
int deepep_dispatch_pack_cast_ue8m0(const void* x, int64_t x_row_stride_bytes, int hidden,
                                    const int64_t* topk_idx, const float* topk_weights, int num_tokens, int num_topk,
                                    int32_t src_base, const int32_t* dst_slot, const int32_t* send_offsets,
                                    int num_ranks, void* packed, const uint64_t* dest_bases, int64_t row_bytes,
                                    int64_t dest_rows, int sf_off, int idx_off, int w_off, int src_off,
                                    int32_t* error_flag, deepep_stream_t stream);

/* The FP8 entries as MXFP8: OCP e4m3fn rows with one UE8M0 exponent byte per 32 columns, the group (and the scale
 * format) of gfx950's block-scaled MFMA, v_mfma_scale_f32_{32x32x64,16x16x128}_f8f6f4 (additive: the ABI version
 * stays).  hidden must be a positive multiple of 128.  Per row and per group of 32 consecutive columns the rule is the
 * round_scale != 0 rule of deepep_cast_fp8 with 32 in place of 128:
 *   amax = max(max|x|, 1e-4f); v = amax * fp32(1 / 448); e = exponent(v) + (mantissa(v) != 0);
 *   byte = e + 127; q = e4m3fn_rne(fp32(x) * 2^-e)
 * -- the library's own power-of-two rule, a ceiling, so no element saturates; it is not the OCP floor rule (either
 * rule's output is a valid MX operand, only this one is bit-compatible with the per-128 entries).  The scale factors
 * are uint8 [rows][hidden / 32], byte g the biased exponent of column group g; contiguous, they are byte for byte a
 * packed int32 [rows][hidden / 128], and the kernels store them as dwords: a pointer to scale factors, and every row
 * start, is 4-byte aligned.  Every other argument, bound and rejection is the *_ue8m0 sibling's.  Finite bf16 input
 * keeps every byte inside 105..247.
 *
 * deepep_cast_fp8_mx: sf uint8 [num_rows][hidden / 32], contiguous. */
int deepep_cast_fp8_mx(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, uint8_t* sf,
                       deepep_stream_t stream);

/* The inverse: sf uint8 [num_rows][hidden / 32], group g of a row at sf[row * sf_row_stride + g * sf_col_stride]
 * (strides in bytes: a column-major tensor is read in place; with sf_col_stride == 1 the rows are read as dwords and
 * sf_row_stride must be a multiple of 4); out = bf16_rne(fp32(q) * float_from_bits(byte << 23)): byte 0 multiplies
 * by +0.0f (signed zeros), the NaN bytes of q come out NaN, byte 255 is unspecified. */
int deepep_cast_back_fp8_mx(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf, int64_t sf_row_stride,
                            int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_dispatch_pack_cast with the packed row [hidden e4m3fn bytes | hidden / 32 exponent bytes @sf_off | ...]:
 * what deepep_dispatch_pack writes for x_bytes = hidden, sf_bytes = hidden / 32 and the pair of deepep_cast_fp8_mx.
 * The exponent bytes go out as dwords, into peer windows too. */
int deepep_dispatch_pack_cast_mx(const void* x, int64_t x_row_stride_bytes, int hidden, const int64_t* topk_idx,
                                 const float* topk_weights, int num_tokens, int num_topk, int32_t src_base,
                                 const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks, void* packed,
                                 const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows, int sf_off,
                                 int idx_off, int w_off, int src_off, int32_t* error_flag, deepep_stream_t stream);

/* The transposed MXFP8 cast (additive: the ABI version stays): the MXFP8 pair of the TRANSPOSED matrix, for a
 * block-scaled MFMA that contracts over the rows of x (an expert's weight gradient dW = dY^T . X contracts over its
 * tokens, and the instruction takes one E8M0 scale per 32 elements along K).
 *   x     bf16 [num_rows][hidden], rows x_row_stride_bytes apart (>= hidden * 2, a multiple of 16, at most 2^24)
 *   q_t   e4m3fn [hidden][num_rows], contiguous: q_t[c][r] is the byte of x[r][c]
 *   sf_t  uint8 [hidden][num_rows / 32], contiguous: byte g of row c the biased exponent of rows [32g, 32g + 32) of
 *         column c; stored as dwords and, where num_rows % 512 == 0 and sf_t is 16-byte aligned, as 16-byte vectors
 * hidden must be a positive multiple of 128 (at most 2^24), num_rows a multiple of 128 (four groups to a dword; fewer
 * than 2^29).  Per block of 32 consecutive rows and per column the rule is deepep_cast_fp8_mx's, unchanged:
 *   amax = max(max|x[32g .. 32g + 31][c]|, 1e-4f); v = amax * fp32(1 / 448); e = exponent(v) + (mantissa(v) != 0);
 *   sf_t[c][g] = e + 127; q_t[c][32g + r] = e4m3fn_rne(fp32(x[32g + r][c]) * 2^-e)
 * so (q_t, sf_t) is bit for bit what deepep_cast_fp8_mx gives for the transposed, contiguous copy of x, and
 * deepep_cast_back_fp8_mx is its inverse.  No element saturates.  NaN / Inf: unspecified, except that a block's output
 * depends on that block's 32 rows only (uninitialised rows behind the valid ones cannot disturb the valid blocks).
 * q / sf: NULL, or both given: the same launch also writes the row-wise pair of deepep_cast_fp8_mx for x itself
 * (q e4m3fn [num_rows][hidden], sf uint8 [num_rows][hidden / 32], both contiguous; q 16-byte, sf 4-byte aligned),
 * bit for bit, from the same single read of x.
 * One launch on `stream`, no workspace, no host synchronisation.  num_rows == 0 returns DEEPEP_OK without a launch;
 * bad arguments return DEEPEP_ERR_INVALID_ARG with text and launch nothing.  x and q_t must be 16-byte aligned, sf_t
 * 4-byte aligned.  Every index is 64-bit; inside one tile of 128 x 128 the kernel uses 32-bit offsets, hence the
 * bounds above. */
int deepep_cast_fp8_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream);

/* MXFP4: OCP e2m1 rows with one UE8M0 exponent byte per 32 columns, the FP4 operand of the same block-scaled MFMA
 * (additive: the ABI version stays).  hidden must be a positive multiple of 128.  A row is the pair
 *   rows           uint8 [rows][hidden / 2]: byte j holds column 2j in bits 3:0 and column 2j + 1 in bits 7:4
 *                  (torch.float4_e2m1fn_x2).  A code is s eem: bit 3 the sign, magnitudes 0..7 = 0, 0.5, 1, 1.5, 2, 3,
 *                  4, 6
 *   scale factors  uint8 [rows][hidden / 32], byte g the biased exponent of column group g: the MXFP8 tensor, stored
 *                  as dwords (a pointer to scale factors, and every row start, is 4-byte aligned)
 * The cast, per row and per group of 32 consecutive columns, is the MXFP8 rule with 6 in place of 448 (the power-of-two
 * ceiling, not the OCP floor rule):
 *   amax = max(max|x|, 1e-4f); v = amax * fp32(1 / 6); e = exponent(v) + (mantissa(v) != 0); byte = e + 127;
 *   code = sign(x) | e2m1_rne(|fp32(x)| * 2^-e)
 * e2m1_rne rounds to the nearest magnitude, ties to the even code: m <= 0.25: 0; 0.25 < m < 0.75: 1;
 * 0.75 <= m <= 1.25: 2; 1.25 < m < 1.75: 3; 1.75 <= m <= 2.5: 4; 2.5 < m < 3.5: 5; 3.5 <= m <= 5: 6; m > 5: 7.  The
 * sign bit of x is always kept (-0.0, and a negative value that rounds to zero: code 0x8).  Finite bf16 input keeps
 * every byte inside 112..253 and the scaled amax inside (3, 6]: nothing saturates.  NaN / Inf: unspecified.
 * The arguments, bounds and rejections are the *_mx (MXFP8) siblings', with rows of hidden / 2 bytes where those have
 * hidden; every entry returns DEEPEP_OK for zero rows.
 *
 * deepep_cast_fp4_mx: x bf16 [num_rows][hidden] (x_row_stride_bytes >= hidden * 2, a multiple of 16) ->
 * q uint8 [num_rows][hidden / 2] and sf uint8 [num_rows][hidden / 32], both contiguous. */
int deepep_cast_fp4_mx(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, uint8_t* sf,
                       deepep_stream_t stream);

/* The inverse: q rows q_row_stride_bytes apart (>= hidden / 2, a multiple of 16); group g of a row at
 * sf[row * sf_row_stride + g * sf_col_stride] (strides in bytes: a column-major tensor is read in place; with
 * sf_col_stride == 1 the rows are read as dwords and sf_row_stride must be a multiple of 4);
 * out bf16 [num_rows][hidden], contiguous = bf16_rne(fp32(code) * float_from_bits(byte << 23)): byte 0 multiplies by
 * +0.0f (signed zeros). */
int deepep_cast_back_fp4_mx(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf, int64_t sf_row_stride,
                            int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_dispatch_pack_cast_mx with the packed row [hidden / 2 codes | hidden / 32 exponent bytes @sf_off | ...]
 * (sf_off >= hidden / 2): what deepep_dispatch_pack writes for x_bytes = hidden / 2, sf_bytes = hidden / 32 and the
 * pair of deepep_cast_fp4_mx.  The exponent bytes go out as dwords, into peer windows too. */
int deepep_dispatch_pack_cast_fp4_mx(const void* x, int64_t x_row_stride_bytes, int hidden, const int64_t* topk_idx,
                                     const float* topk_weights, int num_tokens, int num_topk, int32_t src_base,
                                     const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks, void* packed,
                                     const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows, int sf_off,
                                     int idx_off, int w_off, int src_off, int32_t* error_flag,
                                     deepep_stream_t stream);

/* MXFP6: OCP e2m3 rows with one UE8M0 exponent byte per 32 columns, the FP6 operand of the same block-scaled MFMA,
 * which runs it at the FP4 rate (additive: the ABI version stays).  hidden must be a positive multiple of 128.  A row
 * is the pair
 *   rows           uint8 [rows][3 * hidden / 4].  A group of 32 columns is 24 bytes, group g at bytes
 *                  [24g, 24g + 24) of the row, read as a little-endian 192-bit string: column c of the group sits in
 *                  bits 6c + 5 : 6c.  Equivalently, columns 4j .. 4j + 3 are the 24-bit little-endian word
 *                  c0 | c1 << 6 | c2 << 12 | c3 << 18 in bytes 3j .. 3j + 2.  This is the order in which
 *                  v_cvt_scalef32_pk32_fp6_bf16 leaves the 32 codes in its six registers and in which
 *                  v_cvt_scalef32_pk32_f32_fp6 reads them (both read off the MI355X; the kernels use them).  There is
 *                  no torch dtype for it.  A code is s ee mmm: bit 5 the sign; ee == 0: magnitude mmm / 8; otherwise
 *                  (1 + mmm / 8) * 2^(ee - 1); the largest magnitude is 7.5.  (E3M2 is not produced.)
 *   scale factors  uint8 [rows][hidden / 32], byte g the biased exponent of column group g: the MXFP8 / MXFP4 tensor,
 *                  stored as dwords (a pointer to scale factors, and every row start, is 4-byte aligned)
 * The cast, per row and per group of 32 consecutive columns, is the MXFP8 rule with 7.5 in place of 448 (the
 * power-of-two ceiling, not the OCP floor rule):
 *   amax = max(max|x|, 1e-4f); v = amax * fp32(1 / 7.5); e = exponent(v) + (mantissa(v) != 0); byte = e + 127;
 *   code = sign(x) | e2m3_rne(|fp32(x)| * 2^-e)
 * e2m3_rne rounds to the nearest of the 32 magnitudes, ties to the even code: the 31 tie points are the midpoints of
 * neighbouring magnitudes (0.0625 -> 0, 0.1875 -> 0.25, 0.3125 -> 0.25, ..., 6.75 -> 7, 7.25 -> 7).  The sign bit of x
 * is always kept (-0.0, and a negative value that rounds to zero: code 0x20).  Finite bf16 input keeps every byte
 * inside 111..253 and the scaled amax inside (3.75, 7.5]: nothing saturates.  NaN / Inf: unspecified.
 * The arguments, bounds and rejections are the *_fp4_mx siblings', with rows of 3 * hidden / 4 bytes where those have
 * hidden / 2; every entry returns DEEPEP_OK for zero rows.
 *
 * deepep_cast_fp6_mx: x bf16 [num_rows][hidden] (x_row_stride_bytes >= hidden * 2, a multiple of 16) ->
 * q uint8 [num_rows][3 * hidden / 4] and sf uint8 [num_rows][hidden / 32], both contiguous. */
int deepep_cast_fp6_mx(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q, uint8_t* sf,
                       deepep_stream_t stream);

/* deepep_cast_fp6_mx with the width of its row stores chosen, for measurements: store_bytes 16 (a lane pair's 48
 * bytes as three 16-byte stores after a two-dword exchange) or 8 (three 8-byte stores a lane).  The bytes written are
 * the same; deepep_cast_fp6_mx runs the form measured faster. */
int deepep_cast_fp6_mx_stores(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* q,
                              uint8_t* sf, int store_bytes, deepep_stream_t stream);

/* The inverse: q rows q_row_stride_bytes apart (>= 3 * hidden / 4, a multiple of 16); group g of a row at
 * sf[row * sf_row_stride + g * sf_col_stride] (strides in bytes: a column-major tensor is read in place; with
 * sf_col_stride == 1 the rows are read as dwords and sf_row_stride must be a multiple of 4);
 * out bf16 [num_rows][hidden], contiguous = bf16_rne(fp32(code) * float_from_bits(byte << 23)): byte 0 multiplies by
 * +0.0f (signed zeros).  The factor is applied by an fp32 multiply, not by the conversion's scale operand. */
int deepep_cast_back_fp6_mx(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf, int64_t sf_row_stride,
                            int64_t sf_col_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_dispatch_pack_cast_fp4_mx with the packed row [3 * hidden / 4 codes | hidden / 32 exponent bytes @sf_off |
 * ...] (sf_off >= 3 * hidden / 4): what deepep_dispatch_pack writes for x_bytes = 3 * hidden / 4,
 * sf_bytes = hidden / 32 and the pair of deepep_cast_fp6_mx.  The codes go out as 16-byte stores, the exponent bytes
 * as dwords, into peer windows too. */
int deepep_dispatch_pack_cast_fp6_mx(const void* x, int64_t x_row_stride_bytes, int hidden, const int64_t* topk_idx,
                                     const float* topk_weights, int num_tokens, int num_topk, int32_t src_base,
                                     const int32_t* dst_slot, const int32_t* send_offsets, int num_ranks, void* packed,
                                     const uint64_t* dest_bases, int64_t row_bytes, int64_t dest_rows, int sf_off,
                                     int idx_off, int w_off, int src_off, int32_t* error_flag,
                                     deepep_stream_t stream);

/* Receive-side block: DEEPEP_DISPATCH_BLOCK_ROWS consecutive received rows. */
#define DEEPEP_DISPATCH_BLOCK_ROWS 128

/* Receive side, pass 1: src_metadata columns 0-1 ({src_global_idx, src_rank * K + master lane}),
 * recv_topk_idx (local expert or -1, int64 [num_recv][K], may be NULL) and per-block expert
 * histograms block_counts [ceil(num_recv / DEEPEP_DISPATCH_BLOCK_ROWS)][num_local_experts]. recv_counts_stride
 * 0: recv_rank_psum is the inclusive prefix sum of rows per source rank (device memory);
 * recv_counts_stride > 0: recv_rank_psum[s * recv_counts_stride] is the row count of source rank s (the
 * notify records' first column) and the prefix sum is formed here, and written to psum_out (int32
 * [num_ranks], may be NULL).  num_ranks <= 64.  Rows from the last prefix sum
 * up to num_recv (a launch sized for the worst case, dispatch(do_cpu_sync=False)) get src_metadata
 * columns 0-1 = -1 and recv_topk_idx -1; passes 3 and 4 skip them.
 * pad_rows > 0: the packed rows come from a worst-case-sized exchange, source s's rows at s * pad_rows
 * (not contiguous); row_map (int32 [num_recv]) then receives the packed row of every received row i,
 * which passes 3 and 4 take as their row_map.  own_first (the local bypass): packed = [rows from `rank`
 * itself | rows from the other sources in rank order] -- the sender packed its own rows straight behind
 * its send rows, so they never enter the all-to-all -- and row_map is written the same way; with pad_rows
 * the padded slots are in that order too (`rank`'s at 0, source s < rank at (s + 1) * pad_rows, s > rank at
 * s * pad_rows).  Neither: packed row i is row i (row_map may be NULL). */
int deepep_dispatch_count(const void* packed, int64_t row_bytes, int idx_off, int src_off, int num_recv, int num_topk,
                          int rank, int num_local_experts, const int32_t* recv_rank_psum, int num_ranks,
                          int recv_counts_stride, int32_t* psum_out, int pad_rows, int own_first, int32_t* row_map,
                          int32_t* src_metadata, int64_t* recv_topk_idx, int32_t* block_counts,
                          deepep_stream_t stream);

/* Passes 1-3 in one call (the launches back to back, no host work between them): deepep_dispatch_count in
 * counts mode (recv_counts_stride >= 1, psum_out required), deepep_dispatch_scan, and -- expanded -- the
 * slots pass (inv optional); non-expanded, src_metadata columns 2.. are set to -1. */
int deepep_dispatch_receive(const void* packed, int64_t row_bytes, int idx_off, int src_off, int num_recv,
                            int num_topk, int rank, int num_local_experts, const int32_t* recv_counts,
                            int num_ranks, int recv_counts_stride, int32_t* psum_out, int pad_rows, int own_first,
                            int32_t* row_map,
                            int32_t* src_metadata, int64_t* recv_topk_idx, int32_t* block_counts,
                            int expert_alignment, int expanded, int32_t* expert_counts, int32_t* psum_expert,
                            int32_t* inv, deepep_stream_t stream);

/* Pass 2: block_counts becomes each block's first slot inside its expert group (expert
 * groups start at aligned offsets); expert_counts = rows per expert; psum_expert as the reference
 * handle's psum_num_recv_tokens_per_expert (expanded: aligned start + count; else inclusive aligned). */
int deepep_dispatch_scan(int32_t* block_counts, int num_blocks, int num_local_experts, int expert_alignment,
                         int expanded, int32_t* expert_counts, int32_t* psum_expert, deepep_stream_t stream);

/* Pass 3 (expanded only): src_metadata columns 2.. = expanded row of every local slot, -1 elsewhere
 * (all -1 for a row whose column 0 is -1).  inv (int32 [expanded rows], or NULL): the inverse map,
 * inv[slot] = row * num_topk + lane for every slot written (alignment padding rows are not written). */
int deepep_dispatch_slots(const void* packed, int64_t row_bytes, int idx_off, int num_recv, int num_topk,
                          int rank, int num_local_experts, const int32_t* block_offsets, int32_t* src_metadata,
                          int32_t* inv, const int32_t* row_map, deepep_stream_t stream);

/* Pass 4: recv_x / recv_sf rows (row i, or every local slot when expanded) and top-k weights
 * ([num_recv][K] or, expanded, [slot]).  recv_sf / recv_topk_weights may be NULL.  With x_direct
 * (one rank: nothing was exchanged, the packed rows carry only metadata) the x / sf bytes of row i
 * are read from x_direct / sf_direct at row src_metadata[i][0] % num_max_tokens.  Destination rows
 * >= num_out_rows (the rows recv_x holds) are skipped and set bit 1 of error_flag (device int or
 * NULL); once bit 2 is set (a timed-out window barrier) nothing is stored.  Rows whose
 * src_metadata[i][0] is -1 (past the received rows, pass 1) are skipped.
 * inv (expanded only, or NULL): pass 3's inverse map; then the copy runs destination-major inside
 * blocks of received rows -- expert e's rows of block b are [block_offsets[b][e], block_offsets[b+1][e])
 * (pass 2's offsets; the last block ends at expert_end[e], pass 2's psum_expert) -- each block owned
 * by one XCD, whose L2 serves its rows' re-reads.  Same bytes as with inv NULL
 * (source-major: one load of each received row, a store per local slot). */
int deepep_dispatch_copy(const void* packed, int64_t row_bytes, int x_bytes, int sf_off, int sf_bytes, int w_off,
                         int num_recv, int num_topk, const int32_t* src_metadata, int expanded,
                         const void* x_direct, int64_t x_direct_stride_bytes,
                         const void* sf_direct, int64_t sf_direct_stride_bytes, int num_max_tokens,
                         void* recv_x, void* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                         const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                         int num_local_experts, const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream);

/* Pass 4 at one rank with the cast of deepep_cast_fp8 on the way: the x_direct forms of deepep_dispatch_copy
 * for a bf16 source.  x is the sender's bf16 rows [tokens][hidden] (rows x_row_stride_bytes apart); received
 * row i's source is row src_metadata[i][0] % num_max_tokens of x, read as bf16 and quantised in registers;
 * recv_x gets the e4m3fn rows [num_out_rows][hidden], recv_sf (required) the scale factors
 * [num_out_rows][hidden / 128], recv_topk_weights (or NULL) the weights from the packed rows' w_off -- what
 * deepep_dispatch_copy writes for x_direct / sf_direct = the cast pair of x.  expanded, inv, block_offsets,
 * expert_end, num_local_experts, row_map, num_out_rows and error_flag as deepep_dispatch_copy (with inv the
 * blocked destination-major copy: a source row is re-read and re-quantised once per local expert).  packed is
 * read only for the weights.  hidden % 128 != 0, a null or misaligned x / recv_x / recv_sf, a row stride below
 * hidden * 2 or not a multiple of 16 are rejected; num_recv == 0 is a no-op. */
int deepep_dispatch_copy_cast(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                              const int32_t* src_metadata, int expanded, const void* x, int64_t x_row_stride_bytes,
                              int hidden, int round_scale, int num_max_tokens, void* recv_x, float* recv_sf,
                              float* recv_topk_weights, int64_t num_out_rows, const int32_t* inv,
                              const int32_t* block_offsets, const int32_t* expert_end, int num_local_experts,
                              const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream);

/* deepep_dispatch_copy_cast(round_scale = 1) with packed UE8M0 scale factors (see deepep_cast_fp8_ue8m0): recv_sf
 * int32 [num_out_rows][hidden / 512] -- what deepep_dispatch_copy writes for x_direct / sf_direct = the pair of
 * deepep_cast_fp8_ue8m0.  The num_out_rows bound covers the scale-factor stores as it covers the row stores. */
int deepep_dispatch_copy_cast_ue8m0(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                    const int32_t* src_metadata, int expanded, const void* x,
                                    int64_t x_row_stride_bytes, int hidden, int num_max_tokens, void* recv_x,
                                    int32_t* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                                    const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                                    int num_local_experts, const int32_t* row_map, int32_t* error_flag,
                                    deepep_stream_t stream);

/* deepep_dispatch_copy_cast as MXFP8 (see deepep_cast_fp8_mx): recv_sf uint8 [num_out_rows][hidden / 32], written as
 * dwords -- what deepep_dispatch_copy writes for x_direct / sf_direct = the pair of deepep_cast_fp8_mx.  The
 * num_out_rows bound covers the scale-factor stores as it covers the row stores. */
int deepep_dispatch_copy_cast_mx(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                 const int32_t* src_metadata, int expanded, const void* x, int64_t x_row_stride_bytes,
                                 int hidden, int num_max_tokens, void* recv_x, uint8_t* recv_sf,
                                 float* recv_topk_weights, int64_t num_out_rows, const int32_t* inv,
                                 const int32_t* block_offsets, const int32_t* expert_end, int num_local_experts,
                                 const int32_t* row_map, int32_t* error_flag, deepep_stream_t stream);

/* deepep_dispatch_copy_cast_mx as MXFP4 (see deepep_cast_fp4_mx): recv_x uint8 [num_out_rows][hidden / 2], recv_sf
 * uint8 [num_out_rows][hidden / 32], written as dwords -- what deepep_dispatch_copy writes for x_direct / sf_direct =
 * the pair of deepep_cast_fp4_mx.  The num_out_rows bound covers the scale-factor stores as it covers the row
 * stores. */
int deepep_dispatch_copy_cast_fp4_mx(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                     const int32_t* src_metadata, int expanded, const void* x,
                                     int64_t x_row_stride_bytes, int hidden, int num_max_tokens, void* recv_x,
                                     uint8_t* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                                     const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                                     int num_local_experts, const int32_t* row_map, int32_t* error_flag,
                                     deepep_stream_t stream);

/* deepep_dispatch_copy_cast_fp4_mx as MXFP6 (see deepep_cast_fp6_mx): recv_x uint8 [num_out_rows][3 * hidden / 4],
 * recv_sf uint8 [num_out_rows][hidden / 32], written as dwords -- what deepep_dispatch_copy writes for x_direct /
 * sf_direct = the pair of deepep_cast_fp6_mx.  The num_out_rows bound covers the scale-factor stores as it covers the
 * row stores. */
int deepep_dispatch_copy_cast_fp6_mx(const void* packed, int64_t row_bytes, int w_off, int num_recv, int num_topk,
                                     const int32_t* src_metadata, int expanded, const void* x,
                                     int64_t x_row_stride_bytes, int hidden, int num_max_tokens, void* recv_x,
                                     uint8_t* recv_sf, float* recv_topk_weights, int64_t num_out_rows,
                                     const int32_t* inv, const int32_t* block_offsets, const int32_t* expert_end,
                                     int num_local_experts, const int32_t* row_map, int32_t* error_flag,
                                     deepep_stream_t stream);

/* The transposed MXFP4 and MXFP6 casts (additive: the ABI version stays): the pair of deepep_cast_fp4_mx /
 * deepep_cast_fp6_mx of the TRANSPOSED matrix, the FP4 / FP6 operand of a block-scaled MFMA that contracts over the
 * rows of x (an expert's weight gradient).  The argument list, the types, the checks and the bounds are those of
 * deepep_cast_fp8_mx_transposed; only the element type of q_t and q differs.
 *   x     bf16 [num_rows][hidden], rows x_row_stride_bytes apart (>= hidden * 2, a multiple of 16, at most 2^24)
 *   q_t   FP4: uint8 [hidden][num_rows / 2], contiguous: byte j of row c holds the e2m1 code of x[2j][c] in bits 3:0
 *         and of x[2j + 1][c] in bits 7:4.
 *         FP6: uint8 [hidden][3 * num_rows / 4], contiguous: block g of 32 rows of x is bytes [24g, 24g + 24) of row
 *         c, a little-endian 192-bit string with the e2m3 code of x[32g + r][c] in bits 6r + 5 : 6r
 *   sf_t  uint8 [hidden][num_rows / 32], contiguous: byte g of row c the biased exponent of rows [32g, 32g + 32) of
 *         column c; stored as dwords and, where num_rows % 512 == 0 and sf_t is 16-byte aligned, as 16-byte vectors
 * hidden must be a positive multiple of 128 (at most 2^24), num_rows a multiple of 128 (fewer than 2^29).  Per block
 * of 32 consecutive rows and per column the rule, the codes, the tie rule and the sign rule are deepep_cast_fp4_mx's /
 * deepep_cast_fp6_mx's, unchanged (the ceiling rule with 6 / 7.5; the sign of x is always kept), so (q_t, sf_t) is bit
 * for bit what that entry gives for the transposed, contiguous copy of x, and deepep_cast_back_fp4_mx /
 * deepep_cast_back_fp6_mx is its inverse.  NaN / Inf: unspecified, except that a block's output depends on that
 * block's 32 rows only.
 * q / sf: NULL, or both given: the same launch also writes the row-wise pair of deepep_cast_fp4_mx / deepep_cast_fp6_mx
 * for x itself (q uint8 [num_rows][hidden / 2] or [num_rows][3 * hidden / 4], sf uint8 [num_rows][hidden / 32], both
 * contiguous; q 16-byte, sf 4-byte aligned), bit for bit, from the same single read of x.
 * One launch on `stream`, no workspace, no host synchronisation.  num_rows == 0 returns DEEPEP_OK without a launch;
 * bad arguments return DEEPEP_ERR_INVALID_ARG with text and launch nothing.  x and q_t must be 16-byte aligned, sf_t
 * 4-byte aligned.  Every index is 64-bit; inside one tile of 128 x 128 the kernel addresses x, q and sf through 32-bit
 * offsets, hence the bounds above. */
int deepep_cast_fp4_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream);
int deepep_cast_fp6_mx_transposed(const void* x, int64_t x_row_stride_bytes, void* q_t, uint8_t* sf_t, void* q,
                                  uint8_t* sf, int num_rows, int hidden, deepep_stream_t stream);

/* Requantisation along the tokens (additive: the ABI version stays): a row-wise quantised pair -- what a casting
 * dispatch returns -- becomes the operand of deepep_cast_fp8_mx_transposed / deepep_cast_fp4_mx_transposed /
 * deepep_cast_fp6_mx_transposed in one read of the pair, without the bf16 [num_rows][hidden] buffer between.  The
 * contract is one rule: (q_t, sf_t) is bit for bit what that transposed cast gives for the rows that
 * deepep_cast_back_fp8{,_ue8m0,_mx} / deepep_cast_back_fp4_mx / deepep_cast_back_fp6_mx gives for (q, sf).  Every
 * element is cast back as there -- exact code -> fp32, one fp32 multiply by its group's factor, one round to nearest
 * even to bf16 (the rounding is part of the contract) -- and the bf16 values go through the token-axis rule unchanged.
 *   q     FP8: e4m3fn [num_rows][hidden]; FP4: uint8 [num_rows][hidden / 2]; FP6: uint8 [num_rows][3 * hidden / 4]
 *         (the formats of deepep_cast_fp8 / deepep_cast_fp4_mx / deepep_cast_fp6_mx); rows q_row_stride_bytes apart
 *         (>= a row's bytes, a multiple of 16, at most 2^24)
 *   sf    the scale factors along hidden, element (r, j) at sf[r * sf_row_stride + j * sf_col_stride]: the strides
 *         count elements and are not negative (a column-major tensor is read in place)
 *         FP8, by sf_form:  DEEPEP_SF_FORM_FP32          float    [num_rows][hidden / 128]
 *                           DEEPEP_SF_FORM_UE8M0_PACKED  uint32_t [num_rows][hidden / 512], hidden % 512 == 0: byte j
 *                                                        of element p the exponent byte of column group 4p + j
 *                           DEEPEP_SF_FORM_MX            uint8_t  [num_rows][hidden / 32]
 *         FP4, FP6:         uint8_t [num_rows][hidden / 32]
 *         an exponent byte b is the factor float_from_bits(b << 23): byte 0 is +0.0f, so the padding rows of a casting
 *         dispatch (zero codes, zero bytes) are zero rows, as in the composition
 *   q_t, sf_t   as the transposed cast of the element type writes them (contiguous; sf_t stored as dwords and, where
 *         num_rows % 512 == 0 and sf_t is 16-byte aligned, as 16-byte vectors)
 * hidden must be a positive multiple of 128 (at most 2^24), num_rows a multiple of 128 (fewer than 2^29).  NaN codes and
 * NaN factors: unspecified, except that a block's output depends on that block's 32 rows only.
 * One launch on `stream`, no workspace, no host synchronisation.  num_rows == 0 returns DEEPEP_OK without a launch;
 * bad arguments return DEEPEP_ERR_INVALID_ARG with text and launch nothing.  q and q_t must be 16-byte aligned, sf_t
 * and float / uint32_t scale factors 4-byte aligned.  Every index is 64-bit; inside one tile of 128 x 128 the kernel
 * addresses q and q_t through 32-bit offsets, hence the bounds above. */
#define DEEPEP_SF_FORM_FP32          0
#define DEEPEP_SF_FORM_UE8M0_PACKED  1
#define DEEPEP_SF_FORM_MX            2
int deepep_requant_fp8_mx_transposed(const void* q, int64_t q_row_stride_bytes, const void* sf, int64_t sf_row_stride,
                                     int64_t sf_col_stride, int sf_form, void* q_t, uint8_t* sf_t, int num_rows,
                                     int hidden, deepep_stream_t stream);
int deepep_requant_fp4_mx_transposed(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf,
                                     int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t,
                                     int num_rows, int hidden, deepep_stream_t stream);
int deepep_requant_fp6_mx_transposed(const void* q, int64_t q_row_stride_bytes, const uint8_t* sf,
                                     int64_t sf_row_stride, int64_t sf_col_stride, void* q_t, uint8_t* sf_t,
                                     int num_rows, int hidden, deepep_stream_t stream);

/* ------------------------------------------------------------------ EP > 1 combine plan
 * The EP > 1 combine runs in pipeline chunks of source tokens: chunk c = tokens
 * [c * B, (c + 1) * B) of every rank, B = blocks_per_chunk * DEEPEP_PLAN_BLOCK_TOKENS.  Phase A on an
 * expert rank reduces the chunk's received rows into partials; they travel to their source ranks
 * (RCCL all-to-all of the chunk's rows grouped by source rank, or xGMI stores into the source rank's
 * window); phase B on the source rank reduces each token's partials.  These three calls build every
 * table of that schedule on the device from the dispatch's counts, so a first combine needs no host
 * synchronisation.  Counts are per block of DEEPEP_PLAN_BLOCK_TOKENS consecutive tokens of a source
 * rank, int32 [num_ranks][num_blocks] (num_blocks >= ceil(num_max_tokens / 64)).
 */
#define DEEPEP_PLAN_BLOCK_TOKENS 64
#define DEEPEP_PLAN_EXPANDED     1    /* x is the expanded layout (metadata columns 2.. are rows)       */
#define DEEPEP_PLAN_SINGLE       2    /* single reduction: every valid (row, lane) travels unreduced     */
#define DEEPEP_PLAN_INTERLEAVE   4    /* phase-A units round-robin over source ranks (xGMI stores)      */
#define DEEPEP_PLAN_RANK_LAYOUT  8    /* receive slot = expert rank (R <= K), else the master lane        */
#define DEEPEP_PLAN_WINDOW      16    /* source side: rows are window rows slot * T_max + t               */
#define DEEPEP_PLAN_LOCAL_BYPASS 32   /* RCCL exchange without the own-rank diagonal (below)              */

/* Sender side of the notify: tok_counts[r][b] = tokens of block b routed to rank r, pair_counts[r][b] =
 * (token, lane) entries of block b routed to r (blocks past num_tokens are zero). */
int deepep_route_block_counts(const int64_t* topk_idx, int num_tokens, int num_topk, int num_experts, int num_ranks,
                              int num_blocks, int32_t* tok_counts, int32_t* pair_counts, deepep_stream_t stream);

/* Expert side: phase-A units of every chunk, concatenated in chunk order.  recv_tok / recv_pairs are
 * the counts received from every source rank (rows received per source block).  Inside a chunk, units
 * are grouped by source rank (the send buffer of an all-to-all), or round-robin over the source ranks
 * with DEEPEP_PLAN_INTERLEAVE.  Multiple reduction: one unit per received row i; table_a[u] = the
 * metadata slots of i (expanded, K wide) or i (1 wide), wtable_a[u][k] = i * K + k (non-expanded,
 * may be NULL).  Single reduction: one unit per valid (row, lane) in (row, lane) order, table_a[u] =
 * the expanded row (1 wide).  out_rows (optional, the xGMI transport): byte address of unit u's row,
 * window_bases[src_rank] + (slot * num_max_tokens + src_token) * window_row_bytes, slot = rank (rank
 * layout) or the master lane (multiple reduction), the lane (single reduction) -- combine.cuh:96-106.
 * Bounds: a received row index >= num_recv (src_metadata rows) or a unit position past its chunk's unit
 * count (counts that disagree with the metadata) writes nothing for that unit (DEEPEP_FAULT_PLAN_UNIT);
 * a window row whose bytes do not lie inside [0, window_bytes) of its window, or metadata no correct
 * dispatch produces, gives out_rows[u] = 0 (DEEPEP_FAULT_PLAN_ROW), which the scatter skips.  Callers
 * pre-fill table_a / wtable_a with -1 and out_rows with 0, so an unwritten unit is never an address.
 * error_flag: DEEPEP_ERROR_RECORD_INTS device ints or NULL (bit 1 and the record are set on a fault).
 * padded_stride > 0 (a handle whose counts only the device knows: dispatch without a CPU sync): chunk c
 * holds num_ranks * padded_stride unit positions starting at c * num_ranks * padded_stride; unit p of
 * source s sits at s * padded_stride + p (or p * num_ranks + s with DEEPEP_PLAN_INTERLEAVE).  The positions
 * no unit takes keep the caller's fill: -1 slots (a zero partial) and, for out_rows, the value 1, which
 * the scatter skips silently.  A unit p >= padded_stride of its source (more (token, lane) pairs on this
 * rank than the padding allows) is rejected like a unit past its chunk, so it never lands in another
 * source's positions.
 * DEEPEP_PLAN_LOCAL_BYPASS (grouped order only): inside every chunk the groups follow the ranks in order
 * except this rank's, which comes last -- [units of the other sources, rank order | units of `rank`] -- so
 * the first part is an all-to-all input whose split for `rank` is 0 and the own units can be written
 * straight into the receive rows deepep_plan_source lays out with the same flag (the reference's own
 * receive slot is local memory, combine.cuh:96-101). */
int deepep_plan_expert(const int32_t* src_metadata, int num_recv, int num_topk, int num_ranks, int rank,
                       int num_max_tokens, const int32_t* recv_tok, const int32_t* recv_pairs, int num_blocks,
                       int blocks_per_chunk, int flags, int32_t* table_a, int32_t* wtable_a,
                       const uint64_t* window_bases, int64_t window_row_bytes, int64_t window_bytes,
                       uint64_t* out_rows, int32_t* error_flag, int padded_stride, deepep_stream_t stream);

/* Source side, per owned token t (chunk c = t / B).  Multiple reduction: table_b [T][min(R, K)] = the
 * rows of t's partials in ascending dedup-master-lane order (a rank's master is its highest top-k
 * lane; combine_reduce_epilogue.cuh:74-95), then -1; wtable [T][K] (or NULL) = row(rank of lane k) *
 * row_floats + weights_offset + k, or -1: the float index of lane k's weight in the packed receive rows.
 * A row is the partial's row in chunk c's receive buffer (grouped by expert rank, ascending token:
 * dst_slot [T][R] from deepep_dispatch_route gives the rank among earlier tokens) or, with
 * DEEPEP_PLAN_WINDOW, the window row slot * num_max_tokens + t.  Single reduction: table_b [T][K] = the
 * row of (t, k): receive-buffer order (expert rank, then (token, lane)) or window row k * T_max + t.
 * padded_stride > 0 (not with DEEPEP_PLAN_WINDOW): the receive buffer of a chunk is worst-case padded,
 * expert rank d's rows from d * padded_stride (the plan_expert layout above, after the exchange); a row
 * past d's padded_stride rows (a unit plan_expert rejects) is -1.
 * DEEPEP_PLAN_LOCAL_BYPASS (not with DEEPEP_PLAN_WINDOW): the chunk's receive rows are [rows from `rank`
 * (phase A's own units, written in place) | rows received from the other ranks, rank order], i.e. the
 * rows of `rank` come first. */
int deepep_plan_source(const int64_t* topk_idx, int num_tokens, int num_topk, int num_experts, int num_ranks,
                       int rank, int num_max_tokens, const int32_t* dst_slot, const int32_t* send_tok,
                       const int32_t* send_pairs, int num_blocks, int blocks_per_chunk, int flags,
                       int64_t row_floats, int64_t weights_offset, int32_t* table_b, int table_b_width,
                       int32_t* wtable, int padded_stride, deepep_stream_t stream);

/* ------------------------------------------------------------------ symmetric buffer over xGMI
 * Replaces the reference's NCCLSymmetricMemoryContext (csrc/elastic/nccl.cu:62-153, buffer.hpp:181-208)
 * and its device barrier (deep_ep/include/deep_ep/common/comm.cuh:88-129).  One uncached device
 * allocation per rank, exported/imported with HIP IPC; kernels on any rank load/store a peer's
 * window over xGMI. */
#define DEEPEP_IPC_HANDLE_BYTES 64

int deepep_sym_alloc(int64_t bytes, void** ptr);            /* zero-filled, hipDeviceMallocUncached */
int deepep_sym_free(void* ptr);
int deepep_sym_export(void* ptr, void* handle);             /* handle: DEEPEP_IPC_HANDLE_BYTES bytes */
int deepep_sym_import(const void* handle, void** ptr);      /* a peer's window, mapped into this process */
int deepep_sym_close(void* ptr);

/* Window header, DEEPEP_SYM_HEADER_BYTES from the window base (zero at allocation): the int64 flag
 * table [DEEPEP_SYM_FLAG_SLOTS][64], then int64 counters [3][DEEPEP_SYM_FLAG_SLOTS] (publishes, waits,
 * workgroup arrivals), then from DEEPEP_SYM_NOTIFY_OFFSET the notify area the dispatch's counts are
 * exchanged through (deepep_sym_put); the data region starts at DEEPEP_SYM_HEADER_BYTES. */
#define DEEPEP_SYM_NOTIFY_OFFSET 65536
#define DEEPEP_SYM_HEADER_BYTES 1048576

/* Store src + d * bytes (bytes % 16 == 0) at dest_bases[d] + dest_offset for every d < num_ranks:
 * system-scope write-through stores into the peers' windows (dest_bases: device uint64 [num_ranks],
 * e.g. the window bases, so dest_offset addresses the header's notify area).  dest_extent: the bytes
 * every destination window spans from its base (header + data); a put whose [dest_offset, dest_offset
 * + bytes) does not lie inside it is rejected (DEEPEP_ERR_INVALID_ARG) before anything is launched.
 * The dispatch notify's transport: rank r puts its count record for every destination into slot r of
 * that destination's area, then a barrier makes them visible (dispatch.cuh:79-258's notify over
 * NVLink).  Nothing is stored once bit 2 of error_flag (device int or NULL) is set. */
int deepep_sym_put(const void* src, int64_t bytes, const uint64_t* dest_bases, int num_ranks, int64_t dest_offset,
                   int64_t dest_extent, const int32_t* error_flag, deepep_stream_t stream);

/* Group barrier on the stream: peer_flags (device, uint64 [num_ranks]) holds the address of every
 * rank's window header (above).  Every XCD's L2 is first written back (the stores into peer windows before
 * the call may sit in any of them).  Rank r then stores
 * the epoch into entry [r] of slot 0 of every rank's table (system-scope release) and waits until
 * its own entries all reach it (system-scope acquire).  epoch <= 0: the next epoch is counted on
 * the device (this rank's counter), so a captured HIP graph replays with fresh epochs -- use it
 * for every call of a window, or host epochs (growing by one per call) for every call, not both.
 * After timeout_us (<= 0: 100 s) the wait gives up and sets bit 2 of *error_flag (comm.cuh:30-54
 * traps instead). */
int deepep_sym_barrier(const uint64_t* peer_flags, int rank, int num_ranks, int64_t epoch, int64_t timeout_us,
                       int32_t* error_flag, deepep_stream_t stream);

/* Split barrier for pipelined phases, on flag slot 1 <= slot < DEEPEP_SYM_FLAG_SLOTS of the same
 * tables (slot 0 is deepep_sym_barrier's): deepep_sym_signal stores `value` into slot `slot`, entry
 * [rank], of every rank's table after the stream's earlier work (system-scope release);
 * deepep_sym_wait waits until every entry of slot `slot` of this rank's table reaches `value`
 * (timeout as deepep_sym_barrier).  value <= 0: counted on the device, signals and waits each
 * with their own per-slot counter (the n-th wait of a slot waits for every rank's n-th signal). */
#define DEEPEP_SYM_FLAG_SLOTS 64
int deepep_sym_signal(const uint64_t* peer_flags, int rank, int num_ranks, int slot, int64_t value,
                      deepep_stream_t stream);
int deepep_sym_wait(const uint64_t* peer_flags, int rank, int num_ranks, int slot, int64_t value, int64_t timeout_us,
                    int32_t* error_flag, deepep_stream_t stream);

/* Phase A writing straight into the owners' receive rows (combine_impl's NVLink push,
 * combine.cuh:96-106, 125-176, 215-226): the reduce of deepep_combine_reduce(DEEPEP_MODE_LOCAL, ...)
 * with unit u's bf16 row stored at byte address out_rows[u] (any rank's window, 16-byte aligned)
 * and, when num_weights > 0, its top-k weights (the wtable / wsrc pass-through rule above, weights_pad
 * floats) at out_rows[u] + weights_offset.  All these stores are system-scope write-through (sc0 sc1),
 * so they are visible to the owning GPU once the kernel has completed.
 * Windows: window_bases (device uint64 [num_windows]) and window_bytes, the data extent of each.  Every
 * row is checked before it is stored: unless all its bytes (the bf16 row and, with weights, the weight
 * tail) lie inside one window, the unit is skipped, bit 4 of error_flag is set and the fault recorded
 * (DEEPEP_FAULT_SCATTER_ROW); out_rows[u] == 0 (a unit plan_expert rejected) is skipped with bit 1,
 * out_rows[u] == 1 (a padding position of a padded plan) silently.
 * error_flag: DEEPEP_ERROR_RECORD_INTS device ints or NULL. */
int deepep_combine_reduce_scatter(int weighted,
                                  const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                  const int32_t* table, int64_t table_stride, int table_width,
                                  const float* row_weights,
                                  const uint64_t* out_rows, int num_units, int hidden,
                                  const int32_t* wtable, int64_t wtable_stride,
                                  const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                  const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                  int32_t* error_flag, deepep_stream_t stream);

/* deepep_combine_reduce_scatter over FP8 source rows, cast back in registers as deepep_combine_reduce_fp8
 * does (src, src_row_stride, hidden, sf, sf_row_stride, sf_col_stride and sf_packed as there): phase A of
 * combine_impl (combine.cuh:114-213) reading the expert rows as an FP8 pair instead of the bf16 rows that
 * per_token_cast_back (deep_ep/utils/math.py:42-56) would have written first.  The rows stored into the
 * windows are bf16, exactly those of deepep_combine_reduce_scatter over the cast-back rows. */
int deepep_combine_reduce_scatter_fp8(int weighted,
                                      const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                      const void* sf, int64_t sf_row_stride, int64_t sf_col_stride, int sf_packed,
                                      const int32_t* table, int64_t table_stride, int table_width,
                                      const float* row_weights,
                                      const uint64_t* out_rows, int num_units, int hidden,
                                      const int32_t* wtable, int64_t wtable_stride,
                                      const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                      const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                      int32_t* error_flag, deepep_stream_t stream);

/* ---- LogFMT-10, fixed length: combine rows at 10 bits per element plus one (amax, amin) bf16 pair per 128
 * columns, the reference's use_logfmt of low_latency_combine.  The arithmetic, its three departures from the
 * reference (every group encoded, degenerate and non-finite groups exact, a decoded value rounded to bf16) and the
 * bit layout are in deepep_amd/csrc/logfmt_codec.h.  A row of `hidden` columns (hidden % 128 == 0) is
 *   planes  hidden + hidden / 4 bytes: [low plane: code & 0xff per column | high plane: two bits per column,
 *           (sign << 1) | (code >> 8), column c in bits 2 * (c & 3) of byte c / 4]
 *   meta    hidden / 128 dwords: amax_bits | amin_bits << 16 of each group.
 *
 * deepep_cast_logfmt: the encode (csrc/kernels/legacy/internode_ll.cu:557-638).  x: num_rows bf16 rows,
 * x_row_stride_bytes apart (>= hidden * 2, 16-byte aligned); planes [num_rows][hidden * 5 / 4] and meta
 * [num_rows][hidden / 128], both contiguous. */
int deepep_cast_logfmt(const void* x, int64_t x_row_stride_bytes, int num_rows, int hidden, void* planes, int32_t* meta,
                       deepep_stream_t stream);

/* deepep_cast_back_logfmt: the decode (csrc/kernels/legacy/internode_ll.cu:672-712) to contiguous bf16 rows
 * out [num_rows][hidden].  The planes' rows are planes_row_stride_bytes apart (>= hidden * 5 / 4, a multiple of
 * 16) and the meta rows meta_row_stride dwords, so the wire rows of deepep_logfmt_pack_rows are read in place. */
int deepep_cast_back_logfmt(const void* planes, int64_t planes_row_stride_bytes, const int32_t* meta,
                            int64_t meta_row_stride, int num_rows, int hidden, void* out, deepep_stream_t stream);

/* deepep_logfmt_pack_rows: the encode (internode_ll.cu:557-638) of the first num_rows packed exchange rows
 * [bf16 row | weight tail at src_tail_offset] into wire rows [low | high | meta | pad | weight tail at
 * dst_tail_offset]: the planes and the meta are those of deepep_cast_logfmt, the tail_bytes of the tail (whole
 * 16-byte vectors) are copied.  src and dst are different buffers. */
int deepep_logfmt_pack_rows(const void* src, int64_t src_row_bytes, int src_tail_offset, int num_rows, int hidden,
                            int tail_bytes, void* dst, int64_t dst_row_bytes, int dst_tail_offset,
                            deepep_stream_t stream);

/* deepep_combine_reduce(mode = DEEPEP_MODE_EPILOGUE) over LogFMT source rows, decoded in registers
 * (internode_ll.cu:672-712 inside the reduction of :992-1100): src is the planes' rows, src_row_stride_bytes apart,
 * meta their dwords, meta_row_stride dwords apart.  Every other argument is deepep_combine_reduce's.  The result is
 * bit for bit deepep_combine_reduce over the rows deepep_cast_back_logfmt writes. */
int deepep_combine_reduce_logfmt(int weighted,
                                 const void* src, int64_t num_src_rows, int64_t src_row_stride_bytes,
                                 const int32_t* meta, int64_t meta_row_stride,
                                 const int32_t* table, int64_t table_stride, int table_width,
                                 const float* row_weights,
                                 const void* bias0, const void* bias1,
                                 void* out, int64_t out_row_stride,
                                 int num_units, int hidden,
                                 const int32_t* wtable, int64_t wtable_stride,
                                 const float* wsrc, float* out_weights, int num_weights,
                                 int64_t out_weights_stride, int weights_pad,
                                 int32_t* error_flag, deepep_stream_t stream);

/* deepep_combine_reduce_scatter storing LogFMT wire rows: phase A of combine(use_logfmt=True) over the windows, the
 * encode fused into the sending kernel as the reference's (csrc/kernels/legacy/internode_ll.cu:557-638 inside the
 * combine of :992-1100).  The arguments are deepep_combine_reduce_scatter's, in its order; hidden is a positive
 * multiple of 128.  Unit u's row at out_rows[u] is
 *   [low plane, hidden bytes | high plane, hidden / 4 | meta, hidden / 128 dwords | padding | fp32 weights at
 *    weights_offset]
 * (deepep_logfmt_pack_rows' wire row): the planes and the meta are bit for bit deepep_cast_logfmt of the bf16 row
 * deepep_combine_reduce_scatter stores for the same arguments, the weights are its weights.  weights_offset (used
 * when num_weights > 0) is 16-byte aligned and at least the coded bytes hidden * 5 / 4 + hidden / 32; the bytes
 * between the meta and the weights are not written.  A row is checked against the windows with the extent
 * max(coded bytes, weights_offset + 4 * weights_pad) (the coded bytes alone without weights); the error record, the
 * out_rows values 0 and 1 and the stores' system scope are deepep_combine_reduce_scatter's. */
int deepep_combine_reduce_scatter_logfmt(int weighted,
                                         const void* src, int64_t num_src_rows, int64_t src_row_stride,
                                         const int32_t* table, int64_t table_stride, int table_width,
                                         const float* row_weights,
                                         const uint64_t* out_rows, int num_units, int hidden,
                                         const int32_t* wtable, int64_t wtable_stride,
                                         const float* wsrc, int num_weights, int64_t weights_offset, int weights_pad,
                                         const uint64_t* window_bases, int num_windows, int64_t window_bytes,
                                         int32_t* error_flag, deepep_stream_t stream);

/* A CU budget: a stream whose kernels run on `num_cus` compute units only, rounded up to a multiple
 * of 8 (hipExtStreamCreateWithCUMask, the first num_cus mask bits = num_cus / 8 CUs on every XCD),
 * leaving the rest to overlapping
 * compute.  It is how this build honours an explicit num_sms (the reference sizes combine_impl's
 * grid with it, csrc/kernels/elastic/combine.hpp:135, elastic.py:1086-1088). */
int deepep_stream_create_cu_budget(int num_cus, deepep_stream_t* stream);
int deepep_stream_destroy(deepep_stream_t stream);
/* Diagnostic: how many distinct CUs (and XCDs) a stream's workgroups run on (8192 one-wave workgroups
 * recording their hardware ids; synchronises the stream). */
int deepep_stream_probe_cus(deepep_stream_t stream, int* num_cus, int* num_xcds);

/* ElasticBuffer::get_combine_buffer_size for one node (num_scaleout_ranks == 1). */
int64_t deepep_combine_buffer_size(int num_max_tokens_per_rank, int hidden, int num_topk,
                                   int num_ranks, int allow_multiple_reduction);

#ifdef __cplusplus
}
#endif

#endif /* DEEPEP_AMD_H */
