"""EPHandle and the per-handle combine plan.

EPHandle keeps the attributes of the reference's handle
(deep_ep/buffers/elastic.py:25-98 in /root/reference) so user code that reads them
keeps working.  What is new is `CombinePlan`: the token -> source-row tables the
combine kernels read, derived once from the handle's routing and cached on it
(the reference re-derives them inside every combine_reduce_epilogue_impl launch,
combine_reduce_epilogue.cuh:62-95, by walking topk_idx and the symmetric receive
buffer; here they are small int32 tables, 4*K bytes per token).

Every table is built by kernels (deepep_build_local_plan at EP = 1, deepep_plan_expert /
deepep_plan_source at EP > 1) from device data, and every exchange size from counts the
host already holds since the dispatch's one host sync (`EPHandle._counts`): building a plan
never synchronises the host, so a first combine on a fresh handle can be captured into a
HIP graph.

Invariant the plan relies on for EP > 1 (guaranteed by ElasticBuffer.dispatch):
on every expert rank the received tokens are grouped by source rank and ascending
source token inside a rank -- the order of refs.dispatch (deep_ep/utils/refs.py:10-123)
and of the reference's deterministic mode (elastic.py:117-131).  The source rank can
then compute where each of its tokens' partials lands after the exchange without
any extra communication.
"""
from dataclasses import dataclass
from typing import List, Optional

import torch

from ._lib import (ERROR_RECORD_INTS, PLAN_BLOCK_TOKENS, PLAN_EXPANDED, PLAN_INTERLEAVE, PLAN_LOCAL_BYPASS,
                   PLAN_RANK_LAYOUT, PLAN_SINGLE, PLAN_WINDOW, describe_error_record)
from .utils import align, ceil_div


@dataclass
class BlockCounts:
    """Per 64-token block of a source rank's tokens (DEEPEP_PLAN_BLOCK_TOKENS), per peer rank: the
    tokens and the (token, top-k lane) pairs routed between them.  `send_*` [R][nb]: this rank's
    tokens to every destination; `recv_*` [R][nb]: every source's tokens to this rank (the dispatch
    notify).  Host lists (known since the dispatch's host sync) size the exchanges; the device tensor
    `dev` [4, R, nb] (send_tok, send_pairs, recv_tok, recv_pairs) feeds the plan kernels."""
    num_blocks: int
    send_tok: Optional[List[List[int]]]              # the host lists are None after a dispatch without a
    send_pairs: Optional[List[List[int]]]            # CPU sync: the combine plan is then worst-case padded
    recv_tok: Optional[List[List[int]]]
    recv_pairs: Optional[List[List[int]]]
    dev: torch.Tensor


@dataclass
class ChunkPlan:
    """One pipeline chunk of the EP > 1 combine: the source tokens [lo, hi) of every rank."""
    lo: int
    hi: int
    table_a: Optional[torch.Tensor]          # expert side: [n, K] expanded slots, [n, 1] rows / expanded rows
    wtable_a: Optional[torch.Tensor]         # expert side: [n, K] weight-source index (non-expanded)
    send_counts: List[int]                   # expert side: units sent back to every source rank
    back_counts: List[int]                   # source side: rows received from every expert rank
    table_b: torch.Tensor                    # source side: [hi - lo, min(R, K)] (multi) / [hi - lo, K] (single)
    wtable_b: Optional[torch.Tensor] = None  # source side: [hi - lo, K] weight index in the packed rows (multi)
    out_rows: Optional[torch.Tensor] = None  # xGMI transport, expert side: [n] window row address per unit
    own: int = 0                             # RCCL local bypass: units (= receive rows) of this rank itself


@dataclass
class CombinePlan:
    num_ranks: int
    num_tokens: int
    num_topk: int
    expanded: bool
    # EP == 1: token-major source-row table for the fused kernel
    local_table: Optional[torch.Tensor] = None        # [T, K] (expanded) or [T, 1] int32
    local_wtable: Optional[torch.Tensor] = None       # [T, K] int32, non-expanded weight pass-through
    # EP > 1: the pipeline chunks (one or more)
    chunks: Optional[List[ChunkPlan]] = None
    window_row_bytes: int = 0
    local_bypass: bool = False                        # RCCL: own units written in place (ChunkPlan.own)
    ready: Optional[tuple] = None                     # (stream, event) the tables were built on
    # RCCL transport: the plan kernels' error record (a unit rejected because the counts disagree with the
    # metadata or exceed the padding), copied to pinned host memory behind the build and checked by
    # poll() at the plan's next use -- no host sync (the xGMI transport uses its window's record)
    error_record: Optional[torch.Tensor] = None
    _flag_host: Optional[torch.Tensor] = None
    _flag_event: Optional[object] = None

    def publish(self, stream) -> None:
        if self.error_record is None or not self.error_record.is_cuda:
            return
        with torch.cuda.stream(stream):
            self._flag_host = torch.zeros((ERROR_RECORD_INTS,), dtype=torch.int32, pin_memory=True)
            self._flag_host.copy_(self.error_record, non_blocking=True)
            self._flag_event = torch.cuda.Event()
            self._flag_event.record(stream)

    def poll(self) -> None:
        """Raise (at every later use) once the published record shows a rejected plan entry: that
        handle's combines are wrong -- the reference has no recovery either (its device asserts trap)."""
        rec = None
        if self.error_record is not None and not self.error_record.is_cuda:
            rec = self.error_record.tolist()
        elif self._flag_event is not None and self._flag_event.query():
            rec = self._flag_host.tolist()
        if rec is not None and rec[0]:
            raise RuntimeError(f'deepep_amd: combine plan {describe_error_record(rec)}: the routing counts of '
                               f'this handle disagree with its metadata or exceed the padding of a dispatch '
                               f'without a CPU sync (a token routed twice to one expert?)')


LINE_BYTES = 128      # a memory-side line: packed rows are whole lines (a partial line costs a read-modify-write)


def packed_row_layout(hidden: int, num_topk: int, with_weights: bool = True, single: bool = False):
    """(row_bytes, weights_offset, weights_pad_floats) of a packed exchange row [bf16 row | fp32
    weights]: the bf16 part and the weight tail each a whole number of 128-byte lines, so every row
    starts on a line and the tail is written as full lines (zeros past the weights).  Measured on
    EP = 8's phase A (round 2, CHANGELOG.md): 32-byte aligned rows with a 32-byte weight tail 303 us,
    line-aligned rows with a partial tail line 281 us, line-aligned rows without a tail 257 us.
    single: one weight per row (the single reduction), else num_topk."""
    w_off = align(hidden * 2, LINE_BYTES)
    tail = align((1 if single else num_topk) * 4, LINE_BYTES) if with_weights else 0
    return w_off + tail, w_off, tail // 4


def logfmt_row_layout(hidden: int, num_topk: int, with_weights: bool = True, single: bool = False):
    """(row_bytes, weights_offset, weights_pad_floats) of a LogFMT wire row (combine(use_logfmt=True)):
    [low plane, hidden bytes | high plane, hidden / 4 | meta, hidden / 128 dwords | padding to a 128-byte line |
    fp32 weights] (csrc/logfmt_codec.h) -- packed_row_layout's rule: the coded part and the weight tail each a
    whole number of lines.  hidden % 128 == 0.  At hidden 7168, top-8: 9,344 bytes against 14,464."""
    if hidden % 128 != 0 or hidden <= 0:
        raise RuntimeError('deepep_amd: LogFMT rows need a hidden size that is a multiple of 128')
    w_off = align(hidden + hidden // 4 + hidden // 128 * 4, LINE_BYTES)
    tail = align((1 if single else num_topk) * 4, LINE_BYTES) if with_weights else 0
    return w_off + tail, w_off, tail // 4


def chunk_geometry(num_max_tokens: int, num_chunks: int):
    """(blocks, blocks per chunk, chunks): chunks are whole 64-token blocks, so their exchange sizes
    are sums of block counts; fewer chunks than asked when the batch is small."""
    nb = max(1, ceil_div(num_max_tokens, PLAN_BLOCK_TOKENS))
    bpc = max(1, ceil_div(nb, max(1, num_chunks)))
    return nb, bpc, ceil_div(nb, bpc)


def _chunk_sums(mat: List[List[int]], bpc: int, n_chunks: int) -> List[List[int]]:
    """[chunk][rank] sums of a [rank][block] count matrix."""
    return [[sum(row[c * bpc:(c + 1) * bpc]) for row in mat] for c in range(n_chunks)]


def build_ep_plan(kern, handle: 'EPHandle', *, num_ranks: int, rank: int, single: bool, num_chunks: int,
                  hidden: int, window=None, stream=None, local_bypass: bool = True,
                  cache_routing: bool = True, row_layout=None) -> CombinePlan:
    """The EP > 1 combine plan of `handle` on device tensors, with no host synchronisation.

    single: every valid expanded row travels unreduced (allow_multiple_reduction=False).
    window: the xGMI transport's SymmetricBuffer (rows go straight into the source ranks' windows)
    or None (RCCL all-to-all of packed rows).  hidden sizes the packed rows the weight tables
    point into.  local_bypass (RCCL): this rank's own partials skip the all-to-all (the default; off only
    to measure what the bypass saves, DEEPEP_LOCAL_BYPASS=0).  cache_routing: EPHandle.routing_idx64's
    `cache` (False while a HIP graph is being captured).  row_layout: the layout of the rows phase B reads --
    and, with a window, of the rows phase A stores into it (the pitch of out_rows, window_row_bytes) --
    packed_row_layout (the default) or logfmt_row_layout."""
    bypass = local_bypass and window is None
    R, T_max = num_ranks, handle.num_max_tokens_per_rank
    T, K = handle.topk_idx.shape
    cnt = handle._counts
    nb, bpc, C = chunk_geometry(T_max, num_chunks)
    if cnt.num_blocks != nb:
        raise RuntimeError('deepep_amd: handle block counts do not match num_max_tokens_per_rank')
    expanded = handle.do_expand
    rank_layout = R <= K                             # use_rank_layout (combine_utils.cuh:8-13)
    dev = handle.recv_src_metadata.device
    # A handle from a dispatch without a CPU sync: the counts live on the device only, so every chunk
    # is laid out for the worst case -- `padded` unit positions per source rank (a chunk's tokens, times
    # min(K, experts per rank) for the single reduction: a token's lanes on one rank are distinct experts
    # there, buffer.hpp:1067-1069's bound; a unit past it is rejected by the plan kernel, flagged, never
    # stored), the unused ones skipped by phase A (zero partials over RCCL, padding rows the scatter
    # ignores over xGMI) -- and the RCCL exchange moves R x padded rows per chunk.  Memory and traffic
    # of that padding: DESIGN.md section 1.
    padded = 0
    if cnt.recv_tok is None:
        padded = bpc * PLAN_BLOCK_TOKENS * (min(K, handle.num_experts // R) if single else 1)
    # ---- expert side: phase-A units of every chunk, concatenated
    if padded:
        units = [[padded] * R for _ in range(C)]
    else:
        units = _chunk_sums(cnt.recv_pairs if single else cnt.recv_tok, bpc, C)   # [c][source rank]
    n_units = [sum(u) for u in units]
    total = sum(n_units)
    # RCCL: the local bypass -- this rank's own units are written by phase A straight into the receive rows
    # phase B reads ([send rows | own rows | received rows], exchange._combine_chunks), so the all-to-all
    # moves no diagonal; xGMI: units round-robin over the peers
    flags = ((PLAN_EXPANDED if expanded else 0) | (PLAN_SINGLE if single else 0) |
             (PLAN_RANK_LAYOUT if rank_layout and not single else 0) |
             (PLAN_INTERLEAVE if window is not None else 0) | (PLAN_LOCAL_BYPASS if bypass else 0))
    width_a = K if expanded and not single else 1
    # Pre-filled, so a unit the plan kernel does not write (counts that disagree with the metadata) is a
    # skipped slot (-1) and a null window row (0) -- never stale allocator bytes used as an address.
    table_a = torch.full((total, width_a), -1, dtype=torch.int32, device=dev)
    wtable_a = torch.full((total, K), -1, dtype=torch.int32, device=dev) if not expanded else None
    if window is not None:
        row_bytes = (row_layout or packed_row_layout)(hidden, K, True, single)[0]
        # 1 marks a padding position (skipped silently), 0 a unit the plan kernel rejects (flagged)
        out_rows = torch.full((total,), 1 if padded else 0, dtype=torch.int64, device=dev)
        bases, win_bytes, err = window.data_bases_dev, window.data_bytes, window.error_flag
    else:
        row_bytes, out_rows, bases, win_bytes = 0, None, None, 0
        err = torch.zeros((ERROR_RECORD_INTS,), dtype=torch.int32, device=dev)
    kern.plan_expert(handle.recv_src_metadata, K, R, rank, T_max, cnt.dev[2], cnt.dev[3], nb, bpc, flags,
                     table_a, wtable_a, bases, row_bytes, out_rows, window_bytes=win_bytes, error_flag=err,
                     padded_stride=padded, stream=stream)
    # ---- source side: the rows phase B reduces per owned token
    if padded:
        back = [[padded] * R for _ in range(C)]
    else:
        back = _chunk_sums(cnt.send_pairs if single else cnt.send_tok, bpc, C)   # [c][expert rank]
    width_b = K if single else min(R, K)
    table_b = torch.empty((T, width_b), dtype=torch.int32, device=dev)
    wtable_b = None
    row_floats = w_off_f = 0
    if not single:
        # weight index into the packed rows: [bf16 partial | fp32 weights (16-byte aligned)]
        rb, w_off, _ = (row_layout or packed_row_layout)(hidden, K, True)
        row_floats, w_off_f = rb // 4, w_off // 4
        max_rows = min(R, K) * T_max if window is not None else max([sum(b) for b in back] + [0])
        if max_rows * row_floats + w_off_f + K < 2 ** 31:
            wtable_b = torch.empty((T, K), dtype=torch.int32, device=dev)
    sflags = (PLAN_SINGLE if single else 0) | (PLAN_WINDOW if window is not None else 0) | \
             (PLAN_LOCAL_BYPASS if bypass else 0) | \
             (PLAN_RANK_LAYOUT if rank_layout and not single else 0)
    kern.plan_source(handle.routing_idx64(cache_routing), handle.num_experts, R, rank, T_max,
                     handle.dst_buffer_slot_idx, cnt.dev[0], cnt.dev[1], nb, bpc, sflags, row_floats, w_off_f,
                     table_b, wtable_b,
                     padded_stride=padded if window is None else 0, stream=stream)
    plan = CombinePlan(num_ranks=R, num_tokens=T, num_topk=K, expanded=expanded, chunks=[],
                       window_row_bytes=row_bytes, error_record=err if window is None else None,
                       local_bypass=bypass)
    u0 = 0
    for c in range(C):
        lo, hi = min(c * bpc * PLAN_BLOCK_TOKENS, T), min((c + 1) * bpc * PLAN_BLOCK_TOKENS, T)
        u1 = u0 + n_units[c]
        # expanded: a unit's weights are those of its expanded rows, so the slot table is the weight table
        plan.chunks.append(ChunkPlan(lo, hi, table_a[u0:u1], wtable_a[u0:u1] if wtable_a is not None else
                                     (table_a[u0:u1] if expanded and not single else None),
                                     units[c], back[c], table_b[lo:hi],
                                     wtable_b[lo:hi] if wtable_b is not None else None,
                                     out_rows[u0:u1] if out_rows is not None else None,
                                     units[c][rank] if bypass else 0))
        u0 = u1
    return plan


class EPHandle:
    """Communication handle returned by `ElasticBuffer.dispatch` (same attributes as the reference)."""

    def __init__(self,
                 do_expand: bool,
                 num_experts: int, expert_alignment: int,
                 num_max_tokens_per_rank: int,
                 num_sms: int,
                 topk_idx: torch.Tensor,
                 num_recv_tokens: int,
                 num_expanded_tokens: int,
                 num_recv_tokens_per_expert_list: list,
                 psum_num_recv_tokens_per_scaleup_rank: torch.Tensor,
                 psum_num_recv_tokens_per_expert: torch.Tensor,
                 num_unaligned_recv_tokens_per_expert: torch.Tensor,
                 recv_src_metadata: torch.Tensor,
                 dst_buffer_slot_idx: torch.Tensor,
                 token_metadata_at_forward: Optional[torch.Tensor],
                 channel_linked_list: Optional[torch.Tensor]):
        assert topk_idx is not None
        self.do_expand = do_expand
        self.num_experts = num_experts
        self.expert_alignment = expert_alignment
        self.num_max_tokens_per_rank = num_max_tokens_per_rank
        self.num_sms = num_sms
        self.topk_idx = topk_idx
        self.psum_num_recv_tokens_per_scaleup_rank = psum_num_recv_tokens_per_scaleup_rank
        self.psum_num_recv_tokens_per_expert = psum_num_recv_tokens_per_expert
        self.num_unaligned_recv_tokens_per_expert = num_unaligned_recv_tokens_per_expert
        self.num_recv_tokens_per_expert_list = num_recv_tokens_per_expert_list
        self.recv_src_metadata = recv_src_metadata
        self.dst_buffer_slot_idx = dst_buffer_slot_idx
        self.token_metadata_at_forward = token_metadata_at_forward
        self.channel_linked_list = channel_linked_list
        self.num_recv_tokens = num_recv_tokens
        self.num_expanded_tokens = num_expanded_tokens
        self.cached_recv_src_metadata_before_sort = None
        # Host-side copies captured at dispatch (counts per source rank), and the combine plan cache
        self._recv_counts: Optional[List[int]] = None
        self._send_counts: Optional[List[int]] = None         # cached dispatch: no host sync needed
        self._send_offsets: Optional[torch.Tensor] = None
        self._recv_topk_idx: Optional[torch.Tensor] = None    # non-expanded recv_topk_idx (int64, N rows)
        self._idx64: Optional[torch.Tensor] = None            # the routing as the kernels read it (routing_idx64)
        self._counts: Optional[BlockCounts] = None            # per-block routing counts (EP > 1 plans)
        self._bypass = False                                  # rows laid out for the dispatch's local bypass
        self._combine_plans = {}

    def routing_idx64(self, cache: bool = True) -> torch.Tensor:
        """The routing as every kernel reads it: contiguous int64.  `topk_idx` keeps the caller's dtype
        (deep_ep.topk_idx_t: int32 with EP_NUM_TOPK_IDX_BITS=32); with int64 routing this IS `topk_idx`
        (no copy, no launch).  The dispatch that makes a handle stores its own int64 routing here; a
        handle built by hand converts on the first use and keeps the result (cache=False: a conversion
        recorded into a HIP graph holds no data outside that graph, so it is not kept)."""
        if self._idx64 is not None:
            return self._idx64
        idx = self.topk_idx
        idx64 = idx if idx.dtype == torch.int64 and idx.is_contiguous() else idx.to(torch.int64).contiguous()
        if cache or idx64 is idx:
            self._idx64 = idx64
        return idx64

    def deterministic_sort(self, do_cpu_sync: bool, is_cached_dispatch: bool, recv_x: torch.Tensor,
                           recv_sf: Optional[torch.Tensor], recv_topk_idx: torch.Tensor,
                           recv_topk_weights: torch.Tensor, channel_linked_list: Optional[torch.Tensor]) -> None:
        """The reference's signature (elastic.py:100-107).  The dispatch of this build is deterministic by
        construction (received tokens sorted by source global index, expanded rows by (expert, source index)),
        which is the order the reference's in-place permutation produces (elastic.py:108-192): the permutation
        is the identity, so nothing moves."""
        return None
