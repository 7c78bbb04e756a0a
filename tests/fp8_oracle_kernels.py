"""The CPU kernel provider with the FP8 cast wrappers, a forwarding spy and the comparison of two dispatch
results -- TEST INFRASTRUCTURE ONLY.

`Fp8OracleKernels` adds the three casting wrappers of deepep_amd.kernels.HipKernels (cast_fp8,
dispatch_pack_cast, dispatch_copy_cast) to tests/oracle_kernels.OracleKernels: each one casts with the torch
code on the CPU (tests/test_fp8_cast_gpu.cast_ref, the contract of the HIP kernels) and calls the parent's
method with the cast pair, after asserting what the HIP wrapper requires of its arguments.  The product never
selects it."""
import threading

import torch

from tests.oracle_kernels import OracleKernels, _routing
from tests.test_fp8_cast_gpu import _same, cast_ref


def _bf16_rows(x_bytes: torch.Tensor, what: str) -> torch.Tensor:
    """The bf16 [T, H] tensor behind its uint8 view [T, 2 * H] (what the HIP wrappers take), H % 128 == 0."""
    assert x_bytes is not None and x_bytes.dtype == torch.uint8 and x_bytes.dim() == 2, \
        f'{what} reads the uint8 view of bf16 rows'
    assert x_bytes.numel() == 0 or x_bytes.stride(1) == 1, f'{what} needs unit column stride'
    H = x_bytes.shape[1] // 2
    assert x_bytes.shape[1] == 2 * H and H % 128 == 0, f'{what} needs bf16 rows of H % 128 == 0 columns'
    return x_bytes.contiguous().view(torch.bfloat16).view(x_bytes.shape[0], H)


def _pair_bytes(x: torch.Tensor, round_scale: bool):
    q, sf = cast_ref(x, round_scale)
    return q.view(torch.uint8), sf.contiguous().view(torch.uint8).view(sf.shape[0], sf.shape[1] * 4)


class Fp8OracleKernels(OracleKernels):
    name = 'oracle-fp8'

    def cast_fp8(self, x, q, sf, round_scale=False, stream=None):
        assert x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1)
        T, H = x.shape
        assert H % 128 == 0
        assert q.dtype == torch.float8_e4m3fn and q.is_contiguous() and tuple(q.shape) == (T, H)
        assert sf.dtype == torch.float32 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 128)
        q_ref, sf_ref = cast_ref(x, round_scale)
        q.view(torch.uint8).copy_(q_ref.view(torch.uint8))
        sf.copy_(sf_ref)

    def dispatch_pack_cast(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed, layout,
                           round_scale=False, dest_bases=None, dest_rows=None, error_flag=None, stream=None):
        _routing(topk_idx)
        x = _bf16_rows(x_bytes, 'dispatch_pack_cast')
        H = x.shape[1]
        assert layout.x_bytes == H and layout.sf_bytes == H // 128 * 4, \
            'dispatch_pack_cast needs the FP8 row layout RowLayout.make(H, H / 128 * 4, K)'
        q_bytes, sf_bytes = _pair_bytes(x, round_scale)
        self.dispatch_pack(q_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout, dest_bases=dest_bases, dest_rows=dest_rows, error_flag=error_flag)

    def dispatch_copy_cast(self, packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=None, sf_direct=None, num_max_tokens=0, error_flag=None, inv=None,
                           block_offsets=None, expert_end=None, row_map=None, round_scale=False, stream=None):
        assert x_direct is not None and sf_direct is None, \
            'dispatch_copy_cast reads the bf16 rows of x_direct and takes no sf_direct'
        x = _bf16_rows(x_direct, 'dispatch_copy_cast')
        H = x.shape[1]
        assert recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and \
            recv_x_bytes.shape[1] == H, 'dispatch_copy_cast writes contiguous bytes [rows, H]'
        assert recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and \
            tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 128 * 4), \
            'dispatch_copy_cast writes contiguous bytes [rows, H / 128 * 4]'
        q_bytes, sf_bytes = _pair_bytes(x, round_scale)
        self.dispatch_copy(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=q_bytes, sf_direct=sf_bytes, num_max_tokens=num_max_tokens,
                           error_flag=error_flag, inv=inv, block_offsets=block_offsets, expert_end=expert_end,
                           row_map=row_map)


CAST_WRAPPERS = ('cast_fp8', 'dispatch_pack_cast', 'dispatch_copy_cast')


def _describe(v):
    """A tensor as (shape, dtype); containers element by element; anything else by value."""
    if isinstance(v, torch.Tensor):
        return ('tensor', tuple(v.shape), str(v.dtype))
    if isinstance(v, (tuple, list)):
        return tuple(_describe(e) for e in v)
    if isinstance(v, dict):
        return tuple((k, _describe(e)) for k, e in sorted(v.items()))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__ if not hasattr(v, '__dataclass_fields__') else repr(v)


class Spy:
    """Forwards every wrapper call to `inner` and records (name, argument shapes / dtypes / values) and, under
    `tensors`, the tensor arguments themselves by parameter name (keyword arguments only)."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = []
        self.tensors = []
        self._lock = threading.Lock()

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def forward(*args, **kwargs):
            with self._lock:
                stream_free = {k: v for k, v in kwargs.items() if k != 'stream'}
                self.calls.append((name, _describe(args), _describe(stream_free)))
                self.tensors.append((name, args, kwargs))
            return attr(*args, **kwargs)
        return forward

    def names(self):
        return [c[0] for c in self.calls]


HANDLE_FIELDS = ('do_expand', 'num_experts', 'expert_alignment', 'num_max_tokens_per_rank', 'num_sms', 'topk_idx',
                 'num_recv_tokens', 'num_expanded_tokens', 'num_recv_tokens_per_expert_list',
                 'psum_num_recv_tokens_per_scaleup_rank', 'psum_num_recv_tokens_per_expert',
                 'num_unaligned_recv_tokens_per_expert', 'recv_src_metadata', 'dst_buffer_slot_idx',
                 'token_metadata_at_forward', 'channel_linked_list')


def dispatch_differences(got, want):
    """The names of what differs, bitwise, between two results of ElasticBuffer.dispatch: recv_x (a tensor or the
    (rows, scale factors) pair; dtype, shape and strides' layout included through the values), recv_topk_idx,
    recv_topk_weights and every field of the handle."""
    bad = []
    for name, a, b in (('recv_x', got[0], want[0]), ('recv_topk_idx', got[1], want[1]),
                       ('recv_topk_weights', got[2], want[2])):
        if not _same(a, b):
            bad.append(name)
    if isinstance(got[0], tuple) and isinstance(want[0], tuple) and got[0][1].stride() != want[0][1].stride():
        bad.append('scale factor strides')
    for f in HANDLE_FIELDS:
        a, b = getattr(got[3], f), getattr(want[3], f)
        if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
            if not _same(a, b):
                bad.append(f'handle.{f}')
        elif a != b:
            bad.append(f'handle.{f}')
    return bad


def cast_pair(x: torch.Tensor, round_scale: bool = False):
    """The CPU-cast pair of a bf16 x (cast_ref), on the device of x."""
    q, sf = cast_ref(x, round_scale)
    return q.to(x.device), sf.to(x.device)


def keyword_cases(buf, inputs, empty_inputs, num_experts: int):
    """dispatch(x, cast_to_fp8=True, ...) against dispatch(cast_pair(x), ...) of the same buffer, in every mode
    the keyword composes with (any kernel provider, any device, any rank count: every rank makes the same calls).
    inputs / empty_inputs: (x, topk_idx, topk_weights), the second for the no-token case (on the ranks that
    have tokens in it, a second full batch).  Returns the list of differences.  Expanded layouts whose padding
    rows nobody writes are compared with zero padding only."""
    fails = []
    x, idx, w = inputs
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def compare(label, xin, round_scale=False, **kw):
        got = buf.dispatch(xin, cast_to_fp8=True, fp8_round_scale=round_scale, **kw)
        want = buf.dispatch(cast_pair(xin, round_scale), **kw)
        bad = dispatch_differences(got, want)
        if not (isinstance(got[0], tuple) and got[0][0].dtype == torch.float8_e4m3fn and
                got[0][1].dtype == torch.float32):
            bad.append('recv_x is not the (float8_e4m3fn, float32) pair')
        if bad:
            fails.append(f'{label}: {bad}')
        return got

    padded = dict(do_expand=True, expert_alignment=16, do_zero_padding=True)
    compare('reduced', x, **base)
    compare('expanded', x, do_expand=True, **base)
    compare('expanded, alignment 16, zero padding', x, **padded, **base)
    compare('reduced, column-major sf', x, use_tma_aligned_col_major_sf=True, **base)
    compare('expanded, column-major sf', x, use_tma_aligned_col_major_sf=True, **padded, **base)
    compare('reduced, round_scale', x, round_scale=True, **base)
    compare('expanded, round_scale', x, round_scale=True, do_expand=True, **base)
    compare('reduced, no CPU sync', x, do_cpu_sync=False, **base)
    compare('expanded, no CPU sync', x, do_cpu_sync=False, **padded, **base)
    # a cached handle remembers nothing about dtypes: a bf16 dispatch's handle serves a casting dispatch ...
    for more in (dict(), dict(do_expand=True), dict(do_cpu_sync=False)):
        h_bf16 = buf.dispatch(x, **more, **base)[3]
        h_cast = buf.dispatch(x, cast_to_fp8=True, **more, **base)[3]
        expand = dict(do_expand=h_bf16.do_expand)
        compare(f'cached on a bf16 handle ({more})', x, handle=h_bf16, **expand)
        compare(f'cached on a casting handle ({more})', x, round_scale=True, handle=h_cast, **expand)
        # ... and the other way round: a casting dispatch's handle serves a bf16 dispatch
        bad = dispatch_differences(buf.dispatch(x, handle=h_cast, **expand), buf.dispatch(x, handle=h_bf16, **expand))
        bad = [b for b in bad if not b.startswith('handle.')]      # each call returns the handle it was given
        if bad:
            fails.append(f'bf16 dispatch cached on a casting handle ({more}): {bad}')
    x0, idx0, w0 = empty_inputs
    for expand in (False, True):
        compare(f'no tokens (expand={expand})', x0, topk_idx=idx0, topk_weights=w0, num_experts=num_experts,
                do_expand=expand)
    return fails
