"""Packed UE8M0 scale factors: the torch reference of the packed form, a CPU kernel provider whose casting wrappers
know `ue8m0`, and the comparison of the keyword dispatch with the tuple dispatch -- TEST INFRASTRUCTURE ONLY.

The packed form (include/deepep_amd.h): for H % 512 == 0 the scale factors are int32 [rows, H / 512]; byte j
(little-endian) of element p is the biased exponent (bits(sf) >> 23) & 0xff of column group 4p + j, sf the
power-of-two factor of the round_scale cast (tests/test_fp8_cast_gpu.cast_ref(x, True)).  The cast back multiplies by
float_from_bits(byte << 23), the reference's `view(uint8).to(int) << 23` viewed as float
(deep_ep/utils/math.py:51-53)."""
import torch

from tests.fp8_oracle_kernels import Fp8OracleKernels, _bf16_rows, dispatch_differences
from tests.oracle_kernels import _routing
from tests.test_fp8_cast_gpu import cast_ref


def pack_ref(sf: torch.Tensor) -> torch.Tensor:
    """fp32 power-of-two factors [rows, G], G % 4 == 0 -> int32 [rows, G / 4] of their exponent bytes."""
    assert sf.dtype == torch.float32 and sf.dim() == 2 and sf.shape[1] % 4 == 0
    exp = ((sf.contiguous().view(torch.int32) >> 23) & 0xff).to(torch.uint8)
    return exp.contiguous().view(torch.int32)


def unpack_ref(sf: torch.Tensor) -> torch.Tensor:
    """The inverse: int32 [rows, P] (any strides) -> fp32 [rows, 4 * P], float_from_bits(byte << 23)."""
    assert sf.dtype == torch.int32 and sf.dim() == 2
    exp = sf.contiguous().view(torch.uint8).to(torch.int32)
    return (exp << 23).view(torch.float32)


def ue8m0_pair(x: torch.Tensor):
    """(cast_ref q, pack_ref sf) of a bf16 x, on the device of x: what every packed result is compared with."""
    q, sf = cast_ref(x, True)
    return q.to(x.device), pack_ref(sf).to(x.device)


def _packed_bytes(x: torch.Tensor):
    q, sf = cast_ref(x, True)
    return q.view(torch.uint8), pack_ref(sf).view(torch.uint8).view(sf.shape[0], sf.shape[1])


class Ue8m0OracleKernels(Fp8OracleKernels):
    """Fp8OracleKernels whose three casting wrappers take `ue8m0` as deepep_amd.kernels.HipKernels' do: they assert
    what the HIP wrappers require and hand the pack_ref bytes to the parent's dispatch_pack / dispatch_copy."""
    name = 'oracle-ue8m0'

    def cast_fp8(self, x, q, sf, round_scale=False, stream=None, ue8m0=False):
        if not ue8m0:
            return super().cast_fp8(x, q, sf, round_scale, stream)
        assert round_scale, 'UE8M0 scale factors are power-of-two factors: round_scale'
        assert x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1)
        T, H = x.shape
        assert H % 512 == 0
        assert q.dtype == torch.float8_e4m3fn and q.is_contiguous() and tuple(q.shape) == (T, H)
        assert sf.dtype == torch.int32 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 512)
        q_ref, sf_ref = cast_ref(x, True)
        q.view(torch.uint8).copy_(q_ref.view(torch.uint8))
        sf.copy_(pack_ref(sf_ref))

    def dispatch_pack_cast(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed, layout,
                           round_scale=False, dest_bases=None, dest_rows=None, error_flag=None, stream=None,
                           ue8m0=False):
        if not ue8m0:
            return super().dispatch_pack_cast(x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets,
                                              packed, layout, round_scale, dest_bases, dest_rows, error_flag, stream)
        _routing(topk_idx)
        assert round_scale, 'UE8M0 scale factors are power-of-two factors: round_scale'
        x = _bf16_rows(x_bytes, 'dispatch_pack_cast')
        H = x.shape[1]
        assert H % 512 == 0 and layout.x_bytes == H and layout.sf_bytes == H // 128, \
            'dispatch_pack_cast(ue8m0) needs H % 512 == 0 and the row layout RowLayout.make(H, H / 128, K)'
        q_bytes, sf_bytes = _packed_bytes(x)
        self.dispatch_pack(q_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout, dest_bases=dest_bases, dest_rows=dest_rows, error_flag=error_flag)

    def dispatch_copy_cast(self, packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=None, sf_direct=None, num_max_tokens=0, error_flag=None, inv=None,
                           block_offsets=None, expert_end=None, row_map=None, round_scale=False, stream=None,
                           ue8m0=False):
        if not ue8m0:
            return super().dispatch_copy_cast(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                                              recv_w, x_direct, sf_direct, num_max_tokens, error_flag, inv,
                                              block_offsets, expert_end, row_map, round_scale, stream)
        assert round_scale, 'UE8M0 scale factors are power-of-two factors: round_scale'
        assert x_direct is not None and sf_direct is None
        x = _bf16_rows(x_direct, 'dispatch_copy_cast')
        H = x.shape[1]
        assert H % 512 == 0
        assert recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and \
            recv_x_bytes.shape[1] == H, 'dispatch_copy_cast writes contiguous bytes [rows, H]'
        assert recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and \
            tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 128), \
            'dispatch_copy_cast(ue8m0) writes contiguous bytes [rows, H / 128]'
        q_bytes, sf_bytes = _packed_bytes(x)
        self.dispatch_copy(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=q_bytes, sf_direct=sf_bytes, num_max_tokens=num_max_tokens,
                           error_flag=error_flag, inv=inv, block_offsets=block_offsets, expert_end=expert_end,
                           row_map=row_map)


UE8M0 = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True)


def packed_differences(got, want):
    """dispatch_differences for results whose scale factors may be one column wide (H = 512): a column-major
    [rows, 1] tensor counts as contiguous while its last stride is not 1, which the byte view of the comparison
    refuses, so the values are compared through copies of standard strides and the strides themselves here."""
    def standard(res):
        if not isinstance(res[0], tuple):
            return res
        q, sf = res[0]
        return ((q, torch.empty(sf.shape, dtype=sf.dtype, device=sf.device).copy_(sf)),) + tuple(res[1:])

    bad = dispatch_differences(standard(got), standard(want))
    if isinstance(got[0], tuple) and isinstance(want[0], tuple) and got[0][1].stride() != want[0][1].stride():
        bad.append('scale factor strides')
    return bad


def compare_ue8m0(buf, xin, **kw):
    """The differences between dispatch(xin, all three flags, **kw) and dispatch(ue8m0_pair(xin), **kw), and the
    keyword result."""
    got = buf.dispatch(xin, **UE8M0, **kw)
    want = buf.dispatch(ue8m0_pair(xin), **kw)
    bad = packed_differences(got, want)
    if not (isinstance(got[0], tuple) and got[0][0].dtype == torch.float8_e4m3fn and got[0][1].dtype == torch.int32 and
            got[0][1].shape[1] == xin.shape[1] // 512):
        bad.append('recv_x is not the (float8_e4m3fn [rows, H], int32 [rows, H / 512]) pair')
    return bad, got


def ue8m0_cases(buf, inputs, empty_inputs, num_experts: int):
    """dispatch(x, cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True, ...) against the tuple dispatch of
    ue8m0_pair(x) on the same buffer, in every mode the keyword composes with (any kernel provider, any device, any
    rank count: every rank makes the same calls).  inputs / empty_inputs: (x, topk_idx, topk_weights), the second
    for the no-token case (on the ranks that have tokens in it, a second full batch).  Returns the differences.
    Expanded layouts whose padding rows nobody writes are compared with zero padding only."""
    fails = []
    x, idx, w = inputs
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def compare(label, xin, **kw):
        bad, got = compare_ue8m0(buf, xin, **kw)
        if bad:
            fails.append(f'{label}: {bad}')
        return got

    padded = dict(do_expand=True, expert_alignment=16, do_zero_padding=True)
    compare('reduced', x, **base)
    compare('expanded', x, do_expand=True, **base)
    compare('expanded, alignment 16, zero padding', x, **padded, **base)
    compare('reduced, column-major sf', x, use_tma_aligned_col_major_sf=True, **base)
    compare('expanded, column-major sf', x, use_tma_aligned_col_major_sf=True, **padded, **base)
    compare('reduced, no CPU sync', x, do_cpu_sync=False, **base)
    compare('expanded, no CPU sync', x, do_cpu_sync=False, **padded, **base)
    # a cached handle remembers nothing about dtypes: a bf16 dispatch's handle and a packed casting dispatch's
    # handle both serve a cached packed dispatch
    for more in (dict(), dict(do_expand=True), dict(do_cpu_sync=False)):
        h_bf16 = buf.dispatch(x, **more, **base)[3]
        h_cast = buf.dispatch(x, **UE8M0, **more, **base)[3]
        expand = dict(do_expand=h_bf16.do_expand)
        compare(f'cached on a bf16 handle ({more})', x, handle=h_bf16, **expand)
        compare(f'cached on a packed casting handle ({more})', x, handle=h_cast, **expand)
    x0, idx0, w0 = empty_inputs
    for expand in (False, True):
        compare(f'no tokens (expand={expand})', x0, topk_idx=idx0, topk_weights=w0, num_experts=num_experts,
                do_expand=expand)
    return fails
