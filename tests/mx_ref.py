"""MXFP8 (OCP e4m3fn rows, one UE8M0 exponent byte per 32 columns): the torch reference built from the pinned
per-128 reference, a CPU kernel provider whose casting wrappers know `mx`, and the comparison of the keyword dispatch
with the tuple dispatch -- TEST INFRASTRUCTURE ONLY.

The form (include/deepep_amd.h): for H % 128 == 0 the scale factors are uint8 [rows, H / 32], byte g the biased
exponent of column group g under the round_scale rule of tests/test_fp8_cast_gpu.cast_ref(x, True) with 32 columns in
place of 128.  The cast back multiplies by float_from_bits(byte << 23)."""
import torch

from tests.fp8_oracle_kernels import _bf16_rows
from tests.oracle_kernels import _routing
from tests.test_fp8_cast_gpu import cast_ref
from tests.ue8m0_ref import Ue8m0OracleKernels, packed_differences
from workloads import per_token_cast_back as torch_cast_back


def mx_pair(x: torch.Tensor):
    """(q float8_e4m3fn [T, H], sf uint8 [T, H / 32]) of a bf16 x, on the device of x.  No new arithmetic: every group
    of 32 columns becomes a row of its own, zero-padded to 128 columns (zeros do not change an amax), and goes through
    cast_ref(.., True); the group's e4m3fn bytes are the first 32 of that row, its byte the exponent of the factor."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 128 == 0
    T, H = x.shape
    groups = x.cpu().contiguous().view(T * H // 32, 32)
    padded = torch.zeros((groups.shape[0], 128), dtype=torch.bfloat16)
    padded[:, :32] = groups
    q, sf = cast_ref(padded, True)
    q = q.view(torch.uint8)[:, :32].contiguous().view(T, H).view(torch.float8_e4m3fn)
    exp = ((sf[:, 0].contiguous().view(torch.int32) >> 23) & 0xff).to(torch.uint8).view(T, H // 32)
    return q.to(x.device), exp.to(x.device)


def mx_factors(sf: torch.Tensor) -> torch.Tensor:
    """uint8 / float8_e8m0fnu [rows, G] exponent bytes (any strides) -> fp32 [rows, G], float_from_bits(byte << 23)."""
    exp = torch.empty(sf.shape, dtype=torch.uint8).copy_(sf.cpu().view(torch.uint8))
    return (exp.to(torch.int32) << 23).view(torch.float32)


def mx_back_ref(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """bf16 [M, H] of an MXFP8 pair on the CPU: the torch per_token_cast_back (tests/test_cast_back_gpu.back_ref's)
    over rows of one 32-column group each, zero-padded to 128 columns, with the factors of mx_factors."""
    M, H = q.shape
    codes = q.cpu().contiguous().view(torch.uint8).view(M * H // 32, 32)
    padded = torch.zeros((codes.shape[0], 128), dtype=torch.uint8)
    padded[:, :32] = codes
    out = torch_cast_back(padded.view(torch.float8_e4m3fn), mx_factors(sf).reshape(-1, 1))
    return out[:, :32].contiguous().view(M, H)


def _mx_bytes(x: torch.Tensor):
    q, sf = mx_pair(x)
    return q.view(torch.uint8), sf


class MxOracleKernels(Ue8m0OracleKernels):
    """Ue8m0OracleKernels whose three casting wrappers take `mx` as deepep_amd.kernels.HipKernels' do: they assert
    what the HIP wrappers require and hand the mx_pair bytes to the parent's dispatch_pack / dispatch_copy."""
    name = 'oracle-mx'

    def cast_fp8(self, x, q, sf, round_scale=False, stream=None, ue8m0=False, mx=False):
        if not mx:
            return super().cast_fp8(x, q, sf, round_scale, stream, ue8m0)
        assert round_scale and not ue8m0, 'MXFP8 scale factors are power-of-two factors: round_scale, not ue8m0'
        assert x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1)
        T, H = x.shape
        assert H % 128 == 0
        assert q.dtype == torch.float8_e4m3fn and q.is_contiguous() and tuple(q.shape) == (T, H)
        assert sf.dtype == torch.uint8 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 32)
        q_ref, sf_ref = mx_pair(x)
        q.view(torch.uint8).copy_(q_ref.view(torch.uint8))
        sf.copy_(sf_ref)

    def dispatch_pack_cast(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed, layout,
                           round_scale=False, dest_bases=None, dest_rows=None, error_flag=None, stream=None,
                           ue8m0=False, mx=False):
        if not mx:
            return super().dispatch_pack_cast(x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets,
                                              packed, layout, round_scale, dest_bases, dest_rows, error_flag, stream,
                                              ue8m0)
        _routing(topk_idx)
        assert round_scale and not ue8m0, 'MXFP8 scale factors are power-of-two factors: round_scale, not ue8m0'
        x = _bf16_rows(x_bytes, 'dispatch_pack_cast')
        H = x.shape[1]
        assert layout.x_bytes == H and layout.sf_bytes == H // 32, \
            'dispatch_pack_cast(mx) needs the row layout RowLayout.make(H, H / 32, K)'
        q_bytes, sf_bytes = _mx_bytes(x)
        self.dispatch_pack(q_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout, dest_bases=dest_bases, dest_rows=dest_rows, error_flag=error_flag)

    def dispatch_copy_cast(self, packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=None, sf_direct=None, num_max_tokens=0, error_flag=None, inv=None,
                           block_offsets=None, expert_end=None, row_map=None, round_scale=False, stream=None,
                           ue8m0=False, mx=False):
        if not mx:
            return super().dispatch_copy_cast(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                                              recv_w, x_direct, sf_direct, num_max_tokens, error_flag, inv,
                                              block_offsets, expert_end, row_map, round_scale, stream, ue8m0)
        assert round_scale and not ue8m0, 'MXFP8 scale factors are power-of-two factors: round_scale, not ue8m0'
        assert x_direct is not None and sf_direct is None
        x = _bf16_rows(x_direct, 'dispatch_copy_cast')
        H = x.shape[1]
        assert recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and \
            recv_x_bytes.shape[1] == H, 'dispatch_copy_cast writes contiguous bytes [rows, H]'
        assert recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and \
            tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 32), \
            'dispatch_copy_cast(mx) writes contiguous bytes [rows, H / 32]'
        q_bytes, sf_bytes = _mx_bytes(x)
        self.dispatch_copy(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=q_bytes, sf_direct=sf_bytes, num_max_tokens=num_max_tokens,
                           error_flag=error_flag, inv=inv, block_offsets=block_offsets, expert_end=expert_end,
                           row_map=row_map)


MX = dict(cast_to_fp8=True, fp8_round_scale=True, fp8_use_ue8m0=True, fp8_group_size=32)


def compare_mx(buf, xin, **kw):
    """The differences between dispatch(xin, the MX flags, **kw) and dispatch(mx_pair(xin), **kw), and the keyword
    result."""
    got = buf.dispatch(xin, **MX, **kw)
    want = buf.dispatch(mx_pair(xin), **kw)
    bad = packed_differences(got, want)
    if not (isinstance(got[0], tuple) and got[0][0].dtype == torch.float8_e4m3fn and got[0][1].dtype == torch.uint8 and
            got[0][1].shape[1] == xin.shape[1] // 32):
        bad.append('recv_x is not the (float8_e4m3fn [rows, H], uint8 [rows, H / 32]) pair')
    return bad, got


def mx_cases(buf, inputs, empty_inputs, num_experts: int):
    """tests/ue8m0_ref.ue8m0_cases for the MX flags: dispatch(x, cast_to_fp8=True, fp8_round_scale=True,
    fp8_use_ue8m0=True, fp8_group_size=32, ...) against the tuple dispatch of mx_pair(x) on the same buffer, in every
    mode the keyword composes with.  Returns the differences."""
    fails = []
    x, idx, w = inputs
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def compare(label, xin, **kw):
        bad, got = compare_mx(buf, xin, **kw)
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
    # a cached handle remembers nothing about dtypes: a bf16 dispatch's handle and an MX casting dispatch's handle
    # both serve a cached MX dispatch
    for more in (dict(), dict(do_expand=True), dict(do_cpu_sync=False)):
        h_bf16 = buf.dispatch(x, **more, **base)[3]
        h_cast = buf.dispatch(x, **MX, **more, **base)[3]
        expand = dict(do_expand=h_bf16.do_expand)
        compare(f'cached on a bf16 handle ({more})', x, handle=h_bf16, **expand)
        compare(f'cached on an MX casting handle ({more})', x, handle=h_cast, **expand)
    x0, idx0, w0 = empty_inputs
    for expand in (False, True):
        compare(f'no tokens (expand={expand})', x0, topk_idx=idx0, topk_weights=w0, num_experts=num_experts,
                do_expand=expand)
    return fails
