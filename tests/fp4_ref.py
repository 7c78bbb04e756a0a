"""MXFP4 (OCP e2m1 rows, two codes to a byte, one UE8M0 exponent byte per 32 columns): the torch reference of the
contract, a CPU kernel provider with the four FP4 wrappers, and the comparison of the keyword dispatch with the tuple
dispatch -- TEST INFRASTRUCTURE ONLY.

The form (include/deepep_amd.h, deepep_cast_fp4_mx): for H % 128 == 0 the rows are uint8 [rows, H / 2], byte j the
codes of columns 2j (bits 3:0) and 2j + 1 (bits 7:4); the scale factors are uint8 [rows, H / 32], byte g the biased
exponent of column group g under the ceiling rule with 6 in place of 448.  The cast back multiplies fp32(code) by
float_from_bits(byte << 23)."""
import torch

from tests.fp8_oracle_kernels import _bf16_rows
from tests.mx_ref import MxOracleKernels, mx_factors
from tests.oracle_kernels import _routing
from tests.ue8m0_ref import packed_differences

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def fp4_codes(x: torch.Tensor):
    """(codes uint8 [T, H], one code 0..15 per column; exponent bytes uint8 [T, H / 32]) of a bf16 x, on the CPU: the
    contract with the threshold table."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 128 == 0
    T, H = x.shape
    v = x.cpu().float().view(T, H // 32, 32)
    amax = v.abs().amax(dim=2).clamp(min=1e-4)
    bits = (amax * torch.tensor(1.0 / 6.0, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    m = v.abs() * ((127 - e) << 23).view(torch.float32).unsqueeze(2)
    code = ((m > 0.25).to(torch.uint8) + (m >= 0.75).to(torch.uint8) + (m > 1.25).to(torch.uint8) +
            (m >= 1.75).to(torch.uint8) + (m > 2.5).to(torch.uint8) + (m >= 3.5).to(torch.uint8) +
            (m > 5.0).to(torch.uint8))
    sign = (x.cpu().contiguous().view(torch.int16).view(T, H // 32, 32) < 0).to(torch.uint8) << 3
    return (code | sign).view(T, H), (e + 127).to(torch.uint8)


def fp4_pack(codes: torch.Tensor) -> torch.Tensor:
    """uint8 [T, H] codes -> uint8 [T, H / 2] rows (torch.float4_e2m1fn_x2's order)."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def fp4_pair(x: torch.Tensor):
    """(q uint8 [T, H / 2], sf uint8 [T, H / 32]) of a bf16 x, on the device of x."""
    codes, sf = fp4_codes(x)
    return fp4_pack(codes).to(x.device), sf.to(x.device)


def fp4_back_ref(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """bf16 [M, H] of an MXFP4 pair (rows uint8 / float4_e2m1fn_x2 [M, H / 2], scale factors uint8 / float8_e8m0fnu
    [M, H / 32] of any strides) on the CPU: bf16_rne(fp32(code) * float_from_bits(byte << 23))."""
    b = torch.empty(q.shape, dtype=torch.uint8).copy_(q.cpu().view(torch.uint8))
    M, H = b.shape[0], b.shape[1] * 2
    codes = torch.stack([b & 0xf, b >> 4], dim=2).view(M, H).to(torch.int64)
    value = torch.tensor(E2M1_VALUES, dtype=torch.float32)[codes & 7]
    value = torch.where((codes & 8) != 0, -value, value)
    out = value.view(M, H // 32, 32) * mx_factors(sf).unsqueeze(2)
    return out.view(M, H).to(torch.bfloat16)


class Fp4OracleKernels(MxOracleKernels):
    """MxOracleKernels with the four wrappers of deepep_amd.kernels.Fp4Kernels: they assert what the HIP wrappers
    require and hand the fp4_pair bytes to the parent's dispatch_pack / dispatch_copy."""
    name = 'oracle-fp4'

    def cast_fp4(self, x, q, sf, stream=None):
        assert x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1)
        T, H = x.shape
        assert H % 128 == 0 and H > 0
        assert q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (T, H // 2)
        assert sf.dtype == torch.uint8 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 32)
        q_ref, sf_ref = fp4_pair(x)
        q.copy_(q_ref)
        sf.copy_(sf_ref)

    def cast_back_fp4(self, q, sf, out, stream=None):
        assert q.dim() == 2 and (q.numel() == 0 or q.stride(1) == 1)
        M, H = q.shape[0], q.shape[1] * 2
        assert H % 128 == 0 and H > 0 and tuple(sf.shape) == (M, H // 32)
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, H)
        out.copy_(fp4_back_ref(q, sf))

    def dispatch_pack_cast_fp4(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed, layout,
                               dest_bases=None, dest_rows=None, error_flag=None, stream=None):
        _routing(topk_idx)
        x = _bf16_rows(x_bytes, 'dispatch_pack_cast_fp4')
        H = x.shape[1]
        assert layout.x_bytes == H // 2 and layout.sf_bytes == H // 32, \
            'dispatch_pack_cast_fp4 needs the row layout RowLayout.make(H / 2, H / 32, K)'
        q_bytes, sf_bytes = fp4_pair(x)
        self.dispatch_pack(q_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout, dest_bases=dest_bases, dest_rows=dest_rows, error_flag=error_flag)

    def dispatch_copy_cast_fp4(self, packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                               x_direct=None, sf_direct=None, num_max_tokens=0, error_flag=None, inv=None,
                               block_offsets=None, expert_end=None, row_map=None, stream=None):
        assert x_direct is not None and sf_direct is None
        x = _bf16_rows(x_direct, 'dispatch_copy_cast_fp4')
        H = x.shape[1]
        assert recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and \
            recv_x_bytes.shape[1] == H // 2, 'dispatch_copy_cast_fp4 writes contiguous bytes [rows, H / 2]'
        assert recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and \
            tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 32), \
            'dispatch_copy_cast_fp4 writes contiguous bytes [rows, H / 32]'
        q_bytes, sf_bytes = fp4_pair(x)
        self.dispatch_copy(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=q_bytes, sf_direct=sf_bytes, num_max_tokens=num_max_tokens,
                           error_flag=error_flag, inv=inv, block_offsets=block_offsets, expert_end=expert_end,
                           row_map=row_map)


FP4 = dict(cast_to_fp4=True)
FP4_WRAPPERS = ('cast_fp4', 'cast_back_fp4', 'dispatch_pack_cast_fp4', 'dispatch_copy_cast_fp4')


def compare_fp4(buf, xin, **kw):
    """The differences between dispatch(xin, cast_to_fp4=True, **kw) and dispatch(fp4_pair(xin), **kw), and the
    keyword result."""
    got = buf.dispatch(xin, **FP4, **kw)
    want = buf.dispatch(fp4_pair(xin), **kw)
    bad = packed_differences(got, want)
    if not (isinstance(got[0], tuple) and got[0][0].dtype == torch.uint8 and got[0][1].dtype == torch.uint8 and
            got[0][0].shape[1] == xin.shape[1] // 2 and got[0][1].shape[1] == xin.shape[1] // 32):
        bad.append('recv_x is not the (uint8 [rows, H / 2], uint8 [rows, H / 32]) pair')
    return bad, got


def fp4_cases(buf, inputs, empty_inputs, num_experts: int):
    """tests/mx_ref.mx_cases for cast_to_fp4: dispatch(x, cast_to_fp4=True, ...) against the tuple dispatch of
    fp4_pair(x) on the same buffer, in every mode the keyword composes with.  Returns the differences."""
    fails = []
    x, idx, w = inputs
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def compare(label, xin, **kw):
        bad, got = compare_fp4(buf, xin, **kw)
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
    # a cached handle remembers nothing about dtypes: a bf16 dispatch's handle and an FP4 casting dispatch's handle
    # both serve a cached FP4 dispatch
    for more in (dict(), dict(do_expand=True), dict(do_cpu_sync=False)):
        h_bf16 = buf.dispatch(x, **more, **base)[3]
        h_cast = buf.dispatch(x, **FP4, **more, **base)[3]
        expand = dict(do_expand=h_bf16.do_expand)
        compare(f'cached on a bf16 handle ({more})', x, handle=h_bf16, **expand)
        compare(f'cached on an FP4 casting handle ({more})', x, handle=h_cast, **expand)
    x0, idx0, w0 = empty_inputs
    for expand in (False, True):
        compare(f'no tokens (expand={expand})', x0, topk_idx=idx0, topk_weights=w0, num_experts=num_experts,
                do_expand=expand)
    return fails
