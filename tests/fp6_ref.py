"""MXFP6 (OCP e2m3 rows, 32 codes to 24 bytes, one UE8M0 exponent byte per 32 columns): the torch reference of the
contract, a CPU kernel provider with the four FP6 wrappers, and the comparison of the keyword dispatch with the tuple
dispatch -- TEST INFRASTRUCTURE ONLY.

The form (include/deepep_amd.h, deepep_cast_fp6_mx): for H % 128 == 0 the rows are uint8 [rows, 3 * H / 4]; a group of
32 columns is 24 bytes, group g at bytes [24g, 24g + 24), a little-endian 192-bit string with column c in bits
6c + 5 : 6c -- columns 4j .. 4j + 3 are the 24-bit word c0 | c1 << 6 | c2 << 12 | c3 << 18 in bytes 3j .. 3j + 2 (the
order of gfx950's v_cvt_scalef32_pk32_fp6_bf16).  A code is s ee mmm.  The scale factors are uint8 [rows, H / 32], byte
g the biased exponent of column group g under the ceiling rule with 7.5 in place of 448.  The cast back multiplies
fp32(code) by float_from_bits(byte << 23)."""
import torch

from tests.fp8_oracle_kernels import _bf16_rows
from tests.mx_ref import MxOracleKernels, mx_factors
from tests.oracle_kernels import _routing
from tests.ue8m0_ref import packed_differences

# magnitude of code ee mmm: mmm / 8 for ee == 0, else (1 + mmm / 8) * 2^(ee - 1)
E2M3_VALUES = tuple((c & 7) / 8.0 if (c >> 3) == 0 else (1 + (c & 7) / 8.0) * 2.0 ** ((c >> 3) - 1) for c in range(32))
# the 31 tie points: the midpoint of magnitudes j and j + 1 (all exact in fp32); a tie goes to the even code
E2M3_TIES = tuple((E2M3_VALUES[j] + E2M3_VALUES[j + 1]) / 2 for j in range(31))


def fp6_codes(x: torch.Tensor):
    """(codes uint8 [T, H], one code 0..63 per column; exponent bytes uint8 [T, H / 32]) of a bf16 x, on the CPU: the
    contract with the threshold table."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 128 == 0
    T, H = x.shape
    v = x.cpu().float().view(T, H // 32, 32)
    amax = v.abs().amax(dim=2).clamp(min=1e-4)
    bits = (amax * torch.tensor(1.0 / 7.5, dtype=torch.float32)).view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    m = v.abs() * ((127 - e) << 23).view(torch.float32).unsqueeze(2)
    code = torch.zeros(m.shape, dtype=torch.uint8)
    for j, t in enumerate(E2M3_TIES):
        # past the midpoint of codes j and j + 1; at the midpoint itself only towards an even j + 1
        code += ((m >= t) if j & 1 else (m > t)).to(torch.uint8)
    sign = (x.cpu().contiguous().view(torch.int16).view(T, H // 32, 32) < 0).to(torch.uint8) << 5
    return (code | sign).view(T, H), (e + 127).to(torch.uint8)


def fp6_pack(codes: torch.Tensor) -> torch.Tensor:
    """uint8 [T, H] codes -> uint8 [T, 3 * H / 4] rows: four codes to three bytes, little-endian."""
    T, H = codes.shape
    c = codes.to(torch.int32).view(T, H // 4, 4)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack([word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff], dim=2).to(torch.uint8).view(T, 3 * H // 4)


def fp6_unpack(q: torch.Tensor) -> torch.Tensor:
    """uint8 [M, 3 * H / 4] rows (any strides) -> int64 [M, H] codes."""
    b = torch.empty(q.shape, dtype=torch.uint8).copy_(q.cpu()).to(torch.int64)
    M, n = b.shape
    b = b.view(M, n // 3, 3)
    word = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(word >> (6 * k)) & 63 for k in range(4)], dim=2).view(M, n // 3 * 4)


def fp6_pair(x: torch.Tensor):
    """(q uint8 [T, 3 * H / 4], sf uint8 [T, H / 32]) of a bf16 x, on the device of x."""
    codes, sf = fp6_codes(x)
    return fp6_pack(codes).to(x.device), sf.to(x.device)


def fp6_back_ref(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """bf16 [M, H] of an MXFP6 pair (rows uint8 [M, 3 * H / 4], scale factors uint8 / float8_e8m0fnu [M, H / 32] of
    any strides) on the CPU: bf16_rne(fp32(code) * float_from_bits(byte << 23))."""
    codes = fp6_unpack(q)
    M, H = codes.shape
    value = torch.tensor(E2M3_VALUES, dtype=torch.float32)[codes & 31]
    value = torch.where((codes & 32) != 0, -value, value)
    out = value.view(M, H // 32, 32) * mx_factors(sf).unsqueeze(2)
    return out.view(M, H).to(torch.bfloat16)


class Fp6OracleKernels(MxOracleKernels):
    """MxOracleKernels with the four wrappers of deepep_amd.kernels.Fp6Kernels: they assert what the HIP wrappers
    require and hand the fp6_pair bytes to the parent's dispatch_pack / dispatch_copy."""
    name = 'oracle-fp6'

    def cast_fp6(self, x, q, sf, stream=None, store_bytes=None):
        assert x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1)
        T, H = x.shape
        assert H % 128 == 0 and H > 0 and store_bytes in (None, 8, 16)
        assert q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (T, 3 * H // 4)
        assert sf.dtype == torch.uint8 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 32)
        q_ref, sf_ref = fp6_pair(x)
        q.copy_(q_ref)
        sf.copy_(sf_ref)

    def cast_back_fp6(self, q, sf, out, stream=None):
        assert q.dim() == 2 and q.dtype == torch.uint8 and (q.numel() == 0 or q.stride(1) == 1)
        assert q.shape[1] % 96 == 0 and q.shape[1] > 0
        M, H = q.shape[0], q.shape[1] // 3 * 4
        assert tuple(sf.shape) == (M, H // 32)
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, H)
        out.copy_(fp6_back_ref(q, sf))

    def dispatch_pack_cast_fp6(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed, layout,
                               dest_bases=None, dest_rows=None, error_flag=None, stream=None):
        _routing(topk_idx)
        x = _bf16_rows(x_bytes, 'dispatch_pack_cast_fp6')
        H = x.shape[1]
        assert layout.x_bytes == 3 * H // 4 and layout.sf_bytes == H // 32, \
            'dispatch_pack_cast_fp6 needs the row layout RowLayout.make(3 * H / 4, H / 32, K)'
        q_bytes, sf_bytes = fp6_pair(x)
        self.dispatch_pack(q_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout, dest_bases=dest_bases, dest_rows=dest_rows, error_flag=error_flag)

    def dispatch_copy_cast_fp6(self, packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                               x_direct=None, sf_direct=None, num_max_tokens=0, error_flag=None, inv=None,
                               block_offsets=None, expert_end=None, row_map=None, stream=None):
        assert x_direct is not None and sf_direct is None
        x = _bf16_rows(x_direct, 'dispatch_copy_cast_fp6')
        H = x.shape[1]
        assert recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and \
            recv_x_bytes.shape[1] == 3 * H // 4, 'dispatch_copy_cast_fp6 writes contiguous bytes [rows, 3 * H / 4]'
        assert recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and \
            tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 32), \
            'dispatch_copy_cast_fp6 writes contiguous bytes [rows, H / 32]'
        q_bytes, sf_bytes = fp6_pair(x)
        self.dispatch_copy(packed, layout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes, recv_w,
                           x_direct=q_bytes, sf_direct=sf_bytes, num_max_tokens=num_max_tokens,
                           error_flag=error_flag, inv=inv, block_offsets=block_offsets, expert_end=expert_end,
                           row_map=row_map)


FP6 = dict(cast_to_fp6=True)
FP6_WRAPPERS = ('cast_fp6', 'cast_back_fp6', 'dispatch_pack_cast_fp6', 'dispatch_copy_cast_fp6')


def compare_fp6(buf, xin, **kw):
    """The differences between dispatch(xin, cast_to_fp6=True, **kw) and dispatch(fp6_pair(xin), **kw), and the
    keyword result."""
    got = buf.dispatch(xin, **FP6, **kw)
    want = buf.dispatch(fp6_pair(xin), **kw)
    bad = packed_differences(got, want)
    if not (isinstance(got[0], tuple) and got[0][0].dtype == torch.uint8 and got[0][1].dtype == torch.uint8 and
            got[0][0].shape[1] == 3 * xin.shape[1] // 4 and got[0][1].shape[1] == xin.shape[1] // 32):
        bad.append('recv_x is not the (uint8 [rows, 3 * H / 4], uint8 [rows, H / 32]) pair')
    return bad, got


def fp6_cases(buf, inputs, empty_inputs, num_experts: int):
    """tests/fp4_ref.fp4_cases for cast_to_fp6: dispatch(x, cast_to_fp6=True, ...) against the tuple dispatch of
    fp6_pair(x) on the same buffer, in every mode the FP4 keyword composes with.  Returns the differences."""
    fails = []
    x, idx, w = inputs
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def compare(label, xin, **kw):
        bad, got = compare_fp6(buf, xin, **kw)
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
    # a cached handle remembers nothing about dtypes: a bf16 dispatch's handle and an FP6 casting dispatch's handle
    # both serve a cached FP6 dispatch
    for more in (dict(), dict(do_expand=True), dict(do_cpu_sync=False)):
        h_bf16 = buf.dispatch(x, **more, **base)[3]
        h_cast = buf.dispatch(x, **FP6, **more, **base)[3]
        expand = dict(do_expand=h_bf16.do_expand)
        compare(f'cached on a bf16 handle ({more})', x, handle=h_bf16, **expand)
        compare(f'cached on an FP6 casting handle ({more})', x, handle=h_cast, **expand)
    x0, idx0, w0 = empty_inputs
    for expand in (False, True):
        compare(f'no tokens (expand={expand})', x0, topk_idx=idx0, topk_weights=w0, num_experts=num_experts,
                do_expand=expand)
    return fails
