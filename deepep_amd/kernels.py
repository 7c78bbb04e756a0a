"""Tensor-level wrappers over the C-ABI (deepep_amd/_lib.py).

`HipKernels` is the only kernel provider the product uses.  It accepts torch
tensors, checks dtypes/shapes/devices on the host (the checks of
csrc/elastic/buffer.hpp:1200-1247 in the reference that concern the kernels), and
passes raw device pointers plus the stream handle to libdeepep_amd.so.
"""
from dataclasses import dataclass
from types import MappingProxyType
from typing import Optional

import torch

from . import _lib
from ._lib import MODE_EPILOGUE, MODE_FUSED, MODE_LOCAL, ptr
from .utils import align

__all__ = ['HipKernels', 'RowLayout', 'MODE_LOCAL', 'MODE_EPILOGUE', 'MODE_FUSED']


@dataclass(frozen=True)
class RowLayout:
    """Byte layout of one packed dispatch row (include/deepep_amd.h, dispatch section)."""
    x_bytes: int
    sf_bytes: int
    num_topk: int
    sf_off: int
    idx_off: int
    w_off: int
    src_off: int
    row_bytes: int

    @staticmethod
    def make(x_bytes: int, sf_bytes: int, num_topk: int) -> 'RowLayout':
        sf_off = x_bytes
        idx_off = align(sf_off + sf_bytes, 16)
        w_off = idx_off + align(num_topk * 8, 16)
        src_off = w_off + align(num_topk * 4, 16)
        # rows are whole 128-byte lines, so every row (and its x bytes) starts on a line
        return RowLayout(x_bytes, sf_bytes, num_topk, sf_off, idx_off, w_off, src_off, align(src_off + 16, 128))


def _require(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(f'deepep_amd: {msg}')


def _stream_handle(stream) -> int:
    return stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream


# the dtypes of MXFP8 scale factors: one UE8M0 exponent byte per 32 columns
MX_SF_DTYPES = (torch.uint8,) + ((torch.float8_e8m0fnu,) if hasattr(torch, 'float8_e8m0fnu') else ())


@dataclass(frozen=True, eq=False)       # three instances, compared by identity
class SfFormat:
    """One FP8 scale-factor format: all that the wrappers below, ElasticBuffer.dispatch and the package's
    per_token_cast_* know about it (the kernels' side: SfFormat<> in csrc/fp8_cast.hip)."""
    name: str                       # in error texts
    suffix: str                     # of its C entries deepep_{cast_fp8,cast_back_fp8,dispatch_{pack,copy}_cast}
    dtype: torch.dtype              # a row of H columns has H / elem_cols scale-factor elements of it
    elem_cols: int
    multiple: int                   # H is a multiple of it
    needs_round_scale: bool         # power-of-two factors only; the C entries then take no round_scale argument
    kw: MappingProxyType            # the keyword the wrappers take for it (passed only when it is on), read-only

    def elems(self, H: int) -> int:
        return H // self.elem_cols

    def row_bytes(self, H: int) -> int:
        return self.elems(H) * self.dtype.itemsize

    def __str__(self) -> str:
        return f'{self.name} scale factors {self.dtype} [rows, H / {self.elem_cols}]'

    def require(self, what: str, H: int, round_scale) -> None:
        _require(H % self.multiple == 0 and (bool(round_scale) or not self.needs_round_scale),
                 f'{what} needs a hidden size that is a multiple of {self.multiple}' +
                 (f' and round_scale for {self.name} scale factors' if self.needs_round_scale else ''))

    def scale_arg(self, round_scale) -> tuple:
        return () if self.needs_round_scale else (int(round_scale),)


SF_FP32 = SfFormat('float32', '', torch.float32, 128, 128, False, MappingProxyType({}))
SF_UE8M0 = SfFormat('packed UE8M0', '_ue8m0', torch.int32, 512, 512, True, MappingProxyType({'ue8m0': True}))
SF_MXFP8 = SfFormat('MXFP8', '_mx', torch.uint8, 32, 128, True, MappingProxyType({'mx': True}))
SF_FORMATS = (SF_FP32, SF_UE8M0, SF_MXFP8)


def sf_format(ue8m0: bool = False, mx: bool = False, what: str = 'the FP8 cast') -> SfFormat:
    """The format the wrappers' keywords name."""
    _require(not (mx and ue8m0), f'{what}: mx (a byte per 32 columns) and ue8m0 (a byte per 128) exclude each other')
    return SF_MXFP8 if mx else SF_UE8M0 if ue8m0 else SF_FP32


def sf_format_of(dtype) -> Optional[SfFormat]:
    """The format a scale-factor tensor of this dtype is in (None: not a scale-factor dtype)."""
    return SF_MXFP8 if dtype in MX_SF_DTYPES else {torch.int32: SF_UE8M0, torch.float32: SF_FP32}.get(dtype)


def _fp8_source(src: torch.Tensor, sf: torch.Tensor, what: str):
    """The checks of cast_back_fp8 on an FP8 source pair (src float8_e4m3fn [M, H], rows may be strided; sf float32
    [M, H / 128] or int32 [M, H / 512] of any strides): (sf pointer, row stride, column stride, packed) for the
    *_fp8 entries.  MXFP8 scale factors (uint8 / float8_e8m0fnu) are not a source of these entries."""
    _require(src.is_cuda and src.dim() == 2 and src.dtype == torch.float8_e4m3fn and
             (src.numel() == 0 or src.stride(1) == 1),
             f'{what} FP8 source must be 2-D float8_e4m3fn on the GPU with unit column stride')
    M, H = src.shape
    _require(H % 128 == 0 and H > 0, f'{what} needs a hidden size that is a multiple of 128 for an FP8 source')
    _require(M == 0 or src.stride(0) % 16 == 0, f'{what} FP8 source rows must be a multiple of 16 bytes apart')
    _require(isinstance(sf, torch.Tensor) and sf.is_cuda and sf.device == src.device,
             f'{what} scale factors must be on the GPU of the FP8 source')
    fmt = sf_format_of(sf.dtype)
    _require(fmt is not SF_MXFP8,
             f'{what} does not take MXFP8 (per-32-column) scale factors: use cast_back_fp8 on the pair first')
    _require(fmt is not None and H % fmt.multiple == 0 and tuple(sf.shape) == (M, fmt.elems(H)),
             f'{what} takes float32 [M, H / 128] or packed UE8M0 int32 [M, H / 512] (H % 512 == 0) scale factors')
    return ptr(sf), sf.stride(0), sf.stride(1), int(fmt is SF_UE8M0)


def _logfmt_pair(planes, meta, H: int, what: str) -> int:
    """The checks on a LogFMT pair of H columns (planes uint8 [M, H * 5 / 4], meta int32 [M, H / 128], rows of both
    may be strided): M."""
    _require(H % 128 == 0 and H > 0, f'{what} needs a hidden size that is a multiple of 128 for LogFMT rows')
    _require(isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dim() == 2 and
             planes.dtype == torch.uint8 and planes.shape[1] == H * 5 // 4 and
             (planes.numel() == 0 or planes.stride(1) == 1),
             f'{what} LogFMT planes must be 2-D uint8 [M, H * 5 / 4] on the GPU with unit column stride')
    M = planes.shape[0]
    _require(isinstance(meta, torch.Tensor) and meta.is_cuda and meta.device == planes.device and
             meta.dtype == torch.int32 and tuple(meta.shape) == (M, H // 128) and
             (meta.numel() == 0 or meta.stride(1) == 1),
             f'{what} LogFMT meta must be int32 [M, H / 128] on the GPU of the planes with unit column stride')
    _require(M == 0 or (planes.stride(0) % 16 == 0 and planes.data_ptr() % 16 == 0 and meta.stride(0) >= H // 128),
             f'{what} LogFMT rows must start 16-byte aligned')
    return M


def _table_view(table: Optional[torch.Tensor]):
    """(tensor, row stride in elements, width) of a 2-D int32 table view (rows may be strided)."""
    if table is None:
        return None, 0, 1
    _require(table.dim() == 2 and table.dtype == torch.int32 and table.stride(1) == 1,
             'slot tables must be 2-D int32 with unit column stride')
    return table, table.stride(0), table.shape[1]


class LogfmtKernels:
    """The LogFMT-10 codec wrappers of HipKernels (csrc/logfmt.hip; the format: csrc/logfmt_codec.h).  Only a
    combine(use_logfmt=True) and the package's per_token_cast_*_logfmt call them."""

    def cast_logfmt(self, x, planes, meta, stream=None):
        """The LogFMT-10 encode: x bf16 [T, H] (rows may be strided), H % 128 == 0 -> planes uint8 [T, H * 5 / 4]
        ([low | high]) and meta int32 [T, H / 128], both contiguous."""
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 'cast_logfmt input must be 2-D bf16 on the GPU with unit column stride')
        T, H = x.shape
        _require(H % 128 == 0 and H > 0, 'cast_logfmt needs a hidden size that is a multiple of 128')
        _require(planes.is_cuda and planes.dtype == torch.uint8 and planes.is_contiguous() and
                 tuple(planes.shape) == (T, H * 5 // 4) and meta.is_cuda and meta.dtype == torch.int32 and
                 meta.is_contiguous() and tuple(meta.shape) == (T, H // 128),
                 'cast_logfmt outputs must be contiguous uint8 [rows, H * 5 / 4] and int32 [rows, H / 128] on the GPU')
        self._entry('cast_logfmt')(ptr(x), x.stride(0) * 2 if T else H * 2, T, H, ptr(planes), ptr(meta),
                                   _stream_handle(stream))

    def cast_back_logfmt(self, planes, meta, out, stream=None):
        """The LogFMT-10 decode: planes uint8 [M, H * 5 / 4] and meta int32 [M, H / 128] (rows of both may be
        strided) -> out bf16 [M, H], contiguous."""
        _require(out.is_cuda and out.dim() == 2 and out.dtype == torch.bfloat16 and out.is_contiguous(),
                 'cast_back_logfmt output must be contiguous bf16 [M, H] on the GPU')
        H = out.shape[1]
        M = _logfmt_pair(planes, meta, H, 'cast_back_logfmt')
        _require(out.shape[0] == M, 'cast_back_logfmt output must have the rows of its input')
        self._entry('cast_back_logfmt')(ptr(planes), planes.stride(0) if M else H * 5 // 4, ptr(meta),
                                        meta.stride(0) if M else H // 128, M, H, ptr(out), _stream_handle(stream))

    def logfmt_pack_rows(self, src, num_rows, hidden, dst, src_tail_offset: int = 0, dst_tail_offset: int = 0,
                         tail_bytes: int = 0, stream=None):
        """The first num_rows packed exchange rows of src (2-D, contiguous, [bf16 row | weight tail at byte
        src_tail_offset], handle.packed_row_layout) as wire rows of dst (2-D, contiguous, [low | high | meta | pad |
        weight tail at byte dst_tail_offset], handle.logfmt_row_layout); tail_bytes of the tail are copied."""
        for t, name in ((src, 'source'), (dst, 'destination')):
            _require(t.is_cuda and t.dim() == 2 and t.is_contiguous(),
                     f'logfmt_pack_rows {name} rows must be 2-D and contiguous on the GPU')
            _require(t.shape[0] >= num_rows >= 0, f'logfmt_pack_rows: fewer {name} rows than num_rows')
        _require(hidden % 128 == 0 and hidden > 0, 'logfmt_pack_rows needs a hidden size that is a multiple of 128')
        src_bytes, dst_bytes = src.shape[1] * src.element_size(), dst.shape[1] * dst.element_size()
        if not tail_bytes:
            src_tail_offset, dst_tail_offset = src_bytes, dst_bytes
        _require(hidden * 2 <= src_tail_offset and src_tail_offset + tail_bytes <= src_bytes and
                 hidden * 5 // 4 + hidden // 32 <= dst_tail_offset and dst_tail_offset + tail_bytes <= dst_bytes,
                 'logfmt_pack_rows: the rows are too short for hidden and the weight tail')
        self._entry('logfmt_pack_rows')(ptr(src), src_bytes, src_tail_offset, num_rows, hidden, tail_bytes,
                                        ptr(dst), dst_bytes, dst_tail_offset, _stream_handle(stream))


# the dtypes of MXFP4 rows: two e2m1 codes to a byte
FP4_ROW_DTYPES = (torch.uint8,) + ((torch.float4_e2m1fn_x2,) if hasattr(torch, 'float4_e2m1fn_x2') else ())


class Fp4Kernels:
    """The MXFP4 wrappers of HipKernels (csrc/fp4_cast.hip; the format: include/deepep_amd.h, deepep_cast_fp4_mx): rows
    of H / 2 bytes, byte j the e2m1 codes of columns 2j (bits 3:0) and 2j + 1 (bits 7:4), and MXFP8's scale factors,
    one UE8M0 exponent byte per 32 columns.  Only a dispatch(cast_to_fp4=True) and the package's per_token_cast_*_fp4
    call them."""

    def cast_fp4(self, x, q, sf, stream=None):
        """The MXFP4 cast: x bf16 [T, H] (rows may be strided), H % 128 == 0 -> q uint8 [T, H / 2] and sf uint8
        [T, H / 32], both contiguous."""
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 'cast_fp4 input must be 2-D bf16 on the GPU with unit column stride')
        T, H = x.shape
        _require(H % 128 == 0 and H > 0, 'cast_fp4 needs a hidden size that is a multiple of 128')
        _require(q.is_cuda and q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (T, H // 2) and
                 sf.is_cuda and sf.dtype == torch.uint8 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 32),
                 'cast_fp4 outputs must be contiguous uint8 [rows, H / 2] and uint8 [rows, H / 32] on the GPU')
        self._entry('cast_fp4_mx')(ptr(x), x.stride(0) * 2 if T else H * 2, T, H, ptr(q), ptr(sf),
                                   _stream_handle(stream))

    def cast_back_fp4(self, q, sf, out, stream=None):
        """The inverse of cast_fp4: q uint8 / float4_e2m1fn_x2 [M, H / 2] (rows may be strided), sf uint8 /
        float8_e8m0fnu [M, H / 32] of any strides (column-major scale factors are read in place) -> out bf16 [M, H],
        contiguous: bf16(fp32(code) * float_from_bits(byte << 23))."""
        _require(q.is_cuda and q.dim() == 2 and q.dtype in FP4_ROW_DTYPES and (q.numel() == 0 or q.stride(1) == 1),
                 'cast_back_fp4 input must be 2-D uint8 / float4_e2m1fn_x2 on the GPU with unit column stride')
        M, H = q.shape[0], q.shape[1] * 2
        _require(H % 128 == 0 and H > 0, 'cast_back_fp4 needs a hidden size that is a multiple of 128')
        _require(M == 0 or (q.stride(0) % 16 == 0 and q.data_ptr() % 16 == 0),
                 'cast_back_fp4 rows must start 16-byte aligned')
        _require(sf.is_cuda and sf.dtype in MX_SF_DTYPES and tuple(sf.shape) == (M, H // 32),
                 'cast_back_fp4 takes uint8 / float8_e8m0fnu [M, H / 32] scale factors on the GPU')
        _require(sf.data_ptr() % 4 == 0 and (sf.stride(1) != 1 or sf.stride(0) % 4 == 0),
                 'cast_back_fp4 scale factors must start 4-byte aligned, as must rows of unit column stride')
        _require(out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, H),
                 'cast_back_fp4 output must be contiguous bf16 [M, H] on the GPU')
        self._entry('cast_back_fp4_mx')(ptr(q), q.stride(0) if M else H // 2, ptr(sf), sf.stride(0), sf.stride(1),
                                        M, H, ptr(out), _stream_handle(stream))

    def dispatch_pack_cast_fp4(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                               layout: RowLayout, dest_bases=None, dest_rows: Optional[int] = None, error_flag=None,
                               stream=None):
        """dispatch_pack with cast_fp4 fused in: x_bytes is the uint8 view [T, 2 * H] of the tokens' bf16 rows, layout
        the MXFP4 row layout RowLayout.make(H / 2, H / 32, K); the packed rows get the codes and the exponent bytes.
        The other arguments as dispatch_pack."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        H = layout.x_bytes * 2
        _require(H % 128 == 0 and H > 0, 'dispatch_pack_cast_fp4 needs a hidden size that is a multiple of 128')
        _require(layout.sf_bytes == H // 32 and x_bytes.dtype == torch.uint8 and x_bytes.dim() == 2 and
                 x_bytes.shape[1] == 2 * H,
                 'dispatch_pack_cast_fp4 needs bf16 rows of H columns and the row layout '
                 'RowLayout.make(H / 2, H / 32, K)')
        if dest_bases is not None:
            _require(dest_bases.is_cuda and dest_bases.dtype == torch.int64 and dest_bases.is_contiguous() and
                     dest_bases.numel() == dst_slot.shape[1], 'dest_bases must be int64 [num_ranks] on the GPU')
            _require(dest_rows is not None, 'dest_rows (rows per destination window) is required with dest_bases')
        else:
            dest_rows = packed.shape[0] if dest_rows is None else min(dest_rows, packed.shape[0])
        self._entry('dispatch_pack_cast_fp4_mx')(
            ptr(x_bytes), x_bytes.stride(0) if T else 2 * H, H,
            ptr(topk_idx), ptr(topk_weights), T, K, src_base, ptr(dst_slot), ptr(send_offsets),
            dst_slot.shape[1], ptr(packed), ptr(dest_bases), layout.row_bytes, int(dest_rows), layout.sf_off,
            layout.idx_off, layout.w_off, layout.src_off, ptr(error_flag), _stream_handle(stream))

    def dispatch_copy_cast_fp4(self, packed, layout: RowLayout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                               recv_w, x_direct=None, sf_direct=None, num_max_tokens: int = 0, error_flag=None,
                               inv=None, block_offsets=None, expert_end=None, row_map=None, stream=None):
        """dispatch_copy's one-rank (x_direct) forms with cast_fp4 fused in: x_direct is the uint8 view [T, 2 * H] of
        the sender's bf16 rows (rows may be strided) and there is no sf_direct; recv_x_bytes [rows, H / 2] gets the
        codes, recv_sf_bytes [rows, H / 32] the exponent bytes.  The other arguments as dispatch_copy."""
        _require(x_direct is not None and sf_direct is None and x_direct.dtype == torch.uint8 and x_direct.dim() == 2,
                 'dispatch_copy_cast_fp4 reads the bf16 rows of x_direct and takes no sf_direct')
        H = x_direct.shape[1] // 2
        _require(H % 128 == 0 and x_direct.shape[1] == 2 * H and (x_direct.numel() == 0 or x_direct.stride(1) == 1),
                 'dispatch_copy_cast_fp4 needs bf16 rows of H % 128 == 0 columns with unit column stride')
        _require(recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and
                 recv_x_bytes.shape[1] == H // 2 and recv_sf_bytes is not None and
                 recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and
                 tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 32),
                 'dispatch_copy_cast_fp4 outputs must be contiguous bytes [rows, H / 2] and [rows, H / 32]')
        if inv is not None:
            _require(expanded and block_offsets is not None and expert_end is not None and
                     block_offsets.dim() == 2 and block_offsets.shape[0] ==
                     (num_recv + _lib.DISPATCH_BLOCK_ROWS - 1) // _lib.DISPATCH_BLOCK_ROWS and
                     expert_end.numel() == block_offsets.shape[1], 'blocked copy tables')
        self._entry('dispatch_copy_cast_fp4_mx')(
            ptr(packed), layout.row_bytes, layout.w_off, num_recv, layout.num_topk, ptr(meta), int(expanded),
            ptr(x_direct), x_direct.stride(0) if x_direct.shape[0] else 2 * H, H,
            num_max_tokens, ptr(recv_x_bytes), ptr(recv_sf_bytes), ptr(recv_w), recv_x_bytes.shape[0], ptr(inv),
            ptr(block_offsets), ptr(expert_end), block_offsets.shape[1] if block_offsets is not None else 0,
            ptr(row_map), ptr(error_flag), _stream_handle(stream))


class Fp6Kernels:
    """The MXFP6 wrappers of HipKernels (csrc/fp6_cast.hip; the format: include/deepep_amd.h, deepep_cast_fp6_mx): rows
    of 3 * H / 4 bytes, a group of 32 columns in 24 bytes with column c in bits 6c + 5 : 6c of that little-endian
    string (e2m3 codes; no torch dtype), and MXFP8's scale factors, one UE8M0 exponent byte per 32 columns.  Only a
    dispatch(cast_to_fp6=True) and the package's per_token_cast_*_fp6 call them."""

    def cast_fp6(self, x, q, sf, stream=None, store_bytes=None):
        """The MXFP6 cast: x bf16 [T, H] (rows may be strided), H % 128 == 0 -> q uint8 [T, 3 * H / 4] and sf uint8
        [T, H / 32], both contiguous.  store_bytes (8 or 16; measurements only): the width of the kernel's row stores,
        by default the one measured faster -- the bytes written are the same."""
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 'cast_fp6 input must be 2-D bf16 on the GPU with unit column stride')
        T, H = x.shape
        _require(H % 128 == 0 and H > 0, 'cast_fp6 needs a hidden size that is a multiple of 128')
        _require(q.is_cuda and q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (T, 3 * H // 4) and
                 sf.is_cuda and sf.dtype == torch.uint8 and sf.is_contiguous() and tuple(sf.shape) == (T, H // 32),
                 'cast_fp6 outputs must be contiguous uint8 [rows, 3 * H / 4] and uint8 [rows, H / 32] on the GPU')
        args = (ptr(x), x.stride(0) * 2 if T else H * 2, T, H, ptr(q), ptr(sf))
        if store_bytes is None:
            self._entry('cast_fp6_mx')(*args, _stream_handle(stream))
        else:
            self._entry('cast_fp6_mx_stores')(*args, int(store_bytes), _stream_handle(stream))

    def cast_back_fp6(self, q, sf, out, stream=None):
        """The inverse of cast_fp6: q uint8 [M, 3 * H / 4] (rows may be strided), sf uint8 / float8_e8m0fnu
        [M, H / 32] of any strides (column-major scale factors are read in place) -> out bf16 [M, H], contiguous:
        bf16(fp32(code) * float_from_bits(byte << 23))."""
        _require(q.is_cuda and q.dim() == 2 and q.dtype == torch.uint8 and (q.numel() == 0 or q.stride(1) == 1),
                 'cast_back_fp6 input must be 2-D uint8 on the GPU with unit column stride')
        M, H = q.shape[0], q.shape[1] // 3 * 4
        _require(q.shape[1] % 96 == 0 and H > 0, 'cast_back_fp6 needs a hidden size that is a multiple of 128')
        _require(M == 0 or (q.stride(0) % 16 == 0 and q.data_ptr() % 16 == 0),
                 'cast_back_fp6 rows must start 16-byte aligned')
        _require(sf.is_cuda and sf.dtype in MX_SF_DTYPES and tuple(sf.shape) == (M, H // 32),
                 'cast_back_fp6 takes uint8 / float8_e8m0fnu [M, H / 32] scale factors on the GPU')
        _require(sf.data_ptr() % 4 == 0 and (sf.stride(1) != 1 or sf.stride(0) % 4 == 0),
                 'cast_back_fp6 scale factors must start 4-byte aligned, as must rows of unit column stride')
        _require(out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, H),
                 'cast_back_fp6 output must be contiguous bf16 [M, H] on the GPU')
        self._entry('cast_back_fp6_mx')(ptr(q), q.stride(0) if M else 3 * H // 4, ptr(sf), sf.stride(0), sf.stride(1),
                                        M, H, ptr(out), _stream_handle(stream))

    def dispatch_pack_cast_fp6(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                               layout: RowLayout, dest_bases=None, dest_rows: Optional[int] = None, error_flag=None,
                               stream=None):
        """dispatch_pack with cast_fp6 fused in: x_bytes is the uint8 view [T, 2 * H] of the tokens' bf16 rows, layout
        the MXFP6 row layout RowLayout.make(3 * H / 4, H / 32, K); the packed rows get the codes and the exponent
        bytes.  The other arguments as dispatch_pack."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        H = layout.x_bytes // 3 * 4
        _require(layout.x_bytes % 96 == 0 and H > 0,
                 'dispatch_pack_cast_fp6 needs a hidden size that is a multiple of 128')
        _require(layout.sf_bytes == H // 32 and x_bytes.dtype == torch.uint8 and x_bytes.dim() == 2 and
                 x_bytes.shape[1] == 2 * H,
                 'dispatch_pack_cast_fp6 needs bf16 rows of H columns and the row layout '
                 'RowLayout.make(3 * H / 4, H / 32, K)')
        if dest_bases is not None:
            _require(dest_bases.is_cuda and dest_bases.dtype == torch.int64 and dest_bases.is_contiguous() and
                     dest_bases.numel() == dst_slot.shape[1], 'dest_bases must be int64 [num_ranks] on the GPU')
            _require(dest_rows is not None, 'dest_rows (rows per destination window) is required with dest_bases')
        else:
            dest_rows = packed.shape[0] if dest_rows is None else min(dest_rows, packed.shape[0])
        self._entry('dispatch_pack_cast_fp6_mx')(
            ptr(x_bytes), x_bytes.stride(0) if T else 2 * H, H,
            ptr(topk_idx), ptr(topk_weights), T, K, src_base, ptr(dst_slot), ptr(send_offsets),
            dst_slot.shape[1], ptr(packed), ptr(dest_bases), layout.row_bytes, int(dest_rows), layout.sf_off,
            layout.idx_off, layout.w_off, layout.src_off, ptr(error_flag), _stream_handle(stream))

    def dispatch_copy_cast_fp6(self, packed, layout: RowLayout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                               recv_w, x_direct=None, sf_direct=None, num_max_tokens: int = 0, error_flag=None,
                               inv=None, block_offsets=None, expert_end=None, row_map=None, stream=None):
        """dispatch_copy's one-rank (x_direct) forms with cast_fp6 fused in: x_direct is the uint8 view [T, 2 * H] of
        the sender's bf16 rows (rows may be strided) and there is no sf_direct; recv_x_bytes [rows, 3 * H / 4] gets the
        codes, recv_sf_bytes [rows, H / 32] the exponent bytes.  The other arguments as dispatch_copy."""
        _require(x_direct is not None and sf_direct is None and x_direct.dtype == torch.uint8 and x_direct.dim() == 2,
                 'dispatch_copy_cast_fp6 reads the bf16 rows of x_direct and takes no sf_direct')
        H = x_direct.shape[1] // 2
        _require(H % 128 == 0 and x_direct.shape[1] == 2 * H and (x_direct.numel() == 0 or x_direct.stride(1) == 1),
                 'dispatch_copy_cast_fp6 needs bf16 rows of H % 128 == 0 columns with unit column stride')
        _require(recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and
                 recv_x_bytes.shape[1] == 3 * H // 4 and recv_sf_bytes is not None and
                 recv_sf_bytes.dtype == torch.uint8 and recv_sf_bytes.is_contiguous() and
                 tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], H // 32),
                 'dispatch_copy_cast_fp6 outputs must be contiguous bytes [rows, 3 * H / 4] and [rows, H / 32]')
        if inv is not None:
            _require(expanded and block_offsets is not None and expert_end is not None and
                     block_offsets.dim() == 2 and block_offsets.shape[0] ==
                     (num_recv + _lib.DISPATCH_BLOCK_ROWS - 1) // _lib.DISPATCH_BLOCK_ROWS and
                     expert_end.numel() == block_offsets.shape[1], 'blocked copy tables')
        self._entry('dispatch_copy_cast_fp6_mx')(
            ptr(packed), layout.row_bytes, layout.w_off, num_recv, layout.num_topk, ptr(meta), int(expanded),
            ptr(x_direct), x_direct.stride(0) if x_direct.shape[0] else 2 * H, H,
            num_max_tokens, ptr(recv_x_bytes), ptr(recv_sf_bytes), ptr(recv_w), recv_x_bytes.shape[0], ptr(inv),
            ptr(block_offsets), ptr(expert_end), block_offsets.shape[1] if block_offsets is not None else 0,
            ptr(row_map), ptr(error_flag), _stream_handle(stream))


class TransposedCastKernels:
    """The transposed MXFP8 cast of HipKernels (csrc/fp8_cast_t.hip; the contract: include/deepep_amd.h,
    deepep_cast_fp8_mx_transposed): the groups of 32 that share an exponent byte run along the token axis and the
    bytes are stored [H, N], the operand of a block-scaled MFMA that contracts over tokens (the weight gradient).  Only
    the package's cast_to_mxfp8_transposed calls it."""

    def cast_fp8_mx_transposed(self, x, q_t, sf_t, q=None, sf=None, stream=None):
        """x bf16 [N, H] (rows may be strided: unit column stride, row stride a multiple of 8 elements), N % 128 == 0,
        H % 128 == 0 -> q_t float8_e4m3fn [H, N] and sf_t uint8 / float8_e8m0fnu [H, N / 32], both contiguous: bit
        for bit cast_fp8(mx=True) of x.t().contiguous().  q and sf (both or neither): the same launch also writes
        cast_fp8(mx=True) of x itself, q float8_e4m3fn [N, H] and sf [N, H / 32], from the same read."""
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 'cast_fp8_mx_transposed input must be 2-D bf16 on the GPU with unit column stride')
        N, H = x.shape
        _require(H % 128 == 0 and H > 0 and N % 128 == 0,
                 'cast_fp8_mx_transposed needs a hidden size and a row count that are multiples of 128')
        _require(N == 0 or (x.stride(0) % 8 == 0 and x.stride(0) >= H and x.data_ptr() % 16 == 0),
                 'cast_fp8_mx_transposed rows must start 16-byte aligned')
        _require(q_t.is_cuda and q_t.dtype == torch.float8_e4m3fn and q_t.is_contiguous() and
                 tuple(q_t.shape) == (H, N) and sf_t.is_cuda and sf_t.dtype in MX_SF_DTYPES and
                 sf_t.is_contiguous() and tuple(sf_t.shape) == (H, N // 32),
                 'cast_fp8_mx_transposed outputs must be contiguous float8_e4m3fn [H, N] and uint8 [H, N / 32] on the '
                 'GPU')
        _require((q is None) == (sf is None), 'cast_fp8_mx_transposed takes the row-wise pair as both q and sf')
        if q is not None:
            _require(q.is_cuda and q.dtype == torch.float8_e4m3fn and q.is_contiguous() and tuple(q.shape) == (N, H)
                     and sf.is_cuda and sf.dtype in MX_SF_DTYPES and sf.is_contiguous() and
                     tuple(sf.shape) == (N, H // 32),
                     'cast_fp8_mx_transposed row-wise outputs must be contiguous float8_e4m3fn [N, H] and uint8 '
                     '[N, H / 32] on the GPU')
        self._entry('cast_fp8_mx_transposed')(ptr(x), x.stride(0) * 2 if N else H * 2, ptr(q_t), ptr(sf_t), ptr(q),
                                              ptr(sf), N, H, _stream_handle(stream))


class TransposedFp4Fp6Kernels:
    """The transposed MXFP4 and MXFP6 casts of HipKernels (csrc/fp46_cast_t.hip; the contract: include/deepep_amd.h,
    deepep_cast_fp4_mx_transposed): cast_fp8_mx_transposed over e2m1 and e2m3 codes, stored [H, N / 2] and
    [H, 3 * N / 4].  Only the package's cast_to_mxfp4_transposed / cast_to_mxfp6_transposed call them."""

    def _cast_mx_transposed(self, name, num, den, x, q_t, sf_t, q, sf, stream):
        # a row of 32 elements is 32 * num / den bytes of codes (FP4: 1 / 2, FP6: 3 / 4)
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 f'{name} input must be 2-D bf16 on the GPU with unit column stride')
        N, H = x.shape
        _require(H % 128 == 0 and H > 0 and N % 128 == 0,
                 f'{name} needs a hidden size and a row count that are multiples of 128')
        _require(N == 0 or (x.stride(0) % 8 == 0 and x.stride(0) >= H and x.data_ptr() % 16 == 0),
                 f'{name} rows must start 16-byte aligned')
        _require(q_t.is_cuda and q_t.dtype == torch.uint8 and q_t.is_contiguous() and
                 tuple(q_t.shape) == (H, N * num // den) and sf_t.is_cuda and sf_t.dtype in MX_SF_DTYPES and
                 sf_t.is_contiguous() and tuple(sf_t.shape) == (H, N // 32),
                 f'{name} outputs must be contiguous uint8 [H, {num} * N / {den}] and uint8 [H, N / 32] on the GPU')
        _require((q is None) == (sf is None), f'{name} takes the row-wise pair as both q and sf')
        if q is not None:
            _require(q.is_cuda and q.dtype == torch.uint8 and q.is_contiguous() and
                     tuple(q.shape) == (N, H * num // den) and sf.is_cuda and sf.dtype in MX_SF_DTYPES and
                     sf.is_contiguous() and tuple(sf.shape) == (N, H // 32),
                     f'{name} row-wise outputs must be contiguous uint8 [N, {num} * H / {den}] and uint8 [N, H / 32] '
                     'on the GPU')
        self._entry(name)(ptr(x), x.stride(0) * 2 if N else H * 2, ptr(q_t), ptr(sf_t), ptr(q), ptr(sf), N, H,
                          _stream_handle(stream))

    def cast_fp4_mx_transposed(self, x, q_t, sf_t, q=None, sf=None, stream=None):
        """x bf16 [N, H] (rows may be strided: unit column stride, row stride a multiple of 8 elements), N % 128 == 0,
        H % 128 == 0 -> q_t uint8 [H, N / 2] and sf_t uint8 / float8_e8m0fnu [H, N / 32], both contiguous: bit for
        bit cast_fp4 of x.t().contiguous().  q and sf (both or neither): the same launch also writes cast_fp4 of x
        itself, q uint8 [N, H / 2] and sf [N, H / 32], from the same read."""
        self._cast_mx_transposed('cast_fp4_mx_transposed', 1, 2, x, q_t, sf_t, q, sf, stream)

    def cast_fp6_mx_transposed(self, x, q_t, sf_t, q=None, sf=None, stream=None):
        """cast_fp4_mx_transposed over e2m3 codes: q_t uint8 [H, 3 * N / 4], bit for bit cast_fp6 of
        x.t().contiguous(); the row-wise q is uint8 [N, 3 * H / 4]."""
        self._cast_mx_transposed('cast_fp6_mx_transposed', 3, 4, x, q_t, sf_t, q, sf, stream)


class RequantTransposedKernels:
    """The requantisation along the tokens of HipKernels (csrc/requant_t.hip; the contract: include/deepep_amd.h,
    deepep_requant_fp8_mx_transposed): a row-wise quantised pair -> the pair of the transposed cast of its cast back,
    bit for bit, in one read and without the bf16 rows.  Only the package's requant_mxfp8_transposed /
    requant_mxfp4_transposed / requant_mxfp6_transposed call them."""

    def _requant(self, name, row_dtypes, num, den, q_t_dtype, form, q, sf, q_t, sf_t, stream):
        # a row of 32 elements is 32 * num / den bytes of codes (FP8: 1, FP4: 1 / 2, FP6: 3 / 4); form: the FP8 entry's
        # sf_form, None for the entries that take exponent bytes per 32 columns only
        _require(q.is_cuda and q.dim() == 2 and q.dtype in row_dtypes and (q.numel() == 0 or q.stride(1) == 1),
                 f'{name} rows must be 2-D codes on the GPU with unit column stride')
        N, H = q.shape[0], q.shape[1] * den // num
        _require(H % 128 == 0 and H > 0 and N % 128 == 0,
                 f'{name} needs a hidden size and a row count that are multiples of 128')
        _require(N == 0 or (q.stride(0) % 16 == 0 and q.stride(0) >= q.shape[1] and q.data_ptr() % 16 == 0),
                 f'{name} rows must start 16-byte aligned')
        fmt = sf_format_of(sf.dtype)
        _require(fmt is not None and (form is not None or fmt is SF_MXFP8) and sf.is_cuda and
                 sf.device == q.device and H % fmt.multiple == 0 and tuple(sf.shape) == (N, fmt.elems(H)),
                 f'{name} takes the scale factors of its rows on their GPU')
        _require(sf.data_ptr() % sf.element_size() == 0, f'{name} scale factors must be aligned to their elements')
        _require(q_t.is_cuda and q_t.dtype == q_t_dtype and q_t.is_contiguous() and
                 tuple(q_t.shape) == (H, N * num // den) and sf_t.is_cuda and sf_t.dtype in MX_SF_DTYPES and
                 sf_t.is_contiguous() and tuple(sf_t.shape) == (H, N // 32),
                 f'{name} outputs must be contiguous {q_t_dtype} [H, {num} * N / {den}] and uint8 [H, N / 32] on the '
                 'GPU')
        forms = {SF_FP32: _lib.SF_FORM_FP32, SF_UE8M0: _lib.SF_FORM_UE8M0_PACKED, SF_MXFP8: _lib.SF_FORM_MX}
        self._entry(name)(ptr(q), q.stride(0) if N else q.shape[1], ptr(sf), sf.stride(0), sf.stride(1),
                          *((forms[fmt],) if form is not None else ()), ptr(q_t), ptr(sf_t), N, H,
                          _stream_handle(stream))

    def requant_fp8_mx_transposed(self, q, sf, q_t, sf_t, stream=None):
        """q float8_e4m3fn [N, H] (rows may be strided, a multiple of 16 bytes apart) with sf in any form cast_back_fp8
        takes (float32 [N, H / 128], int32 [N, H / 512], uint8 / float8_e8m0fnu [N, H / 32]; any strides), N % 128 == 0,
        H % 128 == 0 -> q_t float8_e4m3fn [H, N] and sf_t uint8 / float8_e8m0fnu [H, N / 32], both contiguous: bit for
        bit cast_fp8_mx_transposed of cast_back_fp8(q, sf)."""
        self._requant('requant_fp8_mx_transposed', (torch.float8_e4m3fn,), 1, 1, torch.float8_e4m3fn, True, q, sf,
                      q_t, sf_t, stream)

    def requant_fp4_mx_transposed(self, q, sf, q_t, sf_t, stream=None):
        """q uint8 / float4_e2m1fn_x2 [N, H / 2] with sf uint8 / float8_e8m0fnu [N, H / 32] of any strides -> q_t uint8
        [H, N / 2] and sf_t [H, N / 32]: bit for bit cast_fp4_mx_transposed of cast_back_fp4(q, sf)."""
        self._requant('requant_fp4_mx_transposed', FP4_ROW_DTYPES, 1, 2, torch.uint8, None, q, sf, q_t, sf_t, stream)

    def requant_fp6_mx_transposed(self, q, sf, q_t, sf_t, stream=None):
        """q uint8 [N, 3 * H / 4] with sf uint8 / float8_e8m0fnu [N, H / 32] of any strides -> q_t uint8 [H, 3 * N / 4]
        and sf_t [H, N / 32]: bit for bit cast_fp6_mx_transposed of cast_back_fp6(q, sf)."""
        self._requant('requant_fp6_mx_transposed', (torch.uint8,), 3, 4, torch.uint8, None, q, sf, q_t, sf_t, stream)


class HipKernels(LogfmtKernels, Fp4Kernels, Fp6Kernels, TransposedCastKernels, TransposedFp4Fp6Kernels,
                 RequantTransposedKernels):
    """The HIP implementation of the combine primitives (gfx950)."""

    name = 'hip'

    def __init__(self):
        self.lib = _lib.load()

    def _entry(self, name: str):                    # looked up before its arguments are formed
        fn = getattr(self.lib, 'deepep_' + name)
        return lambda *args: _lib.check(fn(*args), name)

    def combine_reduce(self, mode: int, src: torch.Tensor, out: torch.Tensor, num_units: int,
                       table: Optional[torch.Tensor] = None,
                       row_weights: Optional[torch.Tensor] = None,
                       bias0: Optional[torch.Tensor] = None, bias1: Optional[torch.Tensor] = None,
                       wtable: Optional[torch.Tensor] = None, wsrc: Optional[torch.Tensor] = None,
                       out_weights: Optional[torch.Tensor] = None,
                       units_per_block: int = 0, error_flag: Optional[torch.Tensor] = None,
                       weights_pad: int = 0, stream=None, src_sf: Optional[torch.Tensor] = None,
                       src_logfmt_meta: Optional[torch.Tensor] = None) -> None:
        """weights_pad: floats written per weight row (zeros past the weights); 32 fills a packed
        row's 128-byte tail line, so no partial line reaches the memory side.
        src_sf: the scale factors of an FP8 source -- src is then float8_e4m3fn [M, H] (rows may be strided) and
        src_sf float32 [M, H / 128] or int32 [M, H / 512] (packed UE8M0) of any strides, as cast_back_fp8 takes
        them; the result is bit for bit that of the same call over cast_back_fp8(src, src_sf).
        src_logfmt_meta (MODE_EPILOGUE only): the meta dwords of a LogFMT source -- src is then the planes uint8
        [M, H * 5 / 4] and src_logfmt_meta int32 [M, H / 128], rows of both may be strided (cast_logfmt's outputs, or
        views of logfmt_pack_rows' wire rows); the result is bit for bit that of the same call over
        cast_back_logfmt(src, src_logfmt_meta)."""
        _require(src.is_cuda and out.is_cuda, 'combine tensors must be on the GPU')
        if src_logfmt_meta is not None:
            _require(src_sf is None and mode == MODE_EPILOGUE and units_per_block == 0,
                     'a LogFMT source is reduced by the epilogue only, and is not an FP8 source')
            return self._combine_reduce_logfmt(src, src_logfmt_meta, out, num_units, table, row_weights, bias0, bias1,
                                               wtable, wsrc, out_weights, error_flag, weights_pad, stream)
        fp8 = _fp8_source(src, src_sf, 'combine_reduce') if src_sf is not None else None
        _require((fp8 is not None or src.dtype == torch.bfloat16) and out.dtype == torch.bfloat16,
                 'combine rows must be bfloat16')
        _require(src.dim() == 2 and out.dim() == 2 and (src.numel() == 0 or src.stride(1) == 1) and
                 (out.numel() == 0 or out.stride(1) == 1), 'combine rows must be 2-D with unit column stride')
        hidden = out.shape[1]
        _require(src.shape[1] == hidden or src.shape[0] == 0, 'source and output hidden sizes differ')
        _require(out.shape[0] >= num_units, 'output has fewer rows than units')
        for b in (bias0, bias1):
            if b is not None:
                _require(b.is_cuda and b.dtype == torch.bfloat16 and b.is_contiguous() and
                         tuple(b.shape) == (num_units, hidden), 'bias must be contiguous bf16 [num_tokens, hidden]')
        t, t_stride, t_width = _table_view(table)
        if t is not None:
            _require(t.shape[0] >= num_units, 'slot table has fewer rows than units')
        w, w_stride, _ = _table_view(wtable)
        num_weights = 0
        ow_stride = 0
        if out_weights is not None:
            _require(out_weights.dtype == torch.float32 and out_weights.dim() == 2 and out_weights.stride(1) == 1,
                     'weights must be float32 [units, k] with unit column stride')
            _require(out_weights.shape[0] >= num_units, 'weight output has fewer rows than units')
            num_weights = out_weights.shape[1]
            ow_stride = out_weights.stride(0)
            _require(wsrc is not None and wsrc.dtype == torch.float32 and wsrc.dim() == 1 and
                     (wsrc.stride(0) == 1 or wsrc.numel() <= 1), 'weight source must be a 1-D float32 view')
        weighted = row_weights is not None
        if weighted:
            _require(row_weights.dtype == torch.float32 and row_weights.is_contiguous(),
                     'row weights must be contiguous float32')
        entry, sf_args = ((self.lib.deepep_combine_reduce, ()) if fp8 is None else
                          (self.lib.deepep_combine_reduce_fp8, fp8))
        rc = entry(
            mode, int(weighted),
            ptr(src), src.shape[0], src.stride(0) if src.shape[0] > 0 else hidden, *sf_args,
            ptr(t), t_stride, t_width,
            ptr(row_weights),
            ptr(bias0), ptr(bias1),
            ptr(out), out.stride(0) if out.shape[0] > 0 else hidden,
            num_units, hidden,
            ptr(w), w_stride,
            ptr(wsrc), ptr(out_weights), num_weights, ow_stride, weights_pad,
            units_per_block, ptr(error_flag),
            _stream_handle(stream))
        _lib.check(rc, 'combine_reduce' if fp8 is None else 'combine_reduce_fp8')

    def _combine_reduce_logfmt(self, src, meta, out, num_units, table, row_weights, bias0, bias1, wtable, wsrc,
                               out_weights, error_flag, weights_pad, stream) -> None:
        """combine_reduce(MODE_EPILOGUE) over a LogFMT source (its checks, then deepep_combine_reduce_logfmt)."""
        _require(out.dtype == torch.bfloat16 and out.dim() == 2 and (out.numel() == 0 or out.stride(1) == 1),
                 'combine rows must be 2-D bfloat16 with unit column stride')
        hidden = out.shape[1]
        M = _logfmt_pair(src, meta, hidden, 'combine_reduce')
        _require(out.shape[0] >= num_units, 'output has fewer rows than units')
        for b in (bias0, bias1):
            if b is not None:
                _require(b.is_cuda and b.dtype == torch.bfloat16 and b.is_contiguous() and
                         tuple(b.shape) == (num_units, hidden), 'bias must be contiguous bf16 [num_tokens, hidden]')
        t, t_stride, t_width = _table_view(table)
        if t is not None:
            _require(t.shape[0] >= num_units, 'slot table has fewer rows than units')
        w, w_stride, _ = _table_view(wtable)
        num_weights = 0
        ow_stride = 0
        if out_weights is not None:
            _require(out_weights.dtype == torch.float32 and out_weights.dim() == 2 and out_weights.stride(1) == 1,
                     'weights must be float32 [units, k] with unit column stride')
            _require(out_weights.shape[0] >= num_units, 'weight output has fewer rows than units')
            num_weights = out_weights.shape[1]
            ow_stride = out_weights.stride(0)
            _require(wsrc is not None and wsrc.dtype == torch.float32 and wsrc.dim() == 1 and
                     (wsrc.stride(0) == 1 or wsrc.numel() <= 1), 'weight source must be a 1-D float32 view')
        weighted = row_weights is not None
        if weighted:
            _require(row_weights.dtype == torch.float32 and row_weights.is_contiguous(),
                     'row weights must be contiguous float32')
        self._entry('combine_reduce_logfmt')(
            int(weighted), ptr(src), M, src.stride(0) if M else hidden * 5 // 4,
            ptr(meta), meta.stride(0) if M else hidden // 128,
            ptr(t), t_stride, t_width, ptr(row_weights), ptr(bias0), ptr(bias1),
            ptr(out), out.stride(0) if out.shape[0] > 0 else hidden, num_units, hidden,
            ptr(w), w_stride, ptr(wsrc), ptr(out_weights), num_weights, ow_stride, weights_pad,
            ptr(error_flag), _stream_handle(stream))

    def combine_reduce_scatter(self, src: torch.Tensor, num_units: int, out_rows: torch.Tensor,
                               table: Optional[torch.Tensor] = None, row_weights: Optional[torch.Tensor] = None,
                               wtable: Optional[torch.Tensor] = None, wsrc: Optional[torch.Tensor] = None,
                               num_weights: int = 0, weights_offset: int = 0, weights_pad: int = 0,
                               error_flag: Optional[torch.Tensor] = None, *, windows, stream=None,
                               src_sf: Optional[torch.Tensor] = None, dst_logfmt: bool = False) -> None:
        """Phase A storing unit u's row at byte address out_rows[u] (a peer window over xGMI).
        windows = (bases, bytes): int64 [n] device tensor of window data addresses and the extent of each;
        a row not wholly inside one of them is skipped and flagged (error_flag: an error record of
        _lib.ERROR_RECORD_INTS ints).  src_sf: the scale factors of an FP8 source, as combine_reduce takes them.
        dst_logfmt (H % 128 == 0, a bf16 source): the row stored is the LogFMT wire row [low | high | meta | pad |
        weights at weights_offset] (handle.logfmt_row_layout) -- bit for bit cast_logfmt of the bf16 row the call
        without the flag stores, with the same weights."""
        if dst_logfmt:
            _require(src_sf is None, 'a LogFMT destination takes a bf16 source: reduce an FP8 source into bf16 rows '
                                     'first (combine_reduce(MODE_LOCAL, ..., src_sf=...))')
            return self._combine_reduce_scatter_logfmt(src, num_units, out_rows, table, row_weights, wtable, wsrc,
                                                       num_weights, weights_offset, weights_pad, error_flag, windows,
                                                       stream)
        fp8 = _fp8_source(src, src_sf, 'combine_reduce_scatter') if src_sf is not None else None
        _require(fp8 is not None or (src.is_cuda and src.dtype == torch.bfloat16 and src.dim() == 2 and
                                     (src.numel() == 0 or src.stride(1) == 1)),
                 'combine rows must be 2-D bf16 on the GPU with unit column stride')
        _require(out_rows.is_cuda and out_rows.dtype == torch.int64 and out_rows.is_contiguous() and
                 out_rows.shape[0] >= num_units, 'out_rows must be int64 [num_units] on the GPU')
        win_bases, win_bytes = windows
        _require(win_bases.is_cuda and win_bases.dtype == torch.int64 and win_bases.is_contiguous() and
                 win_bases.dim() == 1, 'window bases must be int64 [num_windows] on the GPU')
        _require(error_flag is None or error_flag.numel() >= 1, 'error flag')
        t, t_stride, t_width = _table_view(table)
        w, w_stride, _ = _table_view(wtable)
        if num_weights:
            _require(wsrc is not None and wsrc.dtype == torch.float32 and wsrc.dim() == 1, 'weight source')
        if row_weights is not None:
            _require(row_weights.dtype == torch.float32 and row_weights.is_contiguous(), 'row weights')
        hidden = src.shape[1]
        entry, sf_args = ((self.lib.deepep_combine_reduce_scatter, ()) if fp8 is None else
                          (self.lib.deepep_combine_reduce_scatter_fp8, fp8))
        rc = entry(
            int(row_weights is not None), ptr(src), src.shape[0], src.stride(0) if src.shape[0] > 0 else hidden,
            *sf_args, ptr(t), t_stride, t_width, ptr(row_weights), ptr(out_rows), num_units, hidden,
            ptr(w), w_stride, ptr(wsrc), num_weights, weights_offset, weights_pad,
            ptr(win_bases), win_bases.shape[0], int(win_bytes), ptr(error_flag), _stream_handle(stream))
        _lib.check(rc, 'combine_reduce_scatter' if fp8 is None else 'combine_reduce_scatter_fp8')

    def _combine_reduce_scatter_logfmt(self, src, num_units, out_rows, table, row_weights, wtable, wsrc, num_weights,
                                       weights_offset, weights_pad, error_flag, windows, stream) -> None:
        """combine_reduce_scatter storing LogFMT wire rows (its checks, then deepep_combine_reduce_scatter_logfmt)."""
        _require(isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.bfloat16 and src.dim() == 2 and
                 (src.numel() == 0 or src.stride(1) == 1),
                 'combine rows must be 2-D bf16 on the GPU with unit column stride')
        hidden = src.shape[1]
        _require(hidden % 128 == 0 and hidden > 0,
                 'combine_reduce_scatter needs a hidden size that is a multiple of 128 for LogFMT rows')
        _require(out_rows.is_cuda and out_rows.dtype == torch.int64 and out_rows.is_contiguous() and
                 out_rows.shape[0] >= num_units, 'out_rows must be int64 [num_units] on the GPU')
        win_bases, win_bytes = windows
        _require(win_bases.is_cuda and win_bases.dtype == torch.int64 and win_bases.is_contiguous() and
                 win_bases.dim() == 1, 'window bases must be int64 [num_windows] on the GPU')
        _require(error_flag is None or error_flag.numel() >= 1, 'error flag')
        t, t_stride, t_width = _table_view(table)
        if t is not None:
            _require(t.shape[0] >= num_units, 'slot table has fewer rows than units')
        else:
            _require(src.shape[0] >= num_units, 'without a slot table unit u reads row u: fewer rows than units')
        w, w_stride, _ = _table_view(wtable)
        if num_weights:
            _require(wsrc is not None and wsrc.dtype == torch.float32 and wsrc.dim() == 1, 'weight source')
            _require(weights_offset % 16 == 0 and weights_offset >= hidden * 5 // 4 + hidden // 32,
                     'the weights of a LogFMT wire row lie 16-byte aligned behind its coded bytes')
        if row_weights is not None:
            _require(row_weights.dtype == torch.float32 and row_weights.is_contiguous(), 'row weights')
        self._entry('combine_reduce_scatter_logfmt')(
            int(row_weights is not None), ptr(src), src.shape[0], src.stride(0) if src.shape[0] > 0 else hidden,
            ptr(t), t_stride, t_width, ptr(row_weights), ptr(out_rows), num_units, hidden,
            ptr(w), w_stride, ptr(wsrc), num_weights, weights_offset, weights_pad,
            ptr(win_bases), win_bases.shape[0], int(win_bytes), ptr(error_flag), _stream_handle(stream))

    def build_local_plan(self, src_metadata: torch.Tensor, num_recv_tokens: int, num_topk: int,
                         num_max_tokens_per_rank: int, expanded: bool, plan: torch.Tensor,
                         num_tokens: int, topk_idx: Optional[torch.Tensor] = None,
                         wtable: Optional[torch.Tensor] = None, stream=None) -> None:
        _require(src_metadata.is_cuda and src_metadata.dtype == torch.int32 and src_metadata.is_contiguous(),
                 'recv_src_metadata must be contiguous int32 on the GPU')
        _require(plan.is_contiguous() and plan.dtype == torch.int32, 'plan must be contiguous int32')
        if wtable is not None:
            # the kernel reads topk_idx only for the weight table, as 8-byte entries
            _require(topk_idx is not None and topk_idx.is_cuda and topk_idx.dtype == torch.int64 and
                     topk_idx.is_contiguous(), 'topk_idx int64')
            _require(wtable.dtype == torch.int32 and wtable.is_contiguous(), 'wtable int32')
        rc = self.lib.deepep_build_local_plan(
            ptr(src_metadata), num_recv_tokens, num_topk, num_max_tokens_per_rank, int(expanded),
            ptr(plan), plan.shape[1], num_tokens, ptr(topk_idx), ptr(wtable), _stream_handle(stream))
        _lib.check(rc, 'build_local_plan')

    # ------------------------------------------------------------------ dispatch (handle producer)
    def dispatch_route(self, topk_idx, num_experts, num_ranks, dst_slot, send_counts, stream=None):
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        block_counts = torch.empty((max(1, (T + 255) // 256) * num_ranks,), dtype=torch.int32, device=topk_idx.device)
        rc = self.lib.deepep_dispatch_route(ptr(topk_idx), T, K, num_experts, num_ranks, ptr(dst_slot),
                                            ptr(send_counts), ptr(block_counts), _stream_handle(stream))
        _lib.check(rc, 'dispatch_route')

    def dispatch_notify(self, topk_idx, num_experts, num_ranks, num_blocks, dst_slot, notify, send_offsets,
                        stream=None):
        """The send side in two launches: dst_slot [T, R], notify int32 [R, 1 + E/R + 2 * num_blocks] (per
        destination: tokens | tokens per expert | per-block tokens | per-block pairs), send_offsets [R]."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        W = 1 + num_experts // num_ranks + 2 * num_blocks
        _require(notify.dtype == torch.int32 and notify.is_contiguous() and tuple(notify.shape) == (num_ranks, W),
                 'notify must be contiguous int32 [num_ranks, 1 + experts_per_rank + 2 * num_blocks]')
        _require(dst_slot.dtype == torch.int32 and dst_slot.is_contiguous() and dst_slot.numel() == T * num_ranks,
                 'dst_slot must be contiguous int32 [num_tokens, num_ranks]')
        _require(send_offsets.dtype == torch.int32 and send_offsets.is_contiguous() and
                 send_offsets.numel() == num_ranks, 'send_offsets must be contiguous int32 [num_ranks]')
        ws_bytes = int(self.lib.deepep_dispatch_notify_workspace(T, num_experts, num_ranks))
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=topk_idx.device)
        rc = self.lib.deepep_dispatch_notify(ptr(topk_idx), T, K, num_experts, num_ranks, num_blocks, ptr(dst_slot),
                                             ptr(notify), ptr(send_offsets), ptr(ws), ws.numel(),
                                             _stream_handle(stream))
        _lib.check(rc, 'dispatch_notify')

    def dispatch_expert_counts(self, topk_idx, num_experts, counts, stream=None):
        """counts[e] = (t, k) entries routed to expert e (int32 [num_experts])."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        _require(counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == num_experts,
                 'expert counts must be contiguous int32 [num_experts]')
        T, K = topk_idx.shape
        rc = self.lib.deepep_dispatch_expert_counts(ptr(topk_idx), T, K, num_experts, ptr(counts),
                                                    _stream_handle(stream))
        _lib.check(rc, 'dispatch_expert_counts')

    # ------------------------------------------------------------------ EP > 1 combine plan (plan.hip)
    def route_block_counts(self, topk_idx, num_experts, num_ranks, num_blocks, tok, pairs, stream=None):
        """tok / pairs: int32 [num_ranks, num_blocks] (64-token blocks of this rank's tokens)."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        for t in (tok, pairs):
            _require(t.dtype == torch.int32 and t.is_contiguous() and t.numel() == num_ranks * num_blocks,
                     'block counts must be contiguous int32 [num_ranks, num_blocks]')
        T, K = topk_idx.shape
        rc = self.lib.deepep_route_block_counts(ptr(topk_idx), T, K, num_experts, num_ranks, num_blocks, ptr(tok),
                                                ptr(pairs), _stream_handle(stream))
        _lib.check(rc, 'route_block_counts')

    def plan_expert(self, meta, num_topk, num_ranks, rank, num_max_tokens, recv_tok, recv_pairs, num_blocks,
                    blocks_per_chunk, flags, table_a, wtable_a, window_bases, window_row_bytes, out_rows,
                    window_bytes: int = 0, error_flag=None, padded_stride: int = 0, stream=None):
        """window_bytes: the data extent of every window (out_rows rows are bounded by it); error_flag:
        an error record (_lib.ERROR_RECORD_INTS ints) or None.  table_a / wtable_a / out_rows should be
        pre-filled with -1 / -1 / 0: a unit the kernel rejects is left as it was."""
        _require(meta.is_cuda and meta.dtype == torch.int32 and meta.is_contiguous(), 'recv_src_metadata int32')
        _require(table_a.dtype == torch.int32 and table_a.is_contiguous(), 'table_a int32')
        _require(wtable_a is None or (wtable_a.dtype == torch.int32 and wtable_a.is_contiguous()), 'wtable_a int32')
        _require(out_rows is None or (out_rows.dtype == torch.int64 and out_rows.is_contiguous() and
                                      window_bases is not None and window_bytes > 0),
                 'out_rows int64 with window bases and extent')
        rc = self.lib.deepep_plan_expert(ptr(meta), meta.shape[0], num_topk, num_ranks, rank, num_max_tokens,
                                         ptr(recv_tok), ptr(recv_pairs), num_blocks, blocks_per_chunk, flags,
                                         ptr(table_a), ptr(wtable_a), ptr(window_bases), window_row_bytes,
                                         int(window_bytes), ptr(out_rows), ptr(error_flag), int(padded_stride),
                                         _stream_handle(stream))
        _lib.check(rc, 'plan_expert')

    def plan_source(self, topk_idx, num_experts, num_ranks, rank, num_max_tokens, dst_slot, send_tok, send_pairs,
                    num_blocks, blocks_per_chunk, flags, row_floats, weights_offset, table_b, wtable,
                    padded_stride: int = 0, stream=None):
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        _require(table_b.dtype == torch.int32 and table_b.is_contiguous(), 'table_b int32')
        _require(wtable is None or (wtable.dtype == torch.int32 and wtable.is_contiguous()), 'wtable int32')
        T, K = topk_idx.shape
        rc = self.lib.deepep_plan_source(ptr(topk_idx), T, K, num_experts, num_ranks, rank, num_max_tokens, ptr(dst_slot),
                                         ptr(send_tok), ptr(send_pairs), num_blocks, blocks_per_chunk, flags,
                                         row_floats, weights_offset, ptr(table_b), table_b.shape[1], ptr(wtable),
                                         int(padded_stride), _stream_handle(stream))
        _lib.check(rc, 'plan_source')

    def dispatch_pack(self, x_bytes, sf_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets,
                      packed, layout: RowLayout, dest_bases=None, dest_rows: Optional[int] = None, error_flag=None,
                      stream=None):
        """x_bytes / sf_bytes: [T, bytes] uint8 views (rows may be strided).  dest_bases: optional
        int64 [R] device tensor of per-destination buffer addresses (peer windows) instead of `packed`;
        dest_rows: the rows each destination holds (default: the rows of `packed`); a row past it is
        not stored (flagged in error_flag, an error record of _lib.ERROR_RECORD_INTS ints)."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        if dest_bases is not None:
            _require(dest_bases.is_cuda and dest_bases.dtype == torch.int64 and dest_bases.is_contiguous() and
                     dest_bases.numel() == dst_slot.shape[1], 'dest_bases must be int64 [num_ranks] on the GPU')
            _require(dest_rows is not None, 'dest_rows (rows per destination window) is required with dest_bases')
        else:
            dest_rows = packed.shape[0] if dest_rows is None else min(dest_rows, packed.shape[0])
        rc = self.lib.deepep_dispatch_pack(
            ptr(x_bytes), x_bytes.stride(0) if T else layout.x_bytes, layout.x_bytes,
            ptr(sf_bytes), sf_bytes.stride(0) if sf_bytes is not None and T else 0, layout.sf_bytes,
            ptr(topk_idx), ptr(topk_weights), T, K, src_base, ptr(dst_slot), ptr(send_offsets),
            dst_slot.shape[1], ptr(packed), ptr(dest_bases), layout.row_bytes, int(dest_rows), layout.sf_off,
            layout.idx_off,
            layout.w_off, layout.src_off, ptr(error_flag), _stream_handle(stream))
        _lib.check(rc, 'dispatch_pack')

    def cast_fp8(self, x, q, sf, round_scale: bool = False, stream=None, ue8m0: bool = False, mx: bool = False):
        """Per-token, per-128-column FP8 cast (per_token_cast_to_fp8, bit for bit): x bf16 [T, H] (rows may
        be strided) -> q float8_e4m3fn [T, H], sf float32 [T, H / 128], both contiguous.  round_scale: power-
        of-two scale factors.  ue8m0 (with round_scale, H % 512 == 0): sf int32 [T, H / 512], the factors'
        exponent bytes, four to an element.  mx (with round_scale, not with ue8m0; H % 128 == 0): MXFP8, the
        round_scale rule per 32 columns, sf uint8 [T, H / 32], one exponent byte per group."""
        _require(x.is_cuda and x.dim() == 2 and x.dtype == torch.bfloat16 and (x.numel() == 0 or x.stride(1) == 1),
                 'cast_fp8 input must be 2-D bf16 on the GPU with unit column stride')
        T, H = x.shape
        fmt = sf_format(ue8m0, mx, 'cast_fp8')
        fmt.require('cast_fp8', H, round_scale)
        _require(q.dtype == torch.float8_e4m3fn and q.is_contiguous() and tuple(q.shape) == (T, H) and
                 sf.dtype == fmt.dtype and sf.is_contiguous() and tuple(sf.shape) == (T, fmt.elems(H)),
                 f'cast_fp8 outputs must be contiguous float8_e4m3fn [rows, H] and {fmt}')
        self._entry('cast_fp8' + fmt.suffix)(ptr(x), x.stride(0) * 2 if T else H * 2, T, H, *fmt.scale_arg(round_scale),
                                             ptr(q), ptr(sf), _stream_handle(stream))

    def cast_back_fp8(self, q, sf, out, stream=None):
        """The inverse of cast_fp8 (per_token_cast_back, bit for bit): q float8_e4m3fn [M, H] (rows may be
        strided), sf float32 [M, H / 128] of any strides (the column-major scale factors are read in place)
        -> out bf16 [M, H], contiguous.  Or sf int32 [M, H / 512] of any strides, H % 512 == 0: the packed UE8M0
        exponent bytes (cast_fp8(ue8m0=True)), out = bf16(fp32(q) * float_from_bits(byte << 23)).  Or sf uint8 /
        float8_e8m0fnu [M, H / 32] of any strides: MXFP8's exponent byte per 32 columns (cast_fp8(mx=True)), the
        same arithmetic."""
        _require(q.is_cuda and q.dim() == 2 and q.dtype == torch.float8_e4m3fn and
                 (q.numel() == 0 or q.stride(1) == 1),
                 'cast_back_fp8 input must be 2-D float8_e4m3fn on the GPU with unit column stride')
        M, H = q.shape
        _require(H % 128 == 0 and H > 0, 'cast_back_fp8 needs a hidden size that is a multiple of 128')
        fmt = sf_format_of(sf.dtype)
        _require(fmt is not None, 'cast_back_fp8 takes float32, int32 (packed UE8M0) or uint8 / float8_e8m0fnu (MXFP8) '
                                  'scale factors')
        _require(sf.is_cuda and H % fmt.multiple == 0 and tuple(sf.shape) == (M, fmt.elems(H)),
                 f'cast_back_fp8 takes {fmt} on the GPU, H % {fmt.multiple} == 0')
        _require(sf.data_ptr() % 4 == 0 and (sf.stride(1) != 1 or sf.stride(0) * sf.element_size() % 4 == 0),
                 'cast_back_fp8 scale factors must start 4-byte aligned, as must rows of unit column stride')
        _require(out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (M, H),
                 'cast_back_fp8 output must be contiguous bf16 [M, H] on the GPU')
        self._entry('cast_back_fp8' + fmt.suffix)(ptr(q), q.stride(0) if M else H, ptr(sf), sf.stride(0), sf.stride(1),
                                                  M, H, ptr(out), _stream_handle(stream))

    def dispatch_pack_cast(self, x_bytes, topk_idx, topk_weights, src_base, dst_slot, send_offsets, packed,
                           layout: RowLayout, round_scale: bool = False, dest_bases=None,
                           dest_rows: Optional[int] = None, error_flag=None, stream=None, ue8m0: bool = False,
                           mx: bool = False):
        """dispatch_pack with cast_fp8 fused in: x_bytes is the uint8 view [T, 2 * H] of the tokens' bf16 rows,
        layout the FP8 row layout RowLayout.make(H, fmt.row_bytes(H), K) of the format fmt that ue8m0 / mx name
        (sf_format; cast_fp8's conditions); the packed rows get the e4m3fn bytes and the scale factors.  The other
        arguments as dispatch_pack."""
        _require(topk_idx.is_cuda and topk_idx.dtype == torch.int64 and topk_idx.is_contiguous(), 'topk_idx int64')
        T, K = topk_idx.shape
        H = layout.x_bytes
        fmt = sf_format(ue8m0, mx, 'dispatch_pack_cast')
        fmt.require('dispatch_pack_cast', H, round_scale)
        _require(layout.sf_bytes == fmt.row_bytes(H) and x_bytes.shape[1] == 2 * H,
                 f'dispatch_pack_cast needs bf16 rows of H columns and, for {fmt}, the row layout '
                 f'RowLayout.make(H, {fmt.row_bytes(H)}, K)')
        if dest_bases is not None:
            _require(dest_bases.is_cuda and dest_bases.dtype == torch.int64 and dest_bases.is_contiguous() and
                     dest_bases.numel() == dst_slot.shape[1], 'dest_bases must be int64 [num_ranks] on the GPU')
            _require(dest_rows is not None, 'dest_rows (rows per destination window) is required with dest_bases')
        else:
            dest_rows = packed.shape[0] if dest_rows is None else min(dest_rows, packed.shape[0])
        self._entry('dispatch_pack_cast' + fmt.suffix)(
            ptr(x_bytes), x_bytes.stride(0) if T else 2 * H, H, *fmt.scale_arg(round_scale),
            ptr(topk_idx), ptr(topk_weights), T, K, src_base, ptr(dst_slot), ptr(send_offsets),
            dst_slot.shape[1], ptr(packed), ptr(dest_bases), layout.row_bytes, int(dest_rows), layout.sf_off,
            layout.idx_off, layout.w_off, layout.src_off, ptr(error_flag), _stream_handle(stream))

    def dispatch_count(self, packed, layout: RowLayout, num_recv, rank, num_local_experts, rank_psum, meta,
                       recv_topk_idx, block_counts, pad_rows: int = 0, row_map=None, rank_counts=None,
                       psum_out=None, own_first: bool = False, stream=None):
        """rank_psum: inclusive prefix of rows per source rank (int32 [R]); or, with rank_psum None,
        rank_counts: rows per source rank (an int32 [R] view of any stride, e.g. the notify records'
        first column), whose prefix the kernel forms and writes to psum_out (int32 [R]).
        pad_rows > 0: `packed` is a worst-case-sized receive buffer, source s's rows at s * pad_rows;
        row_map (int32 [num_recv]) receives each received row's packed row (for slots / copy).
        own_first: `packed` = [rows from this rank | rows from the others, rank order] (the local bypass);
        row_map is written the same way."""
        src = rank_psum if rank_psum is not None else rank_counts
        _require(src is not None and src.dim() == 1 and src.dtype == torch.int32 and src.stride(0) >= 1,
                 'dispatch_count needs rank_psum or rank_counts (int32 [num_ranks])')
        R = src.shape[0]
        stride = 0 if rank_psum is not None else src.stride(0)
        _require(psum_out is None or (psum_out.dtype == torch.int32 and psum_out.is_contiguous() and
                                      psum_out.numel() == R), 'psum_out must be contiguous int32 [num_ranks]')
        _require(pad_rows == 0 or (row_map is not None and row_map.dtype == torch.int32 and
                                   row_map.numel() >= num_recv and packed.shape[0] >= pad_rows * R),
                 'padded receive rows need a row map and R * pad_rows packed rows')
        _require(not own_first or (row_map is not None and row_map.dtype == torch.int32 and
                                   row_map.numel() >= num_recv), 'own-first receive rows need a row map')
        rc = self.lib.deepep_dispatch_count(
            ptr(packed), layout.row_bytes, layout.idx_off, layout.src_off, num_recv, layout.num_topk, rank,
            num_local_experts, ptr(src), R, stride, ptr(psum_out), pad_rows, int(own_first), ptr(row_map), ptr(meta),
            ptr(recv_topk_idx), ptr(block_counts), _stream_handle(stream))
        _lib.check(rc, 'dispatch_count')

    def dispatch_receive(self, packed, layout: RowLayout, num_recv, rank, num_local_experts, rank_counts, psum_out,
                         meta, recv_topk_idx, block_counts, expert_alignment, expanded, expert_counts, psum_expert,
                         inv=None, pad_rows: int = 0, row_map=None, own_first: bool = False, stream=None):
        """count (counts mode) -> scan -> slots (expanded) in one call: the receive side's launches back to
        back.  Non-expanded: meta columns 2.. become -1."""
        _require(rank_counts.dim() == 1 and rank_counts.dtype == torch.int32 and rank_counts.stride(0) >= 1,
                 'rank_counts must be an int32 [num_ranks] view')
        R = rank_counts.shape[0]
        _require(psum_out.dtype == torch.int32 and psum_out.is_contiguous() and psum_out.numel() == R,
                 'psum_out must be contiguous int32 [num_ranks]')
        _require(pad_rows == 0 or (row_map is not None and row_map.dtype == torch.int32 and
                                   row_map.numel() >= num_recv and packed.shape[0] >= pad_rows * R),
                 'padded receive rows need a row map and R * pad_rows packed rows')
        _require(not own_first or (row_map is not None and row_map.dtype == torch.int32 and
                                   row_map.numel() >= num_recv), 'own-first receive rows need a row map')
        _require(inv is None or (inv.dtype == torch.int32 and inv.is_contiguous()), 'inv int32')
        rc = self.lib.deepep_dispatch_receive(
            ptr(packed), layout.row_bytes, layout.idx_off, layout.src_off, num_recv, layout.num_topk, rank,
            num_local_experts, ptr(rank_counts), R, rank_counts.stride(0), ptr(psum_out), pad_rows, int(own_first),
            ptr(row_map),
            ptr(meta), ptr(recv_topk_idx), ptr(block_counts), expert_alignment, int(expanded), ptr(expert_counts),
            ptr(psum_expert), ptr(inv), _stream_handle(stream))
        _lib.check(rc, 'dispatch_receive')

    def dispatch_scan(self, block_counts, num_local_experts, expert_alignment, expanded, expert_counts,
                      psum_expert, stream=None):
        rc = self.lib.deepep_dispatch_scan(ptr(block_counts), block_counts.shape[0], num_local_experts,
                                           expert_alignment, int(expanded), ptr(expert_counts), ptr(psum_expert),
                                           _stream_handle(stream))
        _lib.check(rc, 'dispatch_scan')

    def dispatch_slots(self, packed, layout: RowLayout, num_recv, rank, num_local_experts, block_offsets, meta,
                       inv=None, row_map=None, stream=None):
        """inv: optional int32 [expanded rows]: inv[slot] = row * K + lane (the expanded copy's map)."""
        _require(inv is None or (inv.dtype == torch.int32 and inv.is_contiguous()), 'inv int32')
        rc = self.lib.deepep_dispatch_slots(ptr(packed), layout.row_bytes, layout.idx_off, num_recv,
                                            layout.num_topk, rank, num_local_experts, ptr(block_offsets),
                                            ptr(meta), ptr(inv), ptr(row_map), _stream_handle(stream))
        _lib.check(rc, 'dispatch_slots')

    def dispatch_copy(self, packed, layout: RowLayout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                      recv_w, x_direct=None, sf_direct=None, num_max_tokens: int = 0, error_flag=None,
                      inv=None, block_offsets=None, expert_end=None, row_map=None, stream=None):
        """x_direct / sf_direct: [T, bytes] uint8 views of the sender's rows (one rank: the packed rows
        then carry only metadata and row i's x is x_direct[src_metadata[i][0] % num_max_tokens]).
        inv / block_offsets / expert_end (expanded): the blocked destination-major copy (dispatch_slots'
        inverse map, dispatch_scan's per-block offsets [blocks, local experts] and psum_expert)."""
        if inv is not None:
            _require(expanded and block_offsets is not None and expert_end is not None and
                     block_offsets.dim() == 2 and block_offsets.shape[0] ==
                     (num_recv + _lib.DISPATCH_BLOCK_ROWS - 1) // _lib.DISPATCH_BLOCK_ROWS and
                     expert_end.numel() == block_offsets.shape[1], 'blocked copy tables')
        x_bytes = x_direct.shape[1] if x_direct is not None else layout.x_bytes
        sf_bytes = sf_direct.shape[1] if sf_direct is not None else layout.sf_bytes
        rc = self.lib.deepep_dispatch_copy(ptr(packed), layout.row_bytes, x_bytes, layout.sf_off,
                                           sf_bytes, layout.w_off, num_recv, layout.num_topk, ptr(meta),
                                           int(expanded),
                                           ptr(x_direct), x_direct.stride(0) if x_direct is not None else 0,
                                           ptr(sf_direct), sf_direct.stride(0) if sf_direct is not None else 0,
                                           num_max_tokens,
                                           ptr(recv_x_bytes), ptr(recv_sf_bytes), ptr(recv_w),
                                           recv_x_bytes.shape[0], ptr(inv), ptr(block_offsets), ptr(expert_end),
                                           block_offsets.shape[1] if block_offsets is not None else 0,
                                           ptr(row_map), ptr(error_flag), _stream_handle(stream))
        _lib.check(rc, 'dispatch_copy')

    def dispatch_copy_cast(self, packed, layout: RowLayout, num_recv, meta, expanded, recv_x_bytes, recv_sf_bytes,
                           recv_w, x_direct=None, sf_direct=None, num_max_tokens: int = 0, error_flag=None,
                           inv=None, block_offsets=None, expert_end=None, row_map=None, round_scale: bool = False,
                           stream=None, ue8m0: bool = False, mx: bool = False):
        """dispatch_copy's one-rank (x_direct) forms with cast_fp8 fused in: x_direct is the uint8 view [T, 2 * H]
        of the sender's bf16 rows (rows may be strided) and there is no sf_direct; recv_x_bytes [rows, H] gets the
        e4m3fn bytes, recv_sf_bytes [rows, fmt.row_bytes(H)] the scale factors of the format fmt that ue8m0 / mx name
        (sf_format; cast_fp8's conditions).  The other arguments as dispatch_copy."""
        _require(x_direct is not None and sf_direct is None and x_direct.dtype == torch.uint8 and x_direct.dim() == 2,
                 'dispatch_copy_cast reads the bf16 rows of x_direct and takes no sf_direct')
        H = x_direct.shape[1] // 2
        _require(H % 128 == 0 and x_direct.shape[1] == 2 * H and (x_direct.numel() == 0 or x_direct.stride(1) == 1),
                 'dispatch_copy_cast needs bf16 rows of H % 128 == 0 columns with unit column stride')
        fmt = sf_format(ue8m0, mx, 'dispatch_copy_cast')
        fmt.require('dispatch_copy_cast', H, round_scale)
        _require(recv_x_bytes.dtype == torch.uint8 and recv_x_bytes.is_contiguous() and recv_x_bytes.dim() == 2 and
                 recv_x_bytes.shape[1] == H and recv_sf_bytes is not None and recv_sf_bytes.dtype == torch.uint8 and
                 recv_sf_bytes.is_contiguous() and
                 tuple(recv_sf_bytes.shape) == (recv_x_bytes.shape[0], fmt.row_bytes(H)),
                 f'dispatch_copy_cast outputs must be contiguous bytes [rows, H] and, for {fmt}, '
                 f'[rows, {fmt.row_bytes(H)}]')
        if inv is not None:
            _require(expanded and block_offsets is not None and expert_end is not None and
                     block_offsets.dim() == 2 and block_offsets.shape[0] ==
                     (num_recv + _lib.DISPATCH_BLOCK_ROWS - 1) // _lib.DISPATCH_BLOCK_ROWS and
                     expert_end.numel() == block_offsets.shape[1], 'blocked copy tables')
        self._entry('dispatch_copy_cast' + fmt.suffix)(
            ptr(packed), layout.row_bytes, layout.w_off, num_recv, layout.num_topk, ptr(meta), int(expanded),
            ptr(x_direct), x_direct.stride(0) if x_direct.shape[0] else 2 * H, H, *fmt.scale_arg(round_scale),
            num_max_tokens, ptr(recv_x_bytes), ptr(recv_sf_bytes), ptr(recv_w), recv_x_bytes.shape[0], ptr(inv),
            ptr(block_offsets), ptr(expert_end), block_offsets.shape[1] if block_offsets is not None else 0,
            ptr(row_map), ptr(error_flag), _stream_handle(stream))

    def combine_buffer_size(self, num_max_tokens_per_rank: int, hidden: int, num_topk: int,
                            num_ranks: int, allow_multiple_reduction: bool) -> int:
        v = self.lib.deepep_combine_buffer_size(num_max_tokens_per_rank, hidden, num_topk, num_ranks,
                                                int(allow_multiple_reduction))
        _lib.check(0 if v >= 0 else int(v), 'combine_buffer_size')
        return int(v)
