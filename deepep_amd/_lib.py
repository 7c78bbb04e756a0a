"""ctypes binding of libdeepep_amd.so (C-ABI in include/deepep_amd.h).

The library is built in-tree by __graft_entry__.build() (hipcc --offload-arch=gfx950).
There is no fallback: if the library is missing or a call fails, the error is raised
(RuntimeError, as the reference's EP_HOST_ASSERT -> EPException does).
"""
import ctypes
import hashlib
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DEEPEP_AMD_LIB', os.path.join(_HERE, 'libdeepep_amd.so'))
SOURCES = [os.path.join(_HERE, 'csrc', f) for f in ('combine.hip', 'dispatch.hip', 'symmetric.hip', 'plan.hip',
                                                      'fp8_cast.hip', 'fp4_cast.hip', 'fp6_cast.hip', 'logfmt.hip', 'fault.h',
                                                      'fp8_dequant.h', 'cast_common.h', 'logfmt_codec.h',
                                                      'fp8_cast_t.hip', 'fp8_cast_common.h', 'fp46_cast_t.hip',
                                                      'fp4_cast_common.h', 'fp6_cast_common.h', 'requant_t.hip',
                                                      'fp4_dequant.h', 'fp6_dequant.h')]
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'deepep_amd.h')
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Wall']


def source_build_id() -> Optional[str]:
    """sha256 (16 hex digits) of the library's sources, header and compile flags; None when the
    sources are not next to the package."""
    if not all(os.path.exists(p) for p in SOURCES + [HEADER]):
        return None
    h = hashlib.sha256(' '.join(HIPCC_FLAGS).encode())
    for p in SOURCES + [HEADER]:
        h.update(os.path.basename(p).encode())
        with open(p, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def binary_build_id(path: str) -> Optional[str]:
    """The build id compiled into a library file (read from its bytes, nothing is loaded)."""
    if not os.path.exists(path):
        return None
    with open(path, 'rb') as f:
        data = f.read()
    i = data.find(b'DEEPEP_BUILD_ID=')
    return data[i + 16:i + 32].decode(errors='replace') if i >= 0 else None
ABI_VERSION = 14

MODE_LOCAL, MODE_EPILOGUE, MODE_FUSED = 0, 1, 2
SF_FORM_FP32, SF_FORM_UE8M0_PACKED, SF_FORM_MX = 0, 1, 2     # DEEPEP_SF_FORM_*: deepep_requant_fp8_mx_transposed

# error record of the window paths (DEEPEP_ERROR_RECORD_INTS, DEEPEP_FLAG_*, DEEPEP_FAULT_*)
ERROR_RECORD_INTS = 8
FLAG_BAD_SLOT, FLAG_TIMEOUT, FLAG_BAD_ADDRESS = 1, 2, 4
FAULT_NAMES = {1: 'scatter row outside every window', 2: 'plan window row past its window',
               3: 'plan unit / received row out of range', 4: 'dispatch row past its destination buffer'}


def describe_error_record(rec) -> str:
    """Human-readable text of an error record (a sequence of DEEPEP_ERROR_RECORD_INTS ints)."""
    rec = [int(v) for v in rec]
    bits = [n for b, n in ((FLAG_BAD_SLOT, 'rejected slot / unit'), (FLAG_TIMEOUT, 'barrier timeout'),
                           (FLAG_BAD_ADDRESS, 'address outside every window')) if rec[0] & b]
    text = f'error flag {rec[0]} ({", ".join(bits) or "none"})'
    if len(rec) > 6 and rec[1]:
        addr = (rec[5] & 0xffffffff) << 32 | (rec[4] & 0xffffffff)
        text += (f'; first fault: {FAULT_NAMES.get(rec[1], rec[1])}, unit/row {rec[2]}, rank/lane {rec[3]}, '
                 f'address {addr:#x}, extent {rec[6]}')
    return text

# deepep_plan_* (include/deepep_amd.h)
PLAN_BLOCK_TOKENS = 64
DISPATCH_BLOCK_ROWS = 128          # DEEPEP_DISPATCH_BLOCK_ROWS: receive-side block of the dispatch
PLAN_EXPANDED, PLAN_SINGLE, PLAN_INTERLEAVE, PLAN_RANK_LAYOUT, PLAN_WINDOW, PLAN_LOCAL_BYPASS = 1, 2, 4, 8, 16, 32

_lib = None
_lock = threading.Lock()

_P = ctypes.c_void_p
_I = ctypes.c_int
_I64 = ctypes.c_int64

# Every symbol include/deepep_amd.h declares, with its ctypes signature.
SIGNATURES = {
    'deepep_amd_abi_version': (_I, []),
    'deepep_amd_last_error': (ctypes.c_char_p, []),
    'deepep_amd_build_id': (ctypes.c_char_p, []),
    'deepep_combine_reduce': (_I, [_I, _I,
                                   _P, _I64, _I64,
                                   _P, _I64, _I,
                                   _P,
                                   _P, _P,
                                   _P, _I64,
                                   _I, _I,
                                   _P, _I64,
                                   _P, _P, _I,
                                   _I64, _I,
                                   _I, _P,
                                   _P]),
    # the FP8-source forms: their siblings' arguments with (sf, sf_row_stride, sf_col_stride, sf_packed) after src
    'deepep_combine_reduce_fp8': (_I, [_I, _I,
                                       _P, _I64, _I64,
                                       _P, _I64, _I64, _I,
                                       _P, _I64, _I,
                                       _P,
                                       _P, _P,
                                       _P, _I64,
                                       _I, _I,
                                       _P, _I64,
                                       _P, _P, _I,
                                       _I64, _I,
                                       _I, _P,
                                       _P]),
    'deepep_combine_reduce_scatter_fp8': (_I, [_I, _P, _I64, _I64, _P, _I64, _I64, _I, _P, _I64, _I, _P, _P, _I, _I, _P,
                                               _I64, _P, _I, _I64, _I, _P, _I, _I64, _P, _P]),
    'deepep_build_local_plan': (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _P]),
    'deepep_set_launch_config': (_I, [_I, _I]),
    'deepep_combine_buffer_size': (_I64, [_I, _I, _I, _I, _I]),
    'deepep_dispatch_route': (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P]),
    'deepep_dispatch_notify': (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I64, _P]),
    'deepep_dispatch_notify_workspace': (_I64, [_I, _I, _I]),
    'deepep_dispatch_receive': (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _P,
                                     _P, _P, _P]),
    'deepep_dispatch_expert_counts': (_I, [_P, _I, _I, _I, _P, _P]),
    'deepep_dispatch_pack': (_I, [_P, _I64, _I, _P, _I64, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                  _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_cast_fp8': (_I, [_P, _I64, _I, _I, _I, _P, _P, _P]),
    'deepep_cast_back_fp8': (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _P, _P]),
    'deepep_dispatch_pack_cast': (_I, [_P, _I64, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                       _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_dispatch_copy_cast': (_I, [_P, _I64, _I, _I, _I, _P, _I, _P, _I64, _I, _I, _I, _P, _P, _P, _I64,
                                       _P, _P, _P, _I, _P, _P, _P]),
    # the packed UE8M0 forms: their siblings' arguments without round_scale
    'deepep_cast_fp8_ue8m0': (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    'deepep_cast_back_fp8_ue8m0': (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _P, _P]),
    'deepep_dispatch_pack_cast_ue8m0': (_I, [_P, _I64, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                             _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_dispatch_copy_cast_ue8m0': (_I, [_P, _I64, _I, _I, _I, _P, _I, _P, _I64, _I, _I, _P, _P, _P, _I64,
                                             _P, _P, _P, _I, _P, _P, _P]),
    # the MXFP8 forms (one UE8M0 byte per 32 columns): the argument lists of the packed UE8M0 forms
    'deepep_cast_fp8_mx': (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    'deepep_cast_back_fp8_mx': (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _P, _P]),
    'deepep_dispatch_pack_cast_mx': (_I, [_P, _I64, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                          _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_dispatch_copy_cast_mx': (_I, [_P, _I64, _I, _I, _I, _P, _I, _P, _I64, _I, _I, _P, _P, _P, _I64,
                                          _P, _P, _P, _I, _P, _P, _P]),
    # the transposed MXFP8 cast (csrc/fp8_cast_t.hip): x, row stride, q_t, sf_t, q and sf (both NULL: no row-wise
    # pair), rows, hidden, stream
    'deepep_cast_fp8_mx_transposed': (_I, [_P, _I64, _P, _P, _P, _P, _I, _I, _P]),
    # the transposed MXFP4 / MXFP6 casts (csrc/fp46_cast_t.hip): the transposed MXFP8 cast's arguments
    'deepep_cast_fp4_mx_transposed': (_I, [_P, _I64, _P, _P, _P, _P, _I, _I, _P]),
    'deepep_cast_fp6_mx_transposed': (_I, [_P, _I64, _P, _P, _P, _P, _I, _I, _P]),
    # the requantisation along the tokens (csrc/requant_t.hip): q, row stride, sf, its row and column strides (in
    # elements), [FP8: sf_form,] q_t, sf_t, rows, hidden, stream
    'deepep_requant_fp8_mx_transposed': (_I, [_P, _I64, _P, _I64, _I64, _I, _P, _P, _I, _I, _P]),
    'deepep_requant_fp4_mx_transposed': (_I, [_P, _I64, _P, _I64, _I64, _P, _P, _I, _I, _P]),
    'deepep_requant_fp6_mx_transposed': (_I, [_P, _I64, _P, _I64, _I64, _P, _P, _I, _I, _P]),
    # MXFP4 (csrc/fp4_cast.hip: e2m1 rows of hidden / 2 bytes, one UE8M0 byte per 32 columns): the MXFP8 forms' arguments
    'deepep_cast_fp4_mx': (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    'deepep_cast_back_fp4_mx': (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _P, _P]),
    'deepep_dispatch_pack_cast_fp4_mx': (_I, [_P, _I64, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                              _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_dispatch_copy_cast_fp4_mx': (_I, [_P, _I64, _I, _I, _I, _P, _I, _P, _I64, _I, _I, _P, _P, _P, _I64,
                                              _P, _P, _P, _I, _P, _P, _P]),
    # MXFP6 (csrc/fp6_cast.hip: e2m3 rows of 3 * hidden / 4 bytes, one UE8M0 byte per 32 columns): the MXFP4 forms'
    # arguments; cast_fp6_mx_stores takes the width of the cast's row stores (8 or 16) before the stream
    'deepep_cast_fp6_mx': (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    'deepep_cast_fp6_mx_stores': (_I, [_P, _I64, _I, _I, _P, _P, _I, _P]),
    'deepep_cast_back_fp6_mx': (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _P, _P]),
    'deepep_dispatch_pack_cast_fp6_mx': (_I, [_P, _I64, _I, _P, _P, _I, _I, _I, _P, _P, _I,
                                              _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P]),
    'deepep_dispatch_copy_cast_fp6_mx': (_I, [_P, _I64, _I, _I, _I, _P, _I, _P, _I64, _I, _I, _P, _P, _P, _I64,
                                              _P, _P, _P, _I, _P, _P, _P]),
    # LogFMT-10 (csrc/logfmt_codec.h): the codec, the exchange-row pack and the epilogue over LogFMT rows
    'deepep_cast_logfmt': (_I, [_P, _I64, _I, _I, _P, _P, _P]),
    'deepep_cast_back_logfmt': (_I, [_P, _I64, _P, _I64, _I, _I, _P, _P]),
    'deepep_logfmt_pack_rows': (_I, [_P, _I64, _I, _I, _I, _I, _P, _I64, _I, _P]),
    'deepep_combine_reduce_logfmt': (_I, [_I,
                                          _P, _I64, _I64,
                                          _P, _I64,
                                          _P, _I64, _I,
                                          _P,
                                          _P, _P,
                                          _P, _I64,
                                          _I, _I,
                                          _P, _I64,
                                          _P, _P, _I,
                                          _I64, _I,
                                          _P, _P]),
    'deepep_dispatch_count': (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    'deepep_dispatch_scan': (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    'deepep_dispatch_slots': (_I, [_P, _I64, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    'deepep_dispatch_copy': (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I64, _P, _I64, _I,
                                  _P, _P, _P, _I64, _P, _P, _P, _I, _P, _P, _P]),
    'deepep_route_block_counts': (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P]),
    'deepep_plan_expert': (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I64, _I64, _P, _P, _I,
                                _P]),
    'deepep_plan_source': (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I64, _I64, _P, _I, _P, _I, _P]),
    'deepep_sym_alloc': (_I, [_I64, ctypes.POINTER(ctypes.c_void_p)]),
    'deepep_sym_free': (_I, [_P]),
    'deepep_sym_export': (_I, [_P, _P]),
    'deepep_sym_import': (_I, [_P, ctypes.POINTER(ctypes.c_void_p)]),
    'deepep_sym_close': (_I, [_P]),
    'deepep_sym_barrier': (_I, [_P, _I, _I, _I64, _I64, _P, _P]),
    'deepep_sym_put': (_I, [_P, _I64, _P, _I, _I64, _I64, _P, _P]),
    'deepep_sym_signal': (_I, [_P, _I, _I, _I, _I64, _P]),
    'deepep_sym_wait': (_I, [_P, _I, _I, _I, _I64, _I64, _P, _P]),
    'deepep_stream_create_cu_budget': (_I, [_I, ctypes.POINTER(ctypes.c_void_p)]),
    'deepep_stream_destroy': (_I, [_P]),
    'deepep_stream_probe_cus': (_I, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    'deepep_combine_reduce_scatter': (_I, [_I, _P, _I64, _I64, _P, _I64, _I, _P, _P, _I, _I, _P, _I64, _P, _I,
                                           _I64, _I, _P, _I, _I64, _P, _P]),
    # the scatter storing LogFMT wire rows: deepep_combine_reduce_scatter's arguments
    'deepep_combine_reduce_scatter_logfmt': (_I, [_I, _P, _I64, _I64, _P, _I64, _I, _P, _P, _I, _I, _P, _I64, _P, _I,
                                                  _I64, _I, _P, _I, _I64, _P, _P]),
}


class LibraryMissing(RuntimeError):
    pass


def load(path: Optional[str] = None):
    """Load (once) and return the ctypes library; raise LibraryMissing if absent."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise LibraryMissing(f'deepep_amd: HIP library not found at {p}; run __graft_entry__.build()')
        want = source_build_id() if path is None and 'DEEPEP_AMD_LIB' not in os.environ else None
        if want is not None and binary_build_id(p) != want:
            raise RuntimeError(f'deepep_amd: {p} was built from other sources (build id {binary_build_id(p)}, '
                               f'sources {want}); run __graft_entry__.build()')
        lib = ctypes.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        version = lib.deepep_amd_abi_version()
        if version != ABI_VERSION:
            raise RuntimeError(f'deepep_amd: ABI version {version} != expected {ABI_VERSION}')
        if path is None:
            _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().deepep_amd_last_error().decode(errors='replace')
        raise RuntimeError(f'deepep_amd: {what} failed ({rc}): {msg}')


def ptr(t) -> Optional[int]:
    """Raw device address of a tensor (None for None)."""
    return None if t is None else t.data_ptr()
