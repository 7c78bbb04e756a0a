"""A guarding kernel provider -- TEST INFRASTRUCTURE ONLY.

`Guard(inner)` has the interface of deepep_amd.kernels.HipKernels.  Every wrapper call it forwards runs with
its declared outputs moved into an arena `band | range | band` whose bands hold a canary byte; `verify()`
synchronises once and raises if a kernel changed a band -- a store outside what the wrapper's contract lets it
write.  The parity tests compare what is inside an output; this looks at the bytes around it.

It is handed to the kernel-level drivers directly or injected as `buffer._kernels`, as `Spy`
(tests/fp8_oracle_kernels.py) and `OracleKernels` are; wrap it as `Spy(Guard(inner))` where a test reads the spy's
record.  It is device-agnostic (the arenas live on the device of the tensors), so it wraps the CPU stand-ins too.
The product never selects it.

One call:
  1. every tensor argument is grouped by its underlying storage;
  2. a storage that holds a declared output (OUTPUTS) gets the guarded range: the smallest byte range that
     covers every tensor argument of the call in it,
  3. extended only by what the contract lets the kernel write past a view (EXTENSIONS);
  4. an arena `band | range | band` is allocated, the range at its own address modulo 256 (the wrappers'
     alignment checks see no difference), the bands at least BAND_BYTES and one row of the call's widest row;
  5. the range is copied in, every argument of that storage rebuilt as a view of the arena (same dtype, shape,
     strides and offset inside the range), `inner` called, and the range copied back.
All of it is queued on the stream the call launches on (`stream=`, else the current one); nothing synchronises
the host inside a call, and the arenas live until `verify()`.

Not covered: a call made while the stream is capturing a HIP graph is forwarded unguarded (an arena would be
replayed after its release), and a storage registered with `exclude()` -- a symmetric window, which peers address
by its own address -- is left where it is.  Bytes inside a range that belong to no argument (the gaps between the
rows of a strided view) are not watched either: the drivers pre-fill and compare those themselves.
"""
import inspect
import threading
from typing import Dict, List, Tuple

import torch

CANARY = 0x7f              # bf16 / fp32: a huge finite value; e4m3fn: NaN; int32 / int64: above any row, slot or count
BAND_BYTES = 64 * 1024
ALIGN = 256

# Per wrapper: the tensor parameters the kernel may write (deepep_amd/kernels.py; the non-const pointers of
# include/deepep_amd.h).  Workspaces the wrappers allocate themselves are not arguments and not covered.
OUTPUTS: Dict[str, Tuple[str, ...]] = {
    'combine_reduce': ('out', 'out_weights', 'error_flag'),
    'build_local_plan': ('plan', 'wtable'),
    'dispatch_route': ('dst_slot', 'send_counts'),
    'dispatch_notify': ('dst_slot', 'notify', 'send_offsets'),
    'dispatch_expert_counts': ('counts',),
    'route_block_counts': ('tok', 'pairs'),
    'plan_expert': ('table_a', 'wtable_a', 'out_rows', 'error_flag'),
    'plan_source': ('table_b', 'wtable'),
    'dispatch_pack': ('packed', 'error_flag'),
    'dispatch_pack_cast': ('packed', 'error_flag'),
    'cast_fp8': ('q', 'sf'),
    'cast_back_fp8': ('out',),
    'dispatch_count': ('meta', 'recv_topk_idx', 'block_counts', 'psum_out', 'row_map'),
    'dispatch_receive': ('meta', 'recv_topk_idx', 'block_counts', 'psum_out', 'row_map', 'expert_counts',
                         'psum_expert', 'inv'),
    'dispatch_scan': ('block_counts', 'expert_counts', 'psum_expert'),
    'dispatch_slots': ('meta', 'inv'),
    'dispatch_copy': ('recv_x_bytes', 'recv_sf_bytes', 'recv_w', 'error_flag'),
    'dispatch_copy_cast': ('recv_x_bytes', 'recv_sf_bytes', 'recv_w', 'error_flag'),
}

# Wrappers that write no tensor, or whose outputs are raw addresses: combine_reduce_scatter stores its rows at
# window addresses, which tests/test_window_bounds_gpu.py bounds.  (The stream helpers of kernels.py are module
# functions, not wrapper methods.)
PASS_THROUGH = ('combine_buffer_size', 'combine_reduce_scatter')


def _weights_pad_rule(args) -> Dict[str, int]:
    """combine_reduce(weights_pad=p): each of the num_units weight rows is written as max(K, p) floats (the weights,
    then zeros: a packed row's tail line), so the last unit's row may reach past the [units, K] view."""
    ow, pad, units = args.get('out_weights'), int(args.get('weights_pad') or 0), int(args.get('num_units') or 0)
    if ow is None or units <= 0 or pad <= ow.shape[1]:
        return {}
    return {'out_weights': ow.data_ptr() + ((units - 1) * ow.stride(0) + pad) * ow.element_size()}


# Per wrapper: what the contract lets the kernel write past a view, as {parameter: end address}.
EXTENSIONS = {'combine_reduce': _weights_pad_rule}


def _extent(t: torch.Tensor) -> int:
    """Bytes from the first to one past the last element of a view (non-negative strides)."""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _row_bytes(t: torch.Tensor) -> int:
    return t.shape[-1] * t.element_size() if t.dim() else t.element_size()


def _bytes_of(storage, offset: int, size: int, device) -> torch.Tensor:
    return torch.empty((0,), dtype=torch.uint8, device=device).set_(storage, offset, (size,), (1,))


class BandViolation(AssertionError):
    pass


class _Arena:
    def __init__(self, method, params, shapes, buf, start, size):
        self.method, self.params, self.shapes = method, params, shapes
        self.buf, self.start, self.size = buf, start, size


class Guard:
    def __init__(self, inner):
        self._inner = inner
        self._arenas: List[_Arena] = []
        self._excluded: List[Tuple[int, int]] = []
        self._lock = threading.Lock()
        self.guarded_calls = 0

    def exclude(self, tensor: torch.Tensor) -> None:
        """Never move the storage of `tensor` (a symmetric window)."""
        s = tensor.untyped_storage()
        self._excluded.append((s.data_ptr(), s.data_ptr() + s.nbytes()))

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name.startswith('_') or not callable(attr) or name in PASS_THROUGH:
            return attr
        if name not in OUTPUTS:
            raise LookupError(f'Guard: wrapper {name!r} is neither in the declaration table nor a pass-through')

        def guarded(*args, **kwargs):
            return self._call(name, attr, args, kwargs)
        return guarded

    # ------------------------------------------------------------------ one call
    def _call(self, name, fn, args, kwargs):
        sig = inspect.signature(fn)
        bound = sig.bind(*args, **kwargs)
        # a stand-in that takes some of the wrapper's parameters as **kw: they are arguments by name all the same
        var_kw = next((p.name for p in sig.parameters.values() if p.kind == p.VAR_KEYWORD), None)
        extra = bound.arguments.get(var_kw, {}) if var_kw else {}
        named = {k: v for k, v in bound.arguments.items() if k != var_kw}
        named.update(extra)
        tensors = {k: v for k, v in named.items() if isinstance(v, torch.Tensor)}
        cuda = any(t.is_cuda for t in tensors.values())
        stream = named.get('stream')
        ctx = torch.cuda.stream(stream) if cuda and stream is not None else _null()
        with ctx:
            if cuda and torch.cuda.is_current_stream_capturing():
                return fn(*args, **kwargs)
            ends = EXTENSIONS[name](named) if name in EXTENSIONS else {}
            groups: Dict[int, List[str]] = {}
            for k, t in tensors.items():
                if t.numel() and t.untyped_storage().nbytes():
                    groups.setdefault(t.untyped_storage().data_ptr(), []).append(k)
            widest = max([_row_bytes(t) for t in tensors.values()] + [0])
            band = -(-max(BAND_BYTES, widest) // ALIGN) * ALIGN
            moved = []
            for base, params in groups.items():
                if not any(p in OUTPUTS[name] for p in params):
                    continue
                if any(lo <= base < hi for lo, hi in self._excluded):
                    continue
                first = tensors[params[0]]
                storage, device = first.untyped_storage(), first.device
                lo = min(tensors[p].data_ptr() for p in params)
                hi = max(max(tensors[p].data_ptr() + _extent(tensors[p]), ends.get(p, 0)) for p in params)
                if lo < base or hi > base + storage.nbytes():
                    raise BandViolation(f'Guard: {name}({", ".join(params)}): the wrapper\'s contract lets the kernel '
                                        f'write {hi - base - storage.nbytes()} bytes past the allocation')
                size = hi - lo
                buf = torch.empty((2 * band + ALIGN + size,), dtype=torch.uint8, device=device)
                buf.fill_(CANARY)
                start = band + (lo - buf.data_ptr() - band) % ALIGN
                original = _bytes_of(storage, lo - base, size, device)
                inside = buf[start:start + size]
                inside.copy_(original)
                for p in params:
                    t = tensors[p]
                    off = start + t.data_ptr() - lo
                    assert off % t.element_size() == 0 and (buf.data_ptr() + off) % ALIGN == t.data_ptr() % ALIGN
                    (extra if p in extra else bound.arguments)[p] = torch.empty((0,), dtype=t.dtype, device=device).set_(
                        buf.untyped_storage(), off // t.element_size(), t.shape, t.stride())
                shapes = {p: (tuple(tensors[p].shape), str(tensors[p].dtype).replace('torch.', '')) for p in params}
                moved.append((_Arena(name, tuple(params), shapes, buf, start, size), original, inside))
            result = fn(*bound.args, **bound.kwargs)
            for _, original, inside in moved:
                original.copy_(inside)
        with self._lock:
            self._arenas.extend(a for a, _, _ in moved)
            self.guarded_calls += 1
        return result

    # ------------------------------------------------------------------ the check
    def verify(self) -> int:
        """Synchronise once, check every band of every call since the last verify and release the arenas; returns
        the number of arenas checked."""
        with self._lock:
            arenas, self._arenas = self._arenas, []
        if not arenas:
            return 0
        if any(a.buf.is_cuda for a in arenas):
            torch.cuda.synchronize()
        bands = [(a, side, band, origin) for a in arenas
                 for side, band, origin in (('before', a.buf[:a.start], -a.start),
                                            ('after', a.buf[a.start + a.size:], a.size))]
        # one transfer for the verdict of every band; the offsets only of a band that changed
        dirty = torch.stack([(band != CANARY).any() for _, _, band, _ in bands]).tolist()
        for (a, side, band, origin), bad in zip(bands, dirty):
            if bad:
                changed = (band != CANARY).nonzero()
                if changed.numel():
                    first, last = int(changed[0]) + origin, int(changed[-1]) + origin
                    raise BandViolation(
                        f'{a.method}: a store outside the declared output(s) {", ".join(a.params)}: the band {side} '
                        f'the range changed at byte offsets {first} .. {last} relative to the range of {a.size} '
                        f'bytes ({changed.shape[0]} bytes changed); arguments {a.shapes}')
        return len(arenas)


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False
