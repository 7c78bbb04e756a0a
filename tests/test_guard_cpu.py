"""The guarding kernel provider (tests/guard.py) without a GPU: a store just outside a declared output is caught
and named, the weights_pad rule admits exactly what the contract admits, the declaration table covers every
wrapper of HipKernels with real parameter names, and a guarded run of the CPU stand-ins is bit for bit the
unguarded run.  This is the proof that tests/test_guard_gpu.py can fail."""
import inspect
import os
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepep_amd.kernels import HipKernels
from tests.guard import BAND_BYTES, CANARY, EXTENSIONS, OUTPUTS, PASS_THROUGH, BandViolation, Guard
from tests.helpers import load, ranks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the kernels may write, wrapper by wrapper, stated a second time: an output dropped from the table of
# tests/guard.py fails the comparison below and its stray-store case.
DECLARED = [
    ('combine_reduce', 'out'), ('combine_reduce', 'out_weights'), ('combine_reduce', 'error_flag'),
    ('build_local_plan', 'plan'), ('build_local_plan', 'wtable'),
    ('dispatch_route', 'dst_slot'), ('dispatch_route', 'send_counts'),
    ('dispatch_notify', 'dst_slot'), ('dispatch_notify', 'notify'), ('dispatch_notify', 'send_offsets'),
    ('dispatch_expert_counts', 'counts'),
    ('route_block_counts', 'tok'), ('route_block_counts', 'pairs'),
    ('plan_expert', 'table_a'), ('plan_expert', 'wtable_a'), ('plan_expert', 'out_rows'), ('plan_expert', 'error_flag'),
    ('plan_source', 'table_b'), ('plan_source', 'wtable'),
    ('dispatch_pack', 'packed'), ('dispatch_pack', 'error_flag'),
    ('dispatch_pack_cast', 'packed'), ('dispatch_pack_cast', 'error_flag'),
    ('cast_fp8', 'q'), ('cast_fp8', 'sf'),
    ('cast_back_fp8', 'out'),
    ('dispatch_count', 'meta'), ('dispatch_count', 'recv_topk_idx'), ('dispatch_count', 'block_counts'),
    ('dispatch_count', 'psum_out'), ('dispatch_count', 'row_map'),
    ('dispatch_receive', 'meta'), ('dispatch_receive', 'recv_topk_idx'), ('dispatch_receive', 'block_counts'),
    ('dispatch_receive', 'psum_out'), ('dispatch_receive', 'row_map'), ('dispatch_receive', 'expert_counts'),
    ('dispatch_receive', 'psum_expert'), ('dispatch_receive', 'inv'),
    ('dispatch_scan', 'block_counts'), ('dispatch_scan', 'expert_counts'), ('dispatch_scan', 'psum_expert'),
    ('dispatch_slots', 'meta'), ('dispatch_slots', 'inv'),
    ('dispatch_copy', 'recv_x_bytes'), ('dispatch_copy', 'recv_sf_bytes'), ('dispatch_copy', 'recv_w'),
    ('dispatch_copy', 'error_flag'),
    ('dispatch_copy_cast', 'recv_x_bytes'), ('dispatch_copy_cast', 'recv_sf_bytes'), ('dispatch_copy_cast', 'recv_w'),
    ('dispatch_copy_cast', 'error_flag'),
]


def _wrappers():
    return sorted(n for n, v in vars(HipKernels).items() if callable(v) and not n.startswith('_'))


# ----------------------------------------------------------------------------- the table
def test_every_wrapper_is_declared_or_passed_through():
    names = _wrappers()
    assert len(names) >= 20 and 'combine_reduce' in names and 'dispatch_copy_cast' in names
    missing = [n for n in names if n not in OUTPUTS and n not in PASS_THROUGH]
    assert not missing, f'wrappers in neither the declaration table nor the pass-through list: {missing}'
    assert not set(OUTPUTS) & set(PASS_THROUGH)
    stale = [n for n in list(OUTPUTS) + list(PASS_THROUGH) + list(EXTENSIONS) if n not in names]
    assert not stale, f'not wrappers of HipKernels: {stale}'
    assert sorted((m, p) for m, ps in OUTPUTS.items() for p in ps) == sorted(DECLARED)


def test_every_declared_output_is_a_parameter_of_its_wrapper():
    for method, outs in OUTPUTS.items():
        params = inspect.signature(getattr(HipKernels, method)).parameters
        for p in outs:
            assert p in params, f'{method} has no parameter {p!r}'
    params = inspect.signature(HipKernels.combine_reduce).parameters
    assert {'out_weights', 'weights_pad', 'num_units'} <= set(params)        # what the weights_pad rule reads


def test_an_undeclared_wrapper_raises_and_a_pass_through_is_forwarded():
    class Inner:
        name = 'inner'

        def combine_buffer_size(self, *a):
            return 7

        def brand_new_kernel(self, out):
            out.fill_(1)

    g = Guard(Inner())
    assert g.name == 'inner' and g.combine_buffer_size(1, 2, 3, 4, True) == 7
    with pytest.raises(LookupError, match='brand_new_kernel'):
        g.brand_new_kernel(torch.zeros(4))


# ----------------------------------------------------------------------------- stray stores
class _Stray:
    """Every wrapper of HipKernels, by its signature: fills the parameter `param` with ones and, with `where`,
    stores one element more through the argument's storage -- 'after': directly behind the view, 'before': directly
    in front of it, 'far': at the far end of a band of BAND_BYTES behind it."""

    def __init__(self, param, where):
        self.param, self.where = param, where

    def __getattr__(self, name):
        sig = inspect.signature(getattr(HipKernels, name))
        sig = sig.replace(parameters=list(sig.parameters.values())[1:])          # without self

        def method(*args, **kwargs):
            t = sig.bind(*args, **kwargs).arguments[self.param]
            t.fill_(1)
            n = t.numel()                                                        # the test's views are contiguous
            at = {None: None, 'after': n, 'before': -1, 'far': n + BAND_BYTES // t.element_size() - 1}[self.where]
            if at is not None:
                torch.as_strided(t, (1,), (1,), t.storage_offset() + at).fill_(1)
        method.__signature__ = sig
        return method


def _call(provider, method, param, dtype=torch.int32, device='cpu', **more):
    """Call `method` with a [4, 8] view in the middle of a larger allocation as `param`, None for the rest.  (The
    allocation is larger than view and band, so that a stray store of an unguarded call still lands in it.)"""
    backing = torch.zeros((4 * BAND_BYTES // 4,), dtype=dtype, device=device)
    lo = 2 * BAND_BYTES // 4
    view = backing[lo:lo + 32].view(4, 8)
    required = [p.name for p in list(inspect.signature(getattr(HipKernels, method)).parameters.values())[1:]
                if p.default is p.empty and p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]
    kwargs = {name: None for name in required}
    kwargs[param] = view
    kwargs.update(more)
    getattr(provider, method)(**kwargs)
    return backing, lo


@pytest.mark.parametrize('method,param', DECLARED)
def test_a_store_just_outside_a_declared_output_is_caught(method, param):
    size = 32 * 4
    for where, side, offset in (('after', 'after', size), ('before', 'before', -4),
                                ('far', 'after', size + BAND_BYTES - 4)):
        g = Guard(_Stray(param, where))
        backing, lo = _call(g, method, param)
        with pytest.raises(BandViolation) as e:
            g.verify()
        msg = str(e.value)
        assert msg.startswith(f'{method}:') and param in msg and f'the band {side} the range' in msg, msg
        assert f'at byte offsets {offset} .. {offset + 3} ' in msg and '(4, 8)' in msg, msg
        # the range came back, the stray store stayed in the arena
        assert int(backing.sum()) == 32 and int(backing[lo:lo + 32].sum()) == 32
        assert g.verify() == 0                                  # the arenas of a failed verify are released
    g = Guard(_Stray(param, None))
    backing, lo = _call(g, method, param)
    assert g.verify() == 1 and int(backing.sum()) == 32


def test_the_canary_reads_as_no_benign_value():
    band = torch.full((8,), CANARY, dtype=torch.uint8)
    assert float(band.view(torch.bfloat16)[0]) > 1e38 and float(band.view(torch.float32)[0]) > 1e38
    assert bool(band.view(torch.float8_e4m3fn).float().isnan().all())
    assert int(band.view(torch.int32)[0]) > 2 ** 30 and int(band.view(torch.int64)[0]) > 2 ** 62


# ----------------------------------------------------------------------------- the weights_pad rule
class _PadFake:
    """combine_reduce as the contract states it: num_units rows of `out`, and per unit max(K, weights_pad) floats
    from the start of its out_weights row.  `more`: floats written past that on the last row."""

    def __init__(self, more=0):
        self.more = more

    def combine_reduce(self, mode, src, out, num_units, table=None, row_weights=None, bias0=None, bias1=None,
                       wtable=None, wsrc=None, out_weights=None, units_per_block=0, error_flag=None, weights_pad=0,
                       stream=None, src_sf=None):
        out[:num_units] = 1
        n = max(out_weights.shape[1], weights_pad)
        for u in range(num_units):
            width = n + (self.more if u == num_units - 1 else 0)
            torch.as_strided(out_weights, (width,), (1,), out_weights.storage_offset() + u * out_weights.stride(0)
                             ).fill_(2)


def _packed_rows(units, H, K):
    backing = torch.zeros((units + 2, H + 128), dtype=torch.bfloat16)
    packed = backing[:units]                                     # the last unit's tail line ends the view
    return backing, packed[:, :H], packed.view(torch.float32)[:, H // 2:H // 2 + K]


def test_weights_pad_floats_per_row_are_allowed_and_not_one_more():
    units, H, K = 5, 256, 8
    for pad in (0, 32):
        g = Guard(_PadFake())
        backing, out, ow = _packed_rows(units, H, K)
        g.combine_reduce(0, None, out, units, out_weights=ow, weights_pad=pad)
        assert g.verify() == 1
        tail = backing.view(torch.float32)[:units, H // 2:]
        assert bool((tail[:, :max(K, pad)] == 2).all()) and bool((tail[:, max(K, pad):] == 0).all())
        assert bool((backing[units:] == 0).all())
        g = Guard(_PadFake(more=1))
        backing, out, ow = _packed_rows(units, H, K)
        g.combine_reduce(0, None, out, units, out_weights=ow, weights_pad=pad)
        with pytest.raises(BandViolation) as e:
            g.verify()
        msg = str(e.value)
        assert msg.startswith('combine_reduce:') and 'out_weights' in msg and 'the band after the range' in msg, msg
        assert bool((backing[units:] == 0).all())               # the float too many stayed in the arena
    # a contract that reaches past the allocation is refused before anything is launched
    ow = torch.zeros((units, K))
    with pytest.raises(BandViolation, match='past the allocation'):
        Guard(_PadFake()).combine_reduce(0, None, torch.zeros((units, H), dtype=torch.bfloat16), units, out_weights=ow,
                                         weights_pad=32)
    assert bool((ow == 0).all())


def test_the_fuzz_seeds_of_the_gpu_file_cover_the_edge_shapes():
    """tests/test_guard_gpu.py runs eight seeds of the tests/test_fuzz_gpu.py sweep under the guard."""
    from tests.test_fuzz_gpu import _case
    from tests.test_guard_gpu import FUZZ_SEEDS
    assert len(FUZZ_SEEDS) == 8
    shapes = [_case(seed)[1:5] for seed in FUZZ_SEEDS]
    tokens = {s[0] for s in shapes}
    assert {0, 1} <= tokens and tokens & {7, 129, 300}, shapes                      # none, one, ragged
    assert any(K < E for _, _, K, E in shapes) and any(K == E for _, _, K, E in shapes), shapes
    assert {s[1] for s in shapes} >= {8, 64, 1024, 2056, 4104}, shapes


# ----------------------------------------------------------------------------- transparency
def _bits_equal(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _layer(buf, x, idx, w, E, bias, fp8):
    """Dispatches and combines of one buffer; returns [(label, dispatch result or combine outputs)]."""
    out = []
    d = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E)
    out.append(('dispatch', d))
    out.append(('combine', buf.combine(d[0], d[3], topk_weights=d[2], bias=bias)[:2]))
    e = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True, expert_alignment=4,
                     do_zero_padding=True)             # (padding rows nobody writes are compared zeroed only)
    out.append(('expanded dispatch', e))
    out.append(('expanded combine', buf.combine(e[0], e[3], topk_weights=e[2])[:2]))
    out.append(('weighted combine', buf.combine(e[0], e[3], topk_weights=e[2], bias=bias, apply_topk_weights=True)[:2]))
    p = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True, do_cpu_sync=False,
                     do_zero_padding=True)
    out.append(('no-CPU-sync dispatch', p))
    out.append(('padded-plan combine', buf.combine(p[0], p[3], topk_weights=p[2])[:2]))
    if fp8:
        for ue8m0 in (False, True):
            kw = dict(fp8_round_scale=True, fp8_use_ue8m0=True) if ue8m0 else {}
            q = buf.dispatch(x, topk_idx=idx, topk_weights=w, num_experts=E, do_expand=True, cast_to_fp8=True, **kw)
            out.append((f'casting dispatch ue8m0={ue8m0}', q))
            out.append((f'pair combine ue8m0={ue8m0}', buf.combine(q[0], q[3], topk_weights=q[2])[:2]))
    return out


def _transparency(group, rank, fixture, fp8):
    """The same calls through the stand-in and through Guard(stand-in): what differs, bit for bit."""
    from deepep_amd import ElasticBuffer, topk_idx_t
    from tests.fp8_combine_ref import Fp8CombineOracleKernels
    from tests.fp8_oracle_kernels import dispatch_differences
    from tests.oracle_kernels import OracleKernels
    fx = load(fixture)
    T, H, K, E, _ = (int(v) for v in fx['meta'])
    me = ranks_of(fx)[rank]
    idx = torch.from_numpy(me['topk_idx'].copy()).to(topk_idx_t)
    w = torch.from_numpy(me['topk_weights'].copy())
    x = (torch.randn((T, H), generator=torch.Generator().manual_seed(rank)) * 3).to(torch.bfloat16)
    bias = torch.from_numpy(me['bias0'].view('int16').copy()).view(torch.bfloat16)
    runs = []
    guard = Guard(Fp8CombineOracleKernels() if fp8 else OracleKernels())
    for kernels in (Fp8CombineOracleKernels() if fp8 else OracleKernels(), guard):
        buf = ElasticBuffer(group, num_max_tokens_per_rank=T, hidden=H, num_topk=K, explicitly_destroy=True)
        buf._kernels = kernels
        runs.append(_layer(buf, x, idx, w, E, bias, fp8))
        buf.destroy()
    fails = []
    for (label, want), (_, got) in zip(*runs):
        if 'dispatch' in label:
            fails += [f'{label}: {d}' for d in dispatch_differences(got, want)]
        elif not (_bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])):
            fails.append(label)
    if not guard.guarded_calls >= 10:
        fails.append(f'only {guard.guarded_calls} calls went through the guard')
    if not guard.verify() >= guard.guarded_calls:
        fails.append('fewer arenas than guarded calls')
    return fails


def test_a_guarded_one_rank_layer_is_the_unguarded_one():
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29576')
        dist.init_process_group('gloo', rank=0, world_size=1)
    fails = _transparency(dist.group.WORLD, 0, 'f1_ep1_t128_h1024_k2.npz', fp8=True)
    assert not fails, fails


def _worker(rank, world, port, fixture, queue):
    import sys
    sys.path.insert(0, ROOT)
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        fails = _transparency(dist.group.WORLD, rank, fixture, fp8=False)
        queue.put((rank, fails))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        queue.put((rank, [traceback.format_exc()]))


def test_a_guarded_four_rank_gloo_layer_is_the_unguarded_one():
    from tests.test_buffer_cpu import _free_port
    world = 4
    ctx = mp.get_context('spawn')
    queue = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, 'f4_ep4_t96_h256_k2.npz', queue)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, fails = queue.get(timeout=240)
            results[rank] = fails
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert sorted(results) == list(range(world)), results
    bad = {r: f for r, f in results.items() if f}
    assert not bad, bad
