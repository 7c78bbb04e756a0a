"""FP8 expert rows into the combine: the CPU kernel provider that takes `src_sf`, the input generators and the
comparison of combine(pair) with combine(cast back of the pair) -- TEST INFRASTRUCTURE ONLY.

The one rule (include/deepep_amd.h, deepep_combine_reduce_fp8): combine((x_fp8, x_scales), handle, ...) returns, bit
for bit, what combine(per_token_cast_back(x_fp8, x_scales), handle, ...) returns with every other argument equal.
Every expected value here is therefore the same provider's bf16 route over the cast-back rows; all inputs hold finite
bytes and positive power-of-two or cast factors, and every expected result is asserted free of NaN and Inf."""
import numpy as np
import torch

from tests.test_fp8_cast_gpu import cast_ref
from tests.ue8m0_ref import Ue8m0OracleKernels, pack_ref, unpack_ref
from workloads import per_token_cast_back as torch_cast_back


def back_cpu(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """bf16 [M, H] of a pair in any of the three scale-factor forms (torch code, on the CPU)."""
    if q.shape[0] == 0:
        return torch.empty(q.shape, dtype=torch.bfloat16)
    sf = sf.cpu()
    sf = unpack_ref(sf) if sf.dtype == torch.int32 else sf.contiguous()
    return torch_cast_back(q.cpu().contiguous(), sf)


class Fp8CombineOracleKernels(Ue8m0OracleKernels):
    """Fp8OracleKernels (through its UE8M0 subclass, so that all three pair forms can be dispatched) whose
    combine_reduce takes `src_sf` as deepep_amd.kernels.HipKernels' does: it asserts what the HIP wrapper requires of
    the pair, casts back with the torch reference and delegates to the bf16 reduce."""
    name = 'oracle-fp8-combine'

    def combine_reduce(self, mode, src, out, num_units, *args, src_sf=None, **kw):
        if src_sf is None:
            return super().combine_reduce(mode, src, out, num_units, *args, **kw)
        assert src.dim() == 2 and src.dtype == torch.float8_e4m3fn and (src.numel() == 0 or src.stride(1) == 1)
        M, H = src.shape
        assert H % 128 == 0 and H > 0 and (M == 0 or src.stride(0) % 16 == 0)
        assert isinstance(src_sf, torch.Tensor) and src_sf.device == src.device
        if src_sf.dtype == torch.int32:
            assert H % 512 == 0 and tuple(src_sf.shape) == (M, H // 512)
        else:
            assert src_sf.dtype == torch.float32 and tuple(src_sf.shape) == (M, H // 128)
        return super().combine_reduce(mode, back_cpu(src, src_sf), out, num_units, *args, **kw)


# ----------------------------------------------------------------------------- inputs
def binade_rows(n: int, H: int, seed: int) -> torch.Tensor:
    """bf16 rows whose 128-column groups span 2^-20 .. 2^20 (as _cast_input of tests/test_ue8m0_gpu.py, without
    its largest-finite column: sums of up to 32 such rows stay finite); group 0 below the cast's 1e-4 clamp, row 0's
    group 0 all zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, H), generator=g) * torch.exp2(torch.randint(-20, 20, (n, H // 128, 1), generator=g).float()
                                                      ).expand(n, H // 128, 128).reshape(n, H)
    x[:, :128] = torch.randn((n, 128), generator=g) * 1e-6
    if n:
        x[0, :128] = 0
    return x.to(torch.bfloat16)


def col_major(sf: torch.Tensor) -> torch.Tensor:
    """The same values with column-major strides (1, rows rounded up to 4), as use_tma_aligned_col_major_sf lays
    scale factors out."""
    out = torch.empty_strided(sf.shape, (1, (sf.shape[0] + 3) // 4 * 4 or 4), dtype=sf.dtype, device=sf.device)
    out.copy_(sf)
    return out


def pair_forms(x: torch.Tensor, device='cpu'):
    """{form: (q, sf)} of bf16 rows x cast on the CPU: 'fp32', 'col_major' and, for H % 512 == 0, 'ue8m0'."""
    q, sf = cast_ref(x, False)
    forms = {'fp32': (q.to(device), sf.to(device)), 'col_major': (q.to(device), col_major(sf.to(device)))}
    if x.shape[1] % 512 == 0:
        q2, sf2 = cast_ref(x, True)
        forms['ue8m0'] = (q2.to(device), pack_ref(sf2).to(device))
    return forms


FINITE_BYTES = np.array([b for b in range(256) if (b & 0x7f) != 0x7f], dtype=np.uint8)     # 254: no NaN byte


def byte_sweep_pair(H: int):
    """254 rows in which every column position sees each of the 254 finite e4m3fn bytes (both zeros and the
    subnormals among them) once; the factor of row r's group g is 2^(((r + g) % 41) - 20).  Returns q and the factors
    as fp32 (pack_ref gives the packed form)."""
    r, c = np.arange(254).reshape(-1, 1), np.arange(H).reshape(1, H)
    q = torch.from_numpy(np.ascontiguousarray(FINITE_BYTES[(r + c) % 254])).view(torch.float8_e4m3fn)
    e = (r + np.arange(H // 128).reshape(1, -1)) % 41 - 20
    return q, torch.from_numpy(np.exp2(e).astype(np.float32))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- combine(pair) against combine(cast back)
READERS = ('combine_reduce', 'combine_reduce_scatter')
PLAN_BUILDERS = ('build_local_plan', 'route_block_counts', 'plan_expert', 'plan_source')


def combine_differences(buf, pair, handle, back, wait: bool = False, **kw):
    """What differs between buf.combine(pair, handle, **kw) and buf.combine(back(*pair), handle, **kw): the output
    bits (signed zeros count), the passed-through weights and the wrapper calls made (buf.kernels is a Spy): the same
    names in the same order, no cast_back_fp8, `src_sf` in the pair's calls that read x and in no bf16 call."""
    spy = buf.kernels
    n0 = len(spy.calls)
    got = buf.combine(pair, handle, **kw)
    if wait:
        got[2].current_stream_wait()
    n1 = len(spy.calls)
    y = back(*pair)
    want = buf.combine(y, handle, **kw)
    if wait:
        want[2].current_stream_wait()
    n2 = len(spy.calls)
    if pair[0].is_cuda:
        torch.cuda.synchronize()
    bad = []
    # (the plan is built once per handle, by whichever of the two calls comes first: not part of the comparison)
    calls_pair = [c for c in spy.calls[n0:n1] if c[0] not in PLAN_BUILDERS]
    calls_bf16 = [c for c in spy.calls[n1:n2] if c[0] not in PLAN_BUILDERS]
    if [c[0] for c in calls_pair] != [c[0] for c in calls_bf16]:
        bad.append(f'wrapper calls {[c[0] for c in calls_pair]} != {[c[0] for c in calls_bf16]}')
    if any(c[0] == 'cast_back_fp8' for c in calls_pair):
        bad.append('the pair combine called cast_back_fp8')
    if any('src_sf' in dict(c[2]) for c in calls_bf16):
        bad.append('a bf16 call names src_sf')
    x_rows = pair[0].shape[0]
    readers = [c for c in calls_pair if c[0] in READERS and
               any(a[0] == 'tensor' and a[2] == 'torch.float8_e4m3fn' for a in c[1] if isinstance(a, tuple) and a)]
    if x_rows and calls_pair and not readers:
        bad.append('no call read the float8 rows')
    if any('src_sf' not in dict(c[2]) for c in readers):
        bad.append('a call read the float8 rows without src_sf')
    assert bool(torch.isfinite(want[0].float()).all()), 'wrongly chosen input: the bf16 route gives NaN / Inf'
    if not (got[0].dtype == torch.bfloat16 and same_bits(got[0], want[0])):
        bad.append('combined_x')
    if not same_bits(got[1], want[1]):
        bad.append('combined_topk_weights')
    return bad


def poison_unnamed_rows(pair, handle):
    """The rows of an expanded pair that no slot of the handle names (the padding of an aligned layout) get NaN
    bytes and NaN factors: a combine that read one could not stay finite."""
    q, sf = pair
    meta = handle.recv_src_metadata
    named = torch.zeros((q.shape[0],), dtype=torch.bool, device=q.device)
    slots = meta[:, 2:].reshape(-1).long()
    named[slots[slots >= 0]] = True
    q.view(torch.uint8)[~named] = 0x7f
    if sf.dtype == torch.float32:
        sf[~named] = float('nan')
    else:
        sf[~named] = -1                                        # exponent bytes 0xff: NaN factors
    return int((~named).sum())


def pair_combine_cases(buf, inputs, empty_inputs, num_experts: int, back, ue8m0: bool = True, single=None):
    """combine(pair) against combine(back(pair)) on what dispatch(x, cast_to_fp8=True, ...) returned, in every form
    and mode the pair composes with (any kernel provider, any device, any rank count: every rank makes the same
    calls).  inputs / empty_inputs: (x, topk_idx, topk_weights), the second for the no-token case (on the ranks that
    have tokens in it, a second full batch).  single: a second buffer built with allow_multiple_reduction=False.
    Returns the list of differences."""
    fails = []
    x, idx, w = inputs
    H = x.shape[1]
    base = dict(topk_idx=idx, topk_weights=w, num_experts=num_experts)

    def run(label, b, xin, dispatch_kw, poison=False, weights=True, **combine_kw):
        pair, _, recv_w, handle, _ = b.dispatch(xin, cast_to_fp8=True, **dispatch_kw)
        if poison:
            poison_unnamed_rows(pair, handle)
        if weights:
            combine_kw['topk_weights'] = recv_w
        bad = combine_differences(b, pair, handle, back, **combine_kw)
        if bad:
            fails.append(f'{label}: {bad}')
        return pair

    expanded = dict(do_expand=True, **base)
    run('expanded, fp32 factors', buf, x, expanded)
    pair = run('expanded, column-major factors', buf, x, dict(use_tma_aligned_col_major_sf=True, **expanded))
    if pair[1].shape[0] > 1 and pair[1].is_contiguous():
        fails.append('the column-major case got contiguous factors')
    if ue8m0 and H % 512 == 0:
        pair = run('expanded, UE8M0 factors', buf, x, dict(fp8_round_scale=True, fp8_use_ue8m0=True, **expanded))
        if pair[1].dtype != torch.int32:
            fails.append('the UE8M0 case got no int32 factors')
    run('expanded, alignment 16, padding rows poisoned', buf, x, dict(expert_alignment=16, **expanded), poison=True)
    run('not expanded', buf, x, base)
    run('expanded, apply_topk_weights', buf, x, expanded, apply_topk_weights=True)
    g = torch.Generator().manual_seed(x.shape[0] * 31 + H)
    b0 = torch.randn(x.shape, generator=g).to(torch.bfloat16).to(x.device)
    b1 = torch.randn(x.shape, generator=g).to(torch.bfloat16).to(x.device)
    run('expanded, bias pair', buf, x, expanded, bias=(b0, b1))
    run('expanded, one bias, no weights', buf, x, expanded, weights=False, bias=b0)
    run('expanded, no CPU sync', buf, x, dict(do_cpu_sync=False, expert_alignment=16, do_zero_padding=True, **expanded))
    x0, idx0, w0 = empty_inputs
    run('no tokens on one rank', buf, x0, dict(do_expand=True, topk_idx=idx0, topk_weights=w0,
                                               num_experts=num_experts))
    if single is not None:
        run('single reduction', single, x, expanded, weights=False)
        run('single reduction, apply_topk_weights, bias', single, x, expanded, apply_topk_weights=True, bias=b0)
        run('single reduction, no CPU sync', single, x,
            dict(do_cpu_sync=False, expert_alignment=16, do_zero_padding=True, **expanded), weights=False)
        run('single reduction, no tokens on one rank', single, x0,
            dict(do_expand=True, topk_idx=idx0, topk_weights=w0, num_experts=num_experts), weights=False)
    return fails


def routed_inputs(seed: int, tokens: int, H: int, K: int, E: int, device='cpu'):
    """Many-binade bf16 rows, masked routing with one token routed nowhere, weights."""
    from deepep_amd import topk_idx_t
    g = torch.Generator().manual_seed(seed)
    x = binade_rows(tokens, H, seed)
    idx = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(tokens)]) if tokens else \
        torch.zeros((0, K), dtype=torch.int64)
    idx[torch.rand((tokens, K), generator=g) < 0.2] = -1
    if tokens:
        idx[tokens // 2] = -1
    w = torch.rand((tokens, K), generator=g) * (idx >= 0)
    return x.to(device), idx.to(topk_idx_t).to(device), w.to(device)
