"""Requantisation along the tokens (deepep_amd.requant_mxfp8_transposed / requant_mxfp4_transposed /
requant_mxfp6_transposed): the CPU references, the inputs and the self-checks -- TEST INFRASTRUCTURE ONLY.

The contract is one rule per function: the result is, bit for bit, the transposed cast of the cast back of the pair.
So every reference here is a composition of two existing references and nothing else:
    MXFP8      tests.mxt_ref.mxt_pair(back(q, sf)), back = tests.mx_ref.mx_back_ref for exponent bytes per 32 columns,
               tests.fp8_combine_ref.back_cpu for fp32 and packed UE8M0 factors
    FP4 / FP6  fmt.transposed_pair(fmt.back_ref(q, sf)) over tests.mxt46_ref.FORMATS
The inputs are the casts of tests.mxt_ref.mxt_input(N, H, N + H): every row scaled by a power of two of its own, so
the token-axis blocks span binades and the requantised codes are not the transposed input codes (self-check i); with
fp32 factors that are no powers of two the cast back's product is not a bf16, so its rounding shows in the result
(self-check ii)."""
import torch

from tests.fp8_combine_ref import back_cpu, col_major
from tests.mx_ref import mx_back_ref, mx_pair
from tests.mxt46_ref import FP4, FP6
from tests.mxt_ref import mxt_input, mxt_pair
from tests.test_fp8_cast_gpu import cast_ref
from tests.ue8m0_ref import pack_ref

FP8_FORMS = ('fp32', 'ue8m0', 'mx')                          # the three scale-factor forms of an FP8 pair
FORMS = FP8_FORMS + ('fp4', 'fp6')                           # all five forms


class Form:
    """One of the five forms: its public function, its wrapper and entry, the cast that makes its inputs, its cast
    backs (the reference's and the package's) and the transposed cast the contract composes with."""

    def __init__(self, name):
        self.name = name
        self.fmt = {'fp4': FP4, 'fp6': FP6}.get(name)       # tests.mxt46_ref.Format, None for FP8
        kind = name if self.fmt else 'fp8'
        self.public = f'requant_mx{kind}_transposed'
        self.wrapper = f'requant_{kind}_mx_transposed'
        self.entry = 'deepep_' + self.wrapper
        self.cast_back = 'per_token_cast_back' + (f'_{name}' if self.fmt else '')
        self.transposed_cast = f'cast_to_mx{kind}_transposed'
        self.h_multiple = 512 if name == 'ue8m0' else 128
        self.bits = self.fmt.bits if self.fmt else 8

    def __repr__(self):
        return self.name

    def row_bytes(self, n: int) -> int:
        return n * self.bits // 8

    def cast(self, x: torch.Tensor):
        """The row-wise pair of bf16 x [N, H] in this form, on the CPU (q as stored: float8_e4m3fn or uint8)."""
        if self.fmt:
            return self.fmt.rowwise_pair(x)
        if self.name == 'mx':
            return mx_pair(x.cpu())
        if self.name == 'ue8m0':
            q, sf = cast_ref(x, True)
            return q, pack_ref(sf)
        return cast_ref(x, False)

    def back(self, q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
        """bf16 [N, H] of a pair, on the CPU: the existing reference of the cast back."""
        if self.fmt:
            return self.fmt.back_ref(q, sf)
        return mx_back_ref(q, sf) if self.name == 'mx' else back_cpu(q, sf)

    def transposed(self, y: torch.Tensor):
        """(q_t uint8, sf_t uint8) of bf16 y [N, H], on the CPU: the existing reference of the transposed cast."""
        return self.fmt.transposed_pair(y) if self.fmt else mxt_pair(y)

    def ref(self, q: torch.Tensor, sf: torch.Tensor):
        """The contract: (q_t uint8 [H, N * bits / 8], sf_t uint8 [H, N / 32]) on the CPU."""
        return self.transposed(self.back(q, sf))

    def unpack(self, q: torch.Tensor) -> torch.Tensor:
        """uint8 / float8 rows -> int64 codes, one per element."""
        return self.fmt.unpack(q) if self.fmt else q.cpu().view(torch.uint8).to(torch.int64)


ALL = tuple(Form(n) for n in FORMS)
BY_NAME = {f.name: f for f in ALL}

_inputs = {}


def pair_and_ref(form: Form, N: int, H: int):
    """((q, sf), (q_t, sf_t)) on the CPU for the casts of mxt_input(N, H, N + H): computed once, shared, never
    written to."""
    key = (form.name, N, H)
    if key not in _inputs:
        q, sf = form.cast(mxt_input(N, H, N + H))
        _inputs[key] = ((q, sf), form.ref(q, sf))
    return _inputs[key]


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.uint8)


# ----------------------------------------------------------------------------- self-checks
def code_difference(form: Form, N: int, H: int) -> float:
    """(i) The share of the reference's unpacked codes that differ from the transposed codes of the input pair: the
    requantisation is not a transposition of the bytes."""
    (q, _), (q_t, _) = pair_and_ref(form, N, H)
    return float((form.unpack(q_t) != form.unpack(q).t()).float().mean())


def back_truncating(q: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """workloads.per_token_cast_back for fp32 factors with the round to nearest even replaced by truncation."""
    m, n = q.shape
    prod = (q.to(torch.float32).view(m, -1, 128) * sf.view(m, -1, 1)).view(m, n).contiguous()
    return ((prod.view(torch.int32) >> 16).to(torch.int16)).view(torch.bfloat16)


def rounding_difference(N: int, H: int) -> float:
    """(ii) The share of the reference's q_t bytes, fp32-factor form, that change when the cast back truncates: a
    kernel that skips or alters the bf16 rounding cannot pass."""
    (q, sf), (q_t, _) = pair_and_ref(BY_NAME['fp32'], N, H)
    q_trunc, _ = mxt_pair(back_truncating(q, sf))
    return float((q_trunc != q_t).float().mean())


__all__ = ['ALL', 'BY_NAME', 'FORMS', 'FP8_FORMS', 'Form', 'as_bytes', 'back_truncating', 'code_difference', 'col_major',
           'pair_and_ref', 'rounding_difference']
