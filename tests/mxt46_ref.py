"""The transposed MXFP4 and MXFP6 casts (deepep_amd.cast_to_mxfp4_transposed / cast_to_mxfp6_transposed): their CPU
references and their self-check -- TEST INFRASTRUCTURE ONLY.

The reference is tests/fp4_ref.fp4_pair / tests/fp6_ref.fp6_pair of the transposed, contiguous matrix and nothing
else: the groups of 32 that share an exponent byte run along the token axis, and the result is by definition an
ordinary MXFP4 / MXFP6 pair of x^T.  The row-wise half is the same function of x.  The inputs are tests/mxt_ref's
(every ROW scaled by a power of two of its own over 12 binades), on which the codes of the transposed pair are not
the transposed codes of the row-wise pair (self_check): a kernel that scaled along the wrong axis cannot pass."""
import torch

from tests.fp4_ref import fp4_back_ref, fp4_codes, fp4_pair
from tests.fp6_ref import fp6_back_ref, fp6_codes, fp6_pair, fp6_unpack


class Format:
    """One element type: its public functions' names, the bytes of 32 codes, and its references."""

    def __init__(self, name, bits, pair, codes, back_ref, max_value):
        self.name = name                                    # 'fp4' / 'fp6'
        self.bits = bits
        self.block_bytes = 4 * bits                         # 32 codes
        self.pair, self.codes, self.back_ref = pair, codes, back_ref
        self.max_value = max_value                          # the ceiling rule's constant
        self.public = f'cast_to_mx{name}_transposed'
        self.wrapper = f'cast_{name}_mx_transposed'
        self.entry = f'deepep_cast_{name}_mx_transposed'
        self.rowwise_cast = f'per_token_cast_to_{name}'
        self.cast_back = f'per_token_cast_back_{name}'
        self.dispatch_keyword = f'cast_to_{name}'

    def __repr__(self):
        return self.name

    def row_bytes(self, n: int) -> int:
        """The bytes of a row of n codes."""
        return n * self.bits // 8

    def unpack(self, q: torch.Tensor) -> torch.Tensor:
        """uint8 rows -> int64 [M, n] codes."""
        if self.bits == 6:
            return fp6_unpack(q)
        b = q.cpu().to(torch.int64)
        return torch.stack([b & 0xf, b >> 4], dim=2).view(b.shape[0], 2 * b.shape[1])

    def transposed_pair(self, x: torch.Tensor):
        """(q_t uint8 [H, N * bits / 8], sf_t uint8 [H, N / 32]) of a bf16 x [N, H], on the CPU."""
        return self.pair(x.cpu().t().contiguous())

    def rowwise_pair(self, x: torch.Tensor):
        """(q uint8 [N, H * bits / 8], sf uint8 [N, H / 32]) of a bf16 x [N, H], on the CPU."""
        return self.pair(x.cpu().contiguous())

    def axis_difference(self, x: torch.Tensor) -> float:
        """The share of the reference's unpacked codes that differ from the transposed codes of the row-wise pair."""
        codes_t = self.unpack(self.transposed_pair(x)[0])
        codes = self.unpack(self.rowwise_pair(x)[0])
        return float((codes_t != codes.t()).float().mean())

    def self_check(self, x: torch.Tensor) -> None:
        """The inputs tell the two axes apart: more than half of the codes differ."""
        share = self.axis_difference(x)
        assert share > 0.5, f'only {share:.2f} of the {self.name} codes tell the token axis from the column axis'


FP4 = Format('fp4', 4, fp4_pair, fp4_codes, fp4_back_ref, 6.0)
FP6 = Format('fp6', 6, fp6_pair, fp6_codes, fp6_back_ref, 7.5)
FORMATS = (FP4, FP6)
