"""The transposed MXFP8 cast (deepep_amd.cast_to_mxfp8_transposed): its CPU reference and its inputs -- TEST
INFRASTRUCTURE ONLY.

The reference is tests/mx_ref.mx_pair of the transposed, contiguous matrix and nothing else: the groups of 32 that
share an exponent byte run along the token axis, and the result is by definition an ordinary MXFP8 pair of x^T.  The
row-wise half is mx_pair(x).  The inputs scale every ROW by a power of two of its own over 12 binades, so a column's 32
tokens of one group span binades: the bytes of the transposed pair are then not the transposed bytes of the row-wise
pair (self_check), and a kernel that scaled along the wrong axis cannot pass."""
import torch

from tests.mx_ref import mx_pair


def mxt_input(N: int, H: int, seed: int) -> torch.Tensor:
    """bf16 [N, H] on the CPU: randn rows, each times 2^k, k uniform in -6 .. 5."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H), generator=g)
    scale = torch.exp2(torch.randint(-6, 6, (N, 1), generator=g).float())
    return (x * scale).to(torch.bfloat16)


def mxt_pair(x: torch.Tensor):
    """(q_t uint8 [H, N], sf_t uint8 [H, N / 32]) of a bf16 x [N, H], on the CPU."""
    q_t, sf_t = mx_pair(x.cpu().t().contiguous())
    return q_t.view(torch.uint8), sf_t


def rowwise_pair(x: torch.Tensor):
    """(q uint8 [N, H], sf uint8 [N, H / 32]) of a bf16 x [N, H], on the CPU."""
    q, sf = mx_pair(x.cpu().contiguous())
    return q.view(torch.uint8), sf


def axis_difference(x: torch.Tensor) -> float:
    """The share of the reference's e4m3fn bytes that differ from the transposed bytes of the row-wise pair."""
    q_t, _ = mxt_pair(x)
    q, _ = rowwise_pair(x)
    return float((q_t != q.t()).float().mean())


def self_check(x: torch.Tensor) -> None:
    """The inputs tell the two axes apart: more than half of the bytes differ."""
    share = axis_difference(x)
    assert share > 0.5, f'only {share:.2f} of the bytes tell the token axis from the column axis'
