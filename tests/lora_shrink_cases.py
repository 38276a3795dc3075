"""Cases and inputs shared by tests/test_lora_shrink_host.py (CPU) and tests/test_gpu_lora_shrink.py (GPU): the LoRA shrink matmul
``t = x @ lora_A^T`` as a kernel of the library (``bitsandbytes_amd::lora_shrink``, csrc/lora_shrink.hip), the public
``bitsandbytes_amd.lora_shrink`` and ``nn.Linear4bitLoRA.fused_shrink``.

Exact inputs. ``x``: ``exact_inputs.int_rows`` - integers with |x| <= 4, every row distinct. ``A``: drawn from ``lora_cases.B_VALUES``
(0, +-2^-6 ... +-2^-3), every row distinct. Every product is a multiple of 2^-6 and every partial sum is at most K / 2 = 32 K units,
below 2^24 units for K < 524288: every fp32 partial is exact in ANY order, and the reference - float64, rounded once to T - is the only
right answer (asserted on the CPU by the host test, in the manner of ``exact_inputs.assert_exact_sums``).

Shapes, the smallest at which each mechanism of the kernel can go wrong (one workgroup of sixteen wavefronts per EIGHT adapter rows;
wavefront w takes the 32-k steps w, w + 16, ... in batches of eight):
  K = 64      two steps: fourteen wavefronts never load and contribute their zero tile
  K = 2752    86 steps: K % 256 != 0, wavefronts with 6 and with 5 steps, a partly filled batch
  K = 4096    eight steps per wavefront: exactly one batch
  K = 34816   68 steps per wavefront: nine batches, the last one partly filled
  R = 8       one workgroup; a partly filled tile of any height above 8
  R = 24, 128, 136 (crosses a tile of any power-of-two height), 1024 (the cap; K = 64 and K = 4096 only)
  splits (16, 16, 16), (8, 128, 24), eight of 8
every M from 1 to 16, bf16 and fp16. The grid is rotated so that each K meets three of the four small R, every split table and both
dtypes.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import exact_inputs as X
import lora_cases as LC

MS = tuple(range(1, 17))
MAX_ROWS = 16
KS = (64, 2752, 4096, 34816)
RS = (8, 24, 128, 136)
R_CAP = 1024
R_CAP_KS = (64, 4096)
SPLITS = ((16, 16, 16), (8, 128, 24), (8,) * 8)
DTYPES = (torch.bfloat16, torch.float16)
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
UNIT = 2.0 ** -6
A_VALUES = LC.B_VALUES


@dataclass(frozen=True)
class ShrinkCase:
    K: int
    R: int
    dtype: torch.dtype
    splits: Optional[Tuple[int, ...]] = None

    @property
    def name(self) -> str:
        s = "" if self.splits is None else "-s" + "_".join(map(str, self.splits))
        return f"K{self.K}-R{self.R}-{str(self.dtype).split('.')[-1]}{s}"

    @property
    def seed(self) -> int:
        return (self.K * 13 + self.R * 7 + (1 if self.dtype == torch.float16 else 0)) % (1 << 31)


def _cases():
    out = []
    for i, K in enumerate(KS):
        cells = [(RS[(i + j) % len(RS)], None) for j in range(3)]
        if K in R_CAP_KS:
            cells.append((R_CAP, None))
        cells += [(sum(s), s) for s in SPLITS]
        for n, (R, s) in enumerate(cells):
            out.append(ShrinkCase(K, R, DTYPES[(i + n) % 2], s))
    return tuple(out)


CASES = _cases()

# where bnb_mi355x_lora_shrink_supported must answer 1: (M values, R values, K values), both dtypes - the classes that the
# measurements keep (profiles/lora_shrink_bench.txt): K <= 4096 at every M, 4096 < K <= 14336 at 2 ... 4 rows
MUST_SERVE = ((MS, (16, 8, 64, 128, 136, 384, 1024), (4096, 64, 2752)), ((2, 3, 4), (16, 64, 128, 384), (4160, 8192, 14336)))
# the classes the measurements exclude (the C entry point still computes them; the predicate answers 0): (M values, R values, K values)
EXCLUDED = (((1, 5, 8, 9, 16), (16, 64, 128), (4160, 8192, 14336)), (MS, (16, 128), (14400, 34816)))
# outside each precondition: (dtype code, M, R, K)
MUST_REFUSE = ((2, 0, 16, 4096), (2, 17, 16, 4096), (2, 1, 4, 4096), (2, 1, 12, 4096), (2, 1, 1032, 4096), (2, 1, 16, 96), (2, 1, 16, 32),
               (2, 1, 16, 4096 + 32), (0, 1, 16, 4096), (3, 1, 16, 4096), (2, 1, 0, 4096), (2, 1, 16, 0), (2, -1, 16, 4096))


@functools.lru_cache(maxsize=None)
def build(case: ShrinkCase):
    """(x [MAX_ROWS, K], A [R, K]) in the case's dtype: exact inputs, every row of each distinct."""
    gen = torch.Generator().manual_seed(case.seed)
    x = X.int_rows(MAX_ROWS, case.K, case.dtype, gen)
    values = torch.tensor(A_VALUES, dtype=torch.float32)
    a = LC._distinct_rows(lambda n: values[torch.randint(0, len(A_VALUES), (n, case.K), generator=gen)], case.R)
    assert torch.unique(a, dim=0).shape[0] == case.R
    return x, a.to(case.dtype)


def reference(x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """float64, rounded once to the operands' dtype: [rows, R]."""
    return (x.double() @ a.double().t()).to(x.dtype)


def offsets(splits):
    out, pre = [], 0
    for r in splits:
        out.append(pre)
        pre += r
    return out


def parts_of(flat: torch.Tensor, M: int, splits):
    """The contiguous [M, r_i] parts of the flat output buffer of a splits call."""
    return [flat[M * o:M * (o + r)].view(M, r) for o, r in zip(offsets(splits), splits)]


def tolerance(want64: torch.Tensor, x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """Per-element bound on |t - want| for ordinary data: the one rounding to T (u = the largest relative half-ulp of T) and an fp32
    chain of K products and at most K + 3 additions in any order, each within 2^-24 relative of a partial sum whose magnitude the sum
    of product magnitudes bounds - derived, not measured: u |want| + (K + 4) 2^-24 (|x| |A|^T)."""
    K = x.shape[-1]
    u = 2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11
    return u * want64.abs() + (K + 4) * 2.0 ** -24 * (x.double().abs() @ a.double().abs().t())
