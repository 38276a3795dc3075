"""Cases and inputs shared by tests/test_lora_host.py (CPU) and tests/test_gpu_lora.py (GPU): the LoRA adapter term as the epilogue of
the fused matmul (``bitsandbytes_amd::gemm_4bit_lora``), ``matmul_4bit_lora`` and ``nn.Linear4bitLoRA``.

The exact cases use the base operands of tests/exact_inputs.py with ``exps=(-8, -5)`` (unit 2^-10) and adapter operands for which the
adapter term is exact as well: ``t`` integers in [-4, 4], ``B_l`` from {0, +-2^-6 ... +-2^-3}, ``scaling`` 0.5 or 2 - every adapter
product is a multiple of 2^-7, a multiple of the base unit, and the sum of their magnitudes is at most 128 at r = 128. The reference is
``(x64 @ W64.T + bias64 + s * t64 @ B_l64.T)`` rounded once to the output dtype: the only right answer in any summation order.

Shapes ``N x K`` (blocksize 64 unless noted), the smallest at which each mechanism can go wrong on 256 CUs:
  stream (M = 1; M = 2 ... 4 where the plain call stays on the streaming kernel)
    2816 x 2048          ceil(rows / CUs) = 11 and a partial last workgroup
    64 x 34816, bs 128   fewer rows than CUs; 17 segments: more than one phase
    2001 x 6144          odd N; three segments
    4096 x 4096          the exact-geometry shape
  streaming MFMA (M = 2 ... 16)
    4352 x 256           R = 17
    4352 x 8192          ring instances, several tiles
    4096 x 4096          single-item instances
    4096 x 2752          K % 256 != 0
  neither
    2002 x 1024          5 ... 8 rows run the register-transposed kernel: the raw op raises, the public function composes
each in bf16 and fp16, with and without bias, at every M from 1 to 17, at two of the ranks 8 (one 16-byte piece), 24 (three pieces, not
a power of two) and 128 (the cap), rotated over the shapes; nested statistics on 2816 x 2048, 4096 x 4096, 4352 x 256 and 4096 x 2752.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import exact_inputs as X

MS = tuple(range(1, 18))
MAX_ROWS = max(MS)
EXPS = (-8, -5)
K_STREAM, K_SM = 1, 7
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
RANKS = (8, 24, 128)
SCALINGS = (0.5, 2.0)
T_MAX = 4
B_VALUES = (0.0,) + tuple(s * 2.0 ** e for e in (-6, -5, -4, -3) for s in (1.0, -1.0))
ADAPTER_UNIT = 2.0 ** -7          # |t| integer x B_l a multiple of 2^-6 x scaling >= 0.5
ADAPTER_MAX = 128.0               # r x T_MAX x 2^-3 x scaling at r = 128, scaling = 2


@dataclass(frozen=True)
class LoRACase:
    N: int
    K: int
    blocksize: int = 64
    dtype: torch.dtype = torch.bfloat16
    nested: bool = False

    @property
    def name(self) -> str:
        return f"{self.N}x{self.K}-bs{self.blocksize}-{str(self.dtype).split('.')[-1]}" + ("-nested" if self.nested else "")

    @property
    def seed(self) -> int:
        return (self.N * 31 + self.K * 7 + self.blocksize + 9 + (1 if self.nested else 0)) % (1 << 31)

    @property
    def ranks(self):
        """Two of the three ranks, rotated over the shapes; rank i runs with SCALINGS[i]."""
        i = SHAPES.index((self.N, self.K, self.blocksize))
        return (RANKS[i % 3], RANKS[(i + 1) % 3])


STREAM_SHAPES = ((2816, 2048, 64), (64, 34816, 128), (2001, 6144, 64), (4096, 4096, 64))
SM_SHAPES = ((4352, 256, 64), (4352, 8192, 64), (4096, 4096, 64), (4096, 2752, 64))
OTHER_SHAPES = ((2002, 1024, 64),)
NESTED_SHAPES = ((2816, 2048, 64), (4096, 4096, 64), (4352, 256, 64), (4096, 2752, 64))
SHAPES = tuple(dict.fromkeys(STREAM_SHAPES + SM_SHAPES + OTHER_SHAPES))
DTYPES = (torch.bfloat16, torch.float16)
# cases whose exactness assertions (tests/test_lora_host.py) fail: none
EXCLUDED: tuple = ()
CASES = tuple(c for c in ([LoRACase(N, K, bs, dt, False) for (N, K, bs) in SHAPES for dt in DTYPES] +
                          [LoRACase(N, K, bs, dt, True) for (N, K, bs) in NESTED_SHAPES for dt in DTYPES]) if c not in EXCLUDED)
# where bnb_mi355x_gemm_4bit_lora_supported must answer 1 on 256 CUs (plain and nested statistics, every rank)
MUST_SERVE = tuple((s, (1,)) for s in STREAM_SHAPES) + tuple((s, (2, 4, 8, 16)) for s in SM_SHAPES)


def build_case(case: LoRACase) -> X.ExactInputs:
    """The [N, K] base matrix with MAX_ROWS integer activation rows and an integer bias [N]."""
    return X.build(case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=MAX_ROWS, exps=EXPS)


def _distinct_rows(draw, rows: int) -> torch.Tensor:
    """``draw(n)`` -> [n, cols]; rows that repeat an earlier one are drawn again until every row is different from every other."""
    m = draw(rows)
    for _ in range(64):
        _, inverse = torch.unique(m, dim=0, return_inverse=True)
        first = torch.full((int(inverse.max()) + 1,), rows, dtype=torch.long).scatter_reduce(0, inverse, torch.arange(rows), "amin")
        dup = first[inverse] != torch.arange(rows)
        if not bool(dup.any()):
            return m
        m[dup] = draw(int(dup.sum()))
    raise AssertionError("could not make the rows distinct")


def build_adapter(case: LoRACase, r: int):
    """(t [MAX_ROWS, r] integers in [-T_MAX, T_MAX], B_l [N, r] from B_VALUES) in the case's dtype, every row of each distinct."""
    gen = torch.Generator().manual_seed(case.seed * 131 + r)
    values = torch.tensor(B_VALUES, dtype=torch.float32)
    t = _distinct_rows(lambda n: torch.randint(-T_MAX, T_MAX + 1, (n, r), generator=gen).float(), MAX_ROWS)
    b = _distinct_rows(lambda n: values[torch.randint(0, len(B_VALUES), (n, r), generator=gen)], case.N)
    assert torch.unique(t, dim=0).shape[0] == MAX_ROWS and torch.unique(b, dim=0).shape[0] == case.N
    return t.to(case.dtype), b.to(case.dtype)


def adapter_term64(t: torch.Tensor, b: torch.Tensor, scaling: float) -> torch.Tensor:
    return scaling * (t.double() @ b.double().t())


def tolerance(want64: torch.Tensor, y: torch.Tensor, t: torch.Tensor, b: torch.Tensor, scaling: float, dtype: torch.dtype) -> torch.Tensor:
    """Per-element bound on ``|out - want|`` for ordinary data, ``want = y64 + s * t64 @ B_l64.T`` with ``y`` the plain op's output:
    the two roundings to T that separate the fused result, the composition and ``want`` (``u`` = the largest relative half-ulp of T)
    and an fp32 chain of r + 2 operations - derived, not measured."""
    r = t.shape[-1]
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    mag = y.double().abs() + abs(scaling) * (t.double().abs() @ b.double().abs().t())
    tol = u * (want64.abs() + y.double().abs()) * (1 + 2.0 ** -6) + (r + 4) * 2.0 ** -24 * mag
    return tol + 2.0 ** -25 if dtype == torch.float16 else tol
