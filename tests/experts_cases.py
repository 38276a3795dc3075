"""Cases and inputs shared by tests/test_experts_host.py (CPU) and tests/test_gpu_experts.py (GPU): the expert-indexed fused
matmul ``bitsandbytes_amd::gemm_4bit_experts``.

The exact cases use the operands of tests/exact_inputs.py: the expert stack is ``exact_inputs.build(E * N, K, ...)`` viewed as
``[E, N, K]`` (with nested statistics the groups of 256 blocks then straddle experts by construction), so that every
``y[t, s, :]`` is known to the last bit whatever the order of summation.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import exact_inputs as X

P_VALUES = (1, 2, 5, 16, 64, 65, 200)
# P -> (T, S): P = T * S pairs
TS_OF_P = {1: (1, 1), 2: (1, 2), 5: (5, 1), 16: (8, 2), 64: (8, 8), 65: (13, 5), 200: (25, 8)}
ID_PATTERNS = ("one", "distinct", "ends", "random", "masked")
MAX_ROWS = max(P_VALUES)


@dataclass(frozen=True)
class ExpertCase:
    E: int
    N: int
    K: int
    blocksize: int = 64
    dtype: torch.dtype = torch.bfloat16
    nested: bool = False
    exps: tuple = (-2, 3)

    @property
    def name(self) -> str:
        dt = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[self.dtype]
        return f"{self.E}x{self.N}x{self.K}-{dt}-bs{self.blocksize}-{'nested' if self.nested else 'plain'}"

    @property
    def seed(self) -> int:
        return (self.E * 131 + self.N * 31 + self.K * 7 + self.blocksize + (1 if self.nested else 0)) % (1 << 31)

    @property
    def large(self) -> bool:
        return self.E * self.N * self.K >= 1 << 28


def _medium_cases():
    out = []
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for bs in (32, 64, 128):
            for nested in (False, True):
                # fp16: the scales of plain statistics stay within (-2, 1) so that the sums stay below 65504 (exact_inputs.py)
                out.append(ExpertCase(16, 1024, 1024, bs, dtype, nested, exps=(-2, 1) if dtype == torch.float16 else (-2, 3)))
    return out


EXACT_CASES = tuple(
    [
        ExpertCase(8, 14336, 4096),                 # Mixtral gate / up
        ExpertCase(8, 4096, 14336, nested=True),    # Mixtral down; K = 7 segments of 2048
        ExpertCase(128, 768, 2048, nested=True),    # 128 experts, top-8 style
        ExpertCase(128, 2048, 768, nested=True),
    ]
    + _medium_cases()
    + [
        ExpertCase(5, 130, 768),                    # ragged: a partial row tile, a partial 2048-k segment
        ExpertCase(5, 130, 768, nested=True),
        ExpertCase(4, 96, 96, blocksize=32),        # smallest K: three lanes of a wavefront
        ExpertCase(4, 96, 96, blocksize=32, nested=True),
    ]
)


def build_case(case: ExpertCase) -> X.ExactInputs:
    """The expert stack as the flat [E * N, K] matrix with MAX_ROWS integer activation rows and an integer bias [E * N]; asserts
    the exact-sum bound (exact_inputs.assert_exact_sums, called by build) for every row against every expert."""
    return X.build(case.E * case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=MAX_ROWS, exps=case.exps)


def make_ids(pattern: str, P: int, E: int, gen: torch.Generator) -> torch.Tensor:
    """[P] int64 expert ids (CPU) of one pattern."""
    if pattern == "one":           # all pairs on one expert
        return torch.full((P,), int(torch.randint(0, E, (1,), generator=gen)), dtype=torch.int64)
    if pattern == "distinct":      # all different (cycling once P exceeds E)
        return (torch.randperm(E, generator=gen)[torch.arange(P) % E]).to(torch.int64)
    if pattern == "ends":          # the two end experts only
        return torch.where(torch.rand(P, generator=gen) < 0.5, 0, E - 1).to(torch.int64)
    if pattern == "random":        # random with repeats
        return torch.randint(0, E, (P,), generator=gen)
    if pattern == "masked":        # random with a share of ids that name no expert: -1, E, E + 7
        ids = torch.randint(0, E, (P,), generator=gen)
        bad = torch.tensor([-1, E, E + 7])[torch.randint(0, 3, (P,), generator=gen)]
        return torch.where(torch.rand(P, generator=gen) < 0.3, bad, ids)
    raise ValueError(pattern)
