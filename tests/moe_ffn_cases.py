"""Cases and inputs shared by tests/test_moe_ffn_host.py (CPU) and tests/test_gpu_moe_ffn.py (GPU): the gated-SiLU and routing-weight
epilogues of the expert-indexed fused matmul (``bitsandbytes_amd::gemm_4bit_experts_ffn``) and the block ``moe_ffn_4bit``.

The exact cases use the operands of tests/exact_inputs.py: the CHUNKED stack ``[E, 2 I, K]`` is ``exact_inputs.build(E * 2 I, K, ...)``
viewed as ``[E, 2 I, K]`` (gate rows ``[0, I)``, up rows ``[I, 2 I)`` of every expert), so that every gate and up value is known to the
last bit; the interleaved stack is the same matrix with its rows permuted before quantization (:func:`interleave_rows`).

Shapes ``E x 2I x K``, the smallest at which each mechanism can go wrong:
  5 x 144 x 768   bs 64   I = 72: four full 16-column tiles and one of 8; a partial 2048-k segment
  4 x 96 x 96     bs 32   three lanes of a wavefront
  3 x 64 x 18432  bs 128  nine segments, so two phases
  8 x 512 x 1024  bs 64   plain K
each in bf16, fp16 and fp32, with plain and nested statistics - except K = 18432 with nested statistics in fp16, which fails
exact_inputs' own range assertion (test_moe_ffn_host.py checks that it does). Plain-statistics cases use ``exps=(-8, -5)``: small
power-of-two scales put most gate values where SiLU is neither the identity nor zero (``2^-4 <= |g| <= 8``; asserted >= 50 % by the
host test). Nested cases carry no such condition - their gate values are fixed by the nested construction; they cover the row map
and the statistics path.
"""
from __future__ import annotations

import torch

import exact_inputs as X
from experts_cases import ID_PATTERNS, TS_OF_P, ExpertCase, make_ids  # noqa: F401  (re-exported for the two test files)

P_VALUES = (1, 2, 5, 16, 65)   # 65 pairs: more than four pairs on one expert - several passes over one `part` buffer
MAX_ROWS = max(P_VALUES)
PLAIN_EXPS = (-8, -5)
LIVE_LO, LIVE_HI = 2.0 ** -4, 8.0
SHAPES = ((5, 144, 768, 64), (4, 96, 96, 32), (3, 64, 18432, 128), (8, 512, 1024, 64))
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# does not qualify: nested scales reach 8.25, and 18432 products of magnitude <= 4 * 8.25 pass the fp16 range bound
EXCLUDED = (ExpertCase(3, 64, 18432, 128, torch.float16, True),)


def _cases():
    out = []
    for (E, N, K, bs) in SHAPES:
        for dtype in DTYPES:
            for nested in (False, True):
                case = ExpertCase(E, N, K, bs, dtype, nested, exps=(-2, 3) if nested else PLAIN_EXPS)
                if not any((case.E, case.N, case.K, case.dtype, case.nested) == (x.E, x.N, x.K, x.dtype, x.nested) for x in EXCLUDED):
                    out.append(case)
    return tuple(out)


CASES = _cases()   # ExpertCase.N is the number of WEIGHT rows per expert, 2 I


def build_case(case: ExpertCase) -> X.ExactInputs:
    """The chunked stack as the flat [E * 2 I, K] matrix with MAX_ROWS integer activation rows and an integer bias [E * 2 I]."""
    return X.build(case.E * case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=MAX_ROWS, exps=case.exps)


def interleave_rows(flat: torch.Tensor, E: int, N: int) -> torch.Tensor:
    """[E * N, ...] in the chunked layout (gate rows [0, I), up rows [I, 2 I) per expert) -> the interleaved layout (gate row 2 i,
    up row 2 i + 1): a row permutation inside every expert."""
    I = N // 2
    v = flat.view(E, 2, I, *flat.shape[1:])
    return v.transpose(1, 2).reshape(flat.shape)


def live_share(ex: X.ExactInputs, case: ExpertCase, with_bias: bool) -> float:
    """Share of the gate values (every activation row against every expert's gate rows, rounded to the case's dtype) with
    LIVE_LO <= |g| <= LIVE_HI."""
    I = case.N // 2
    W = ex.W.view(case.E, case.N, case.K)[:, :I].reshape(-1, case.K)
    g = ex.x.double() @ W.double().t()
    if with_bias:
        g = g + ex.bias.view(case.E, case.N)[:, :I].reshape(-1).double()
    g = g.to(case.dtype).double().abs()
    return float(((g >= LIVE_LO) & (g <= LIVE_HI)).double().mean())
