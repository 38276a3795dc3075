"""Cases and inputs shared by tests/test_ffn_host.py (CPU) and tests/test_gpu_ffn.py (GPU): the dense gated-SiLU FFN - the gated
epilogue of the fused matmul (``bitsandbytes_amd::gemm_4bit_gated``), ``matmul_4bit_gated`` / ``ffn_4bit`` and ``nn.FFN4bit``.

The exact cases use the operands of tests/exact_inputs.py: ``exact_inputs.build(2 F, K, ...)`` IS the interleaved matrix - gate row
``i`` = its row ``2 i``, up row ``i`` = its row ``2 i + 1`` - so every ``g`` and ``u`` is known to the last bit from the float64
product. ``exps=(-8, -5)``: small power-of-two scales put most gate values where SiLU is neither the identity nor zero
(``2^-4 <= |g| <= 8``; the host test asserts >= 50 %).

Shapes ``2F x K`` (blocksize 64 unless noted), the smallest at which each mechanism can go wrong on 256 CUs:
  stream (M = 1; M = 2 ... 4 where the plain call stays on the streaming kernel)
    2816 x 2048          ceil(rows / CUs) = 11, odd: a (gate, up) pair would straddle two workgroups
    64 x 34816, bs 128   fewer rows than CUs (one row per workgroup); 17 segments: more than one phase
    2002 x 6144          F odd; three segments; partial last workgroup
    4096 x 4096          the exact-geometry shape
  streaming MFMA (M = 2 ... 16)
    4352 x 256           R = 17, odd
    4352 x 8192          ring instances (K > 4096), several tiles
    4096 x 4096          single-item instances
    4096 x 2752          K % 256 != 0
    6144 x 256           F and 2F both >= 3072 rows: the member identity
  either / neither
    2002 x 1024          small-matrix route table (5 ... 8 rows: no gated kernel - the composition), partial tile
each in bf16 and fp16, with and without bias, at every M from 1 to 17.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import exact_inputs as X

MS = tuple(range(1, 18))
MAX_ROWS = max(MS)
EXPS = (-8, -5)
LIVE_LO, LIVE_HI = 2.0 ** -4, 8.0
K_STREAM, K_SM = 1, 7
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@dataclass(frozen=True)
class FFNCase:
    N: int                      # weight rows of the interleaved matrix, 2 F
    K: int
    blocksize: int = 64
    dtype: torch.dtype = torch.bfloat16

    @property
    def F(self) -> int:
        return self.N // 2

    @property
    def name(self) -> str:
        return f"{self.N}x{self.K}-bs{self.blocksize}-{str(self.dtype).split('.')[-1]}"

    @property
    def seed(self) -> int:
        return (self.N * 31 + self.K * 7 + self.blocksize + 5) % (1 << 31)


STREAM_SHAPES = ((2816, 2048, 64), (64, 34816, 128), (2002, 6144, 64), (4096, 4096, 64))
SM_SHAPES = ((4352, 256, 64), (4352, 8192, 64), (4096, 4096, 64), (4096, 2752, 64), (6144, 256, 64))
OTHER_SHAPES = ((2002, 1024, 64),)
SHAPES = tuple(dict.fromkeys(STREAM_SHAPES + SM_SHAPES + OTHER_SHAPES))
DTYPES = (torch.bfloat16, torch.float16)
# cases whose exact-sum assertion (tests/exact_inputs.py) fails: none - with scales <= 2^-5 the longest row, 34816 products of
# magnitude <= 4 x 2^-5, stays below 4352 + 8, inside the fp16 range and below 2^24 units of 2^-10 (the host test checks both ways)
EXCLUDED: tuple = ()
CASES = tuple(FFNCase(N, K, bs, dt) for (N, K, bs) in SHAPES for dt in DTYPES if FFNCase(N, K, bs, dt) not in EXCLUDED)
# where bnb_mi355x_gemm_4bit_gated_supported must answer 1 on 256 CUs
MUST_SERVE = tuple((s, (1,)) for s in STREAM_SHAPES) + tuple((s, (2, 4, 8, 16)) for s in SM_SHAPES)


def build_case(case: FFNCase) -> X.ExactInputs:
    """The interleaved [2 F, K] matrix with MAX_ROWS integer activation rows and an integer bias [2 F]."""
    return X.build(case.N, case.K, case.blocksize, case.dtype, False, case.seed, rows=MAX_ROWS, exps=EXPS)


def live_share(ex: X.ExactInputs, with_bias: bool) -> float:
    """Share of the gate values (every activation row against every gate row, rounded to the case's dtype) with
    LIVE_LO <= |g| <= LIVE_HI."""
    g = ex.x.double() @ ex.W[0::2].double().t()
    if with_bias:
        g = g + ex.bias[0::2].double()
    g = g.to(ex.dtype).double().abs()
    return float(((g >= LIVE_LO) & (g <= LIVE_HI)).double().mean())


def interleave_rows(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[F, ...] and [F, ...] -> [2 F, ...]: gate row i at row 2 i, up row i at row 2 i + 1."""
    return torch.stack([gate, up], dim=1).reshape(2 * gate.shape[0], *gate.shape[1:])
