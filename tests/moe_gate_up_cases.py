"""Cases of tests/test_moe_gate_up_host.py and tests/test_gpu_moe_gate_up.py: the token-major gate / up launch
(csrc/gemm4_experts_gate_up.hip). The chunked stack ``[E, 2 I, K]`` is ``exact_inputs.build(E * 2 I, K)`` as in tests/moe_ffn_cases.py
(whose ``build_case``, ``interleave_rows`` and ``live_share`` serve here unchanged), ``x[t]`` is activation row ``t``. Shapes
``E x 2I x K`` and the lane map the kernel derives from K (chunks of 32 k; L lanes per row, Q rounds, segments):
  4 x 96 x 96     bs 32   3 chunks under L = 8: a row shorter than any lane group
  5 x 72 x 768    bs 64   L = 8, Q = 3: eight weight rows per wavefront-wide load
  3 x 86 x 1024   bs 64   L = 16, Q = 2; I = 43: a ragged tile and a ragged row group
  6 x 40 x 2560   bs 64   L = 32, Q = 3, 80 of 96 chunk slots live
  3 x 64 x 18432  bs 128  L = 64, five segments: a wavefront's run of units crosses segments
(T, S), the id patterns and the CU counts are those of tests/moe_combine_cases.py.
"""
import torch

from experts_cases import ExpertCase
from moe_combine_cases import CU_COUNTS, ID_PATTERNS, TS, make_ids  # noqa: F401  (re-exported for the two test files)
from moe_ffn_cases import EXCLUDED, PLAIN_EXPS, build_case, interleave_rows, live_share  # noqa: F401

SHAPES = ((4, 96, 96, 32), (5, 72, 768, 64), (3, 86, 1024, 64), (6, 40, 2560, 64), (3, 64, 18432, 128))
CASES = tuple(
    c for c in (ExpertCase(E, N, K, bs, dt, nested, exps=(-2, 3) if nested else PLAIN_EXPS)
                for (E, N, K, bs) in SHAPES for dt in (torch.bfloat16, torch.float16, torch.float32) for nested in (False, True))
    if not any((c.E, c.N, c.K, c.dtype, c.nested) == (x.E, x.N, x.K, x.dtype, x.nested) for x in EXCLUDED))
