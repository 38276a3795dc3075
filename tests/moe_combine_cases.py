"""Cases of tests/test_moe_combine_host.py and tests/test_gpu_moe_combine.py. The stack ``[E, N, K]`` is ``exact_inputs.build(E * N, K)``,
``h[t, s]`` activation row ``t * S + s``, routing weights from {0.5, 1, 2}: every ``w * (acc + bias)`` is a multiple of ``ex.unit * 0.5``
and, under :func:`premise`, every fp32 partial sum is exact in any order - the float64 reference rounded once is the only right answer.
Shapes ``E x N x K`` and the lane map the kernel derives from K (chunks of 32 k; L lanes per row, Q rounds, segments):
  4 x 96 x 96     bs 32   3 chunks under L = 8: a row shorter than any lane group
  5 x 72 x 768    bs 64   L = 8, Q = 3: eight rows per wavefront-wide load, several workgroups per token
  3 x 43 x 1024   bs 64   L = 16, Q = 2; 43 rows: a partial tile and a partial row group
  6 x 40 x 2560   bs 64   L = 32, Q = 3, 80 of 96 chunk slots live
  3 x 64 x 18432  bs 128  L = 64, five segments: ten units at S = 2, more than wavefronts; S = 2 only
Every case also runs planned for ONE compute unit (``CU_COUNTS``): tiles of 20 ... 64 rows, so several row groups per wavefront, row groups
shared by 8 / 4 / 2 wavefronts (S = 1 / 2 / 3 with one segment) or owned by one (S = 8), and at 43 rows a ragged last group.
"""
import torch

import exact_inputs as X
from experts_cases import ExpertCase
from moe_ffn_cases import EXCLUDED, PLAIN_EXPS

SHAPES = ((4, 96, 96, 32), (5, 72, 768, 64), (3, 43, 1024, 64), (6, 40, 2560, 64), (3, 64, 18432, 128))
TS = ((1, 1), (1, 8), (3, 2), (2, 16), (5, 3))
CU_COUNTS = (0, 1)      # bnb_mi355x_set_cu_count: the device's own count, and one CU
LONG_K = 18432          # S = 2 there
MAX_ROWS = max(t * s for t, s in TS)
ID_PATTERNS = ("distinct", "same", "one_out", "token_out")
CASES = tuple(
    c for c in (ExpertCase(E, N, K, bs, dt, nested, exps=(-2, 3) if nested else PLAIN_EXPS)
                for (E, N, K, bs) in SHAPES for dt in (torch.bfloat16, torch.float16, torch.float32) for nested in (False, True))
    if not any((c.E, c.N, c.K, c.dtype, c.nested) == (x.E, x.N, x.K, x.dtype, x.nested) for x in EXCLUDED))


def build_case(case: ExpertCase) -> X.ExactInputs:
    ex = X.build(case.E * case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=MAX_ROWS, exps=case.exps)
    if case.nested and case.K == LONG_K:
        # nested scales have no exponent window to narrow (they reach 8.25): activations from {-1, 0, 1} keep S = 2 under the bound
        ex.x = ex.x.sign()
        assert torch.unique(ex.x, dim=0).shape[0] == MAX_ROWS
    return ex


def weights(T: int, S: int) -> torch.Tensor:
    """[T, S] fp32 from {2, 1, 0.5}: (2, 1, 0.5, 0.5, ...) rotated by the token index."""
    base = torch.tensor(([2.0, 1.0] + [0.5] * S)[:S])
    return torch.stack([base.roll(t) for t in range(T)])


def premise(ex: X.ExactInputs, S: int) -> bool:
    """sum_s |w_s| * (sum_k |h W| + |bias|) < 2^24 units of ``ex.unit * 0.5`` for the worst (activation row, weight row) of the case
    with the S largest weights (and inside fp16's range)."""
    worst = float((ex.x.double().abs() @ ex.W.double().abs().t()).max()) + float(ex.bias.abs().max())
    worst *= float(weights(1, S).sum())
    return worst < 2.0 ** 24 * ex.unit * 0.5 and (ex.dtype != torch.float16 or worst < X.FP16_MAX)


def ts_of(case: ExpertCase, ex: X.ExactInputs):
    """The (T, S) of the sweep that the exactness bound allows for this case."""
    return tuple((T, S) for T, S in TS if (S <= 2 or case.K != LONG_K) and premise(ex, S))


def make_ids(pattern: str, T: int, S: int, E: int) -> torch.Tensor:
    """[T, S] int64 ids (CPU). one_out: slot t % S of token t is -1 or E; token_out: every slot of token 0 is out of range."""
    t, s = torch.arange(T)[:, None], torch.arange(S)[None, :]
    if pattern == "same":
        return ((t * 3 + 1) % E).expand(T, S).clone()
    ids = (t * 5 + s) % E          # distinct within a token while S <= E, cycling beyond
    if pattern == "one_out":
        ids = torch.where(s == t % S, torch.where(t % 2 == 0, -1, E), ids)
    elif pattern == "token_out":
        ids[0] = torch.where(torch.arange(S) % 2 == 0, -1, E + 7)
    return ids
