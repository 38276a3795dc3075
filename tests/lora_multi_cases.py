"""Cases and inputs shared by tests/test_lora_multi_host.py (CPU) and tests/test_gpu_lora_multi.py (GPU): the mixed-adapter LoRA shrink
``t[m] = x[m] @ lora_A[ids[m]]^T`` (``bitsandbytes_amd::lora_shrink_ids``, csrc/lora_shrink.hip's ids kernel, the public
``bitsandbytes_amd.lora_shrink_ids``) and - second half of the file - the mixed-adapter expand epilogue
(``bitsandbytes_amd::gemm_4bit_lora_ids``, ``matmul_4bit_lora_ids``, ``nn.Linear4bitMultiLoRA``).

Exact inputs, per adapter: ``x`` is ``exact_inputs.int_rows`` (integers with |x| <= 4, every row distinct); adapter ``a`` of a stack is
drawn from ``lora_cases.B_VALUES`` (0, +-2^-6 ... +-2^-3) with a generator seeded by the case AND by ``a``, so the adapters differ. The
bound is that of tests/lora_shrink_cases.py - every partial sum is exact in fp32 in any order for K < 524288 - and the reference,
float64 rounded once with each row's own adapter, is the only right answer.

Shapes, the smallest at which each mechanism can go wrong (grid = (R / 8, A_n); sixteen wavefronts per workgroup, wavefront w takes
the 32-k steps w, w + 16, ... in batches of eight):
  K = 64      two steps: fewer steps than wavefronts
  K = 2048    four steps per wavefront: one partly filled batch
  K = 4096    eight steps per wavefront: exactly one batch; K = 8192 (ordinary data only): more than one batch
  R = 8 (one tile per adapter), 24, 128; splits (16, 16, 16) and (8, 128, 24)
  A_n = 1 (adapter 0 is every adapter), 3, 17 (more adapters than rows), 64 (the cap)
  M = 1, 2, 3, 4, 8, 16
Id patterns per M (``patterns``): all rows the same id; all distinct (as many distinct ids as A_n allows); two adapters interleaved;
the first and the last adapter; -1 and A_n among valid ids; no row with an adapter; int64 ids with 2^32 + 1 and 2^32 (the aliases of
adapters 1 and 0 if only the low word were compared). Out-of-range ids are the adjacent values and the alias only.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import exact_inputs as X
import lora_cases as LC
import lora_shrink_cases as SC

MS = (1, 2, 3, 4, 8, 16)
MAX_ROWS = 16
DTYPES = SC.DTYPES
DT_CODE = SC.DT_CODE
A_VALUES = SC.A_VALUES
UNIT = SC.UNIT
MAX_ADAPTERS = 64


@dataclass(frozen=True)
class MultiShrinkCase:
    K: int
    A_n: int
    R: int
    dtype: torch.dtype
    splits: Optional[Tuple[int, ...]] = None

    @property
    def name(self) -> str:
        s = "" if self.splits is None else "-s" + "_".join(map(str, self.splits))
        return f"K{self.K}-A{self.A_n}-R{self.R}-{str(self.dtype).split('.')[-1]}{s}"

    @property
    def seed(self) -> int:
        return (self.K * 13 + self.R * 7 + self.A_n * 1009 + (1 if self.dtype == torch.float16 else 0)) % (1 << 31)


BF, FP = torch.bfloat16, torch.float16
# every K meets three adapter counts, the three ranks and both dtypes; 64 adapters at two K; each split table once
CASES = (
    MultiShrinkCase(64, 17, 8, BF), MultiShrinkCase(64, 64, 24, FP), MultiShrinkCase(64, 1, 128, BF),
    MultiShrinkCase(2048, 3, 128, FP), MultiShrinkCase(2048, 17, 24, BF), MultiShrinkCase(2048, 1, 8, FP),
    MultiShrinkCase(4096, 64, 8, BF), MultiShrinkCase(4096, 17, 128, FP), MultiShrinkCase(4096, 3, 24, BF),
    MultiShrinkCase(2048, 3, 48, BF, (16, 16, 16)), MultiShrinkCase(4096, 17, 160, FP, (8, 128, 24)),
)
ADAPTER_COUNTS = (1, 3, 17, 64)

# outside each precondition of bnb_mi355x_lora_shrink_ids_supported: (dtype code, M, A_n, R, K)
MUST_REFUSE = ((2, 1, 0, 16, 4096), (2, 1, 65, 16, 4096), (2, 1, -1, 16, 4096), (2, 0, 3, 16, 4096), (2, 17, 3, 16, 4096), (2, 1, 3, 12, 4096),
               (2, 1, 3, 1032, 4096), (2, 1, 3, 16, 96), (0, 1, 3, 16, 4096), (3, 1, 3, 16, 4096))


def patterns(M: int, A_n: int):
    """[(name, ids as a list of python ints, torch dtype)] for a batch of M rows against A_n adapters."""
    last = A_n - 1
    mid, mid2 = A_n // 2, min(A_n // 2 + 1, last)
    cyc = lambda vals: [vals[i % len(vals)] for i in range(M)]
    distinct = [last - i for i in range(M)] if A_n >= M else [i % A_n for i in range(M)]
    return [
        ("same", [min(1, last)] * M, torch.int32),
        ("distinct", distinct, torch.int32),
        ("distinct64", distinct[::-1], torch.int64),
        ("two", cyc([mid, mid2]), torch.int32),
        ("first_last", cyc([last, 0]), torch.int32),
        ("out_of_range", cyc([-1, mid, A_n, 0]), torch.int32),
        ("none", cyc([A_n, -1]), torch.int32),
        ("alias64", cyc([2 ** 32 + 1, min(1, last), 2 ** 32, 0, -1]), torch.int64),
    ]


def in_range(ids, A_n: int):
    return [0 <= i < A_n for i in ids]


@functools.lru_cache(maxsize=None)
def build(case: MultiShrinkCase):
    """(x [MAX_ROWS, K], A [A_n, R, K]) in the case's dtype: exact inputs; every row of x distinct, every row of every adapter distinct
    from every other row of the stack."""
    gen = torch.Generator().manual_seed(case.seed)
    x = X.int_rows(MAX_ROWS, case.K, case.dtype, gen)
    values = torch.tensor(A_VALUES, dtype=torch.float32)
    mats = []
    for a in range(case.A_n):
        ga = torch.Generator().manual_seed(case.seed * 131 + a)
        mats.append(LC._distinct_rows(lambda n: values[torch.randint(0, len(A_VALUES), (n, case.K), generator=ga)], case.R))
    stack = torch.stack(mats)
    if case.K > 64:
        assert torch.unique(stack.view(-1, case.K), dim=0).shape[0] == case.A_n * case.R
    return x, stack.to(case.dtype)


def reference(x: torch.Tensor, stack: torch.Tensor, ids) -> torch.Tensor:
    """float64 with each row's own adapter, rounded once to the operands' dtype; zeros for a row without an adapter: [rows, R]."""
    A_n, R, _ = stack.shape
    out = torch.zeros(x.shape[0], R, dtype=torch.float64)
    for m, i in enumerate(ids):
        if 0 <= i < A_n:
            out[m] = x[m].double() @ stack[i].double().t()
    return out.to(x.dtype)


def ordinary(M: int, A_n: int, R: int, K: int, dtype: torch.dtype, seed: int):
    """x ~ N(0, 1) [M, K], A ~ N(0, 1 / K) [A_n, R, K]: sums that round."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=gen).to(dtype)
    a = (torch.randn(A_n, R, K, generator=gen) / K ** 0.5).to(dtype)
    return x, a


# ------------------------------------------------------------------------------------------ expand (gemm_4bit_lora_ids)
# The mixed-adapter epilogue of the two decode kernels. Base operands: lora_cases.build_case (exact weights, statistics, integer
# activations and bias). Adapter operands: lora_cases.build_adapter's value sets - t integers in [-4, 4] (one row per batch row, shared
# by the adapters), B_l from B_VALUES seeded per adapter index so that the adapters differ, scalings 0.5 / 2 alternating over the stack:
# every adapter product is a multiple of lora_cases.ADAPTER_UNIT, and T(x64 W64^T + bias64 + s_id t64 B_id64^T) per row is the only
# right answer in any order. Shapes (reasons in lora_cases.py's docstring): streaming 2816 x 2048 and 64 x 34816 bs 128; streaming MFMA
# 4352 x 256, 4096 x 4096, 4352 x 8192, 4096 x 2752; neither family 2002 x 1024 at 5 ... 8 rows. Ranks 8 / 24 / 128, A_n 1 / 3 / 17,
# nested statistics on lora_cases.NESTED_SHAPES, both dtypes - rotated over the shapes.
EXPAND_MS = MS
OTHER_MS = (1, 5, 8)          # 2002 x 1024: the streaming kernel at one row, the register-transposed kernel (no epilogue) at 5 ... 8


@dataclass(frozen=True)
class MultiExpandCase:
    base: LC.LoRACase
    r: int
    A_n: int

    @property
    def name(self) -> str:
        return f"{self.base.name}-r{self.r}-A{self.A_n}"


def _ec(N, K, bs, dtype, nested, r, A_n):
    return MultiExpandCase(LC.LoRACase(N, K, bs, dtype, nested), r, A_n)


EXPAND_CASES = (
    _ec(2816, 2048, 64, BF, False, 8, 3), _ec(2816, 2048, 64, FP, True, 128, 17),
    _ec(64, 34816, 128, BF, False, 24, 17), _ec(64, 34816, 128, FP, False, 8, 1),
    _ec(4352, 256, 64, BF, True, 24, 3), _ec(4352, 256, 64, FP, False, 128, 17),
    _ec(4096, 4096, 64, BF, False, 128, 17), _ec(4096, 4096, 64, FP, True, 8, 3),
    _ec(4352, 8192, 64, BF, False, 8, 1), _ec(4352, 8192, 64, FP, False, 24, 17),
    _ec(4096, 2752, 64, BF, True, 128, 3), _ec(4096, 2752, 64, FP, False, 24, 17),
    _ec(2002, 1024, 64, BF, False, 8, 3),
)
EXPAND_STREAM = ((2816, 2048, 64), (64, 34816, 128))
EXPAND_SM = LC.SM_SHAPES
EXPAND_OTHER = LC.OTHER_SHAPES
# where bnb_mi355x_gemm_4bit_lora_ids_supported must answer 1 on 256 CUs: lora_cases.MUST_SERVE, every rank, both statistics, every A_n
EXPAND_MUST_SERVE = LC.MUST_SERVE


def expand_ms(case: MultiExpandCase):
    return OTHER_MS if (case.base.N, case.base.K, case.base.blocksize) in EXPAND_OTHER else EXPAND_MS


@functools.lru_cache(maxsize=None)
def build_expand_adapters(case: MultiExpandCase):
    """(t [MAX_ROWS, r], B [A_n, N, r] in the case's dtype, scalings [A_n] float32): exact operands, every adapter different."""
    b = case.base
    gen = torch.Generator().manual_seed(b.seed * 131 + case.r)
    values = torch.tensor(LC.B_VALUES, dtype=torch.float32)
    t = LC._distinct_rows(lambda n: torch.randint(-LC.T_MAX, LC.T_MAX + 1, (n, case.r), generator=gen).float(), MAX_ROWS)
    mats = []
    for a in range(case.A_n):
        ga = torch.Generator().manual_seed(b.seed * 977 + case.r * 31 + a)
        mats.append(values[torch.randint(0, len(LC.B_VALUES), (b.N, case.r), generator=ga)])
    stack = torch.stack(mats)
    assert case.A_n == 1 or not torch.equal(stack[0], stack[1])
    scalings = torch.tensor([LC.SCALINGS[a % 2] for a in range(case.A_n)], dtype=torch.float32)
    return t.to(b.dtype), stack.to(b.dtype), scalings


def expand_reference(y64: torch.Tensor, bias64, t: torch.Tensor, stack: torch.Tensor, scalings: torch.Tensor, ids, dtype) -> torch.Tensor:
    """T(y64 + bias64 + s_id t64 B_id64^T) per row; T(y64 + bias64) for a row without an adapter. y64: [rows, N] float64."""
    A_n = stack.shape[0]
    out = y64.clone() if bias64 is None else y64 + bias64
    for m, i in enumerate(ids):
        if 0 <= i < A_n:
            out[m] = out[m] + float(scalings[i]) * (t[m].double() @ stack[i].double().t())
    return out.to(dtype)


def ordinary_expand(M: int, A_n: int, N: int, r: int, dtype: torch.dtype, seed: int):
    """t ~ N(0, 1) [M, r], B ~ N(0, 0.25) [A_n, N, r], scalings in [0.25, 2.25): sums that round."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(M, r, generator=gen).to(dtype)
    b = (torch.randn(A_n, N, r, generator=gen) * 0.5).to(dtype)
    s = (torch.rand(A_n, generator=gen) * 2 + 0.25).float()
    return t, b, s
