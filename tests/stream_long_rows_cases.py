"""Cases and exact operands for the streaming gemv (csrc/gemv4_stream.hip) at its longest rows: K up to 511 * 2048 = 1 046 528, up to
256 phases of the ``kMulti`` loop, 8 KiB of partial sums per weight row and the clamp of the rows per workgroup to 1 or 2.
Shared by tests/test_stream_long_rows_host.py (CPU) and tests/test_gpu_stream_long_rows.py (GPU).

The construction is that of tests/large_offset_cases.py - FP4 nibbles written in place (``build_packed``), a power-of-two scale per
block seeded from the block index (``plain_scale``), a chunked float64 reference of the CONSTRUCTED operands (``rows64``) - with the
value ranges narrowed so that a row of 2^20 products still sums exactly in fp32 in any order (exact_inputs.assert_exact_sums' rule):

* activations from {-1, 0, 1};
* plain statistics: the four exponents ``EXPS = (-7, -4)``, drawn per block from a hash of the block index with the column-parity rule
  (neighbouring blocks of a row never share a scale; no two rows share a pattern). Every product is a multiple of 2^-7 * 0.25 = 2^-9 =
  UNIT_PLAIN, which divides lora_cases' adapter unit 2^-7. The value ranges alone do not give the bound at this K (1 046 528 products of
  magnitude <= 2^-4 could reach 65 408, twice 2^24 units = 32 768), so it is asserted on the weights actually drawn, for every weight
  row: mean |code| is 0.5 and the mean scale 3.75 * 2^-7, about 7.5 units per product - 7.9 * 10^6 units, 15 300 in value, inside fp16 -
  with the bias (<= 8) and the largest adapter term (128) on top;
* nested statistics: ``absmax_code[i] = NESTED_TABLE[i % 4]`` = (0.25, 0.5, 0.75, 1.0), absmax2 alternating 1.0 / 2.0 over the groups of
  256 blocks (neighbours differ), offset 0.25: scales 0.5 ... 2.25, each step of ``code2[q] * absmax2 + offset`` exact in fp32 and
  ``code4 * scale`` exact in bf16. Unit 0.25 * 0.25 = 2^-4; about 9.6 units per product, 10^7 units at the longest row: below 2^24. In
  value that is 6 * 10^5: outside fp16, so the fp16 x nested cases are EXCLUDED (tests/exact_inputs.py's own table and its six-value
  scale range would not fit under 2^24 units at this K at all).

The geometry each case is there for is written down in ``Call.geometry`` and asserted against bnb_mi355x_stream_geometry by both
test modules: a routing or geometry change that moves a case out of its regime fails loudly.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

import exact_inputs as X
import large_offset_cases as L
import lora_cases as LC

EXPS = (-7, -4)
X_LIMIT = 1
UNIT_PLAIN = 2.0 ** EXPS[0] * 0.25
NESTED_TABLE = (0.25, 0.5, 0.75, 1.0)
NESTED_ABSMAX2 = (1.0, 2.0)
NESTED_OFFSET = 0.25
UNIT_NESTED = min(NESTED_TABLE) * min(NESTED_ABSMAX2) * 0.25
REF_ROWS = 8            # activation rows built per case (the largest M is 7)
LORA_R = 8
MAX_K = 511 * 2048
DT_CODE = L.DT_CODE
BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
FORMS = ("plain", "grouped", "gated", "lora", "lora_ids")   # bnb_mi355x_stream_geometry's `form`
K_STREAM, K_SM = 1, 7


@dataclass(frozen=True)
class LongCase:
    name: str
    N: int
    K: int
    blocksize: int

    @property
    def elements(self) -> int:
        return self.N * self.K

    @property
    def seed(self) -> int:
        return (self.N * 31 + self.K * 7 + self.blocksize + 3) % (1 << 31)


MAXK = LongCase("maxk", 8, MAX_K, 64)                 # S = 511: the longest row the kernel takes
RAGGED = LongCase("ragged", 8, MAX_K - 2048 + 32, 32)  # the last of 511 segments holds 32 columns
EDGES = tuple(LongCase(f"edge{K}", 5, K, 32) for K in (32768, 32800, 20480, 20512, 10240, 10272))
RCAP1 = LongCase("rcap1", 258, MAX_K, 64)             # 270 M elements: room for the partial sums of ONE row at four activation rows
RCAP2 = LongCase("rcap2", 514, 349 * 2048, 64)        # 367 M elements: S = 349, room for two rows
# rcap2's row length at 8 rows: the fused forms at four activation rows stay on the streaming kernel here (fewer than 128 rows: no
# streaming MFMA kernel; below 12 Mi weights: no other MFMA kernel), with the same S = 349, SW = 5, P = 70, r_cap = 2 and LDS request
S349 = LongCase("s349", 8, 349 * 2048, 64)
ROWS3 = (0, 0, 3, -1, 0)   # bnb_mi355x_set_stream_tuning: three rows per workgroup asked for - rcap2's row split, at any row count
SMALL = (MAXK, RAGGED, S349) + EDGES
LARGE = (RCAP1, RCAP2)
CASES = SMALL + LARGE
CASE = {c.name: c for c in CASES}


@dataclass(frozen=True)
class Call:
    """One launch: ``form`` of the streaming kernel on ``case`` at M rows. ``public``: the built-in route of the public op picks the
    streaming kernel (else the plain call goes through ``hip._gemm_4bit_fused(..., kernel=3)``). ``geometry``: (mb, waves, SW, P, R,
    grid_x) on 256 CUs - the regime the call is there for. ``tuning``: the stream tuning the call is made under (None: the defaults)."""
    case: LongCase
    form: str
    dtype: torch.dtype
    nested: bool
    M: int
    geometry: tuple
    public: bool = True
    tuning: Optional[tuple] = None

    @property
    def name(self) -> str:
        kind = str(self.dtype).split(".")[-1] + ("-nested" if self.nested else "")
        return f"{self.case.name}-{self.form}-{kind}-M{self.M}" + ("" if self.tuning is None else f"-rows{self.tuning[2]}")


def _maxk_16bit(M):
    # S = 511. One row: 16 columns of 16 wavefronts, 32 phases. Two rows: 8 wavefronts (rows_waves: not one phase), 64 phases. Three and
    # four rows (and passes of four over grid.y at M = 7): 80 KiB of image hold 5 columns of 4 rows, 103 phases, the last of ONE segment.
    return {1: (1, 16, 16, 32, 1, 8), 2: (2, 8, 8, 64, 1, 8)}.get(M, (4, 8, 5, 103, 1, 8))


_MAXK_FP32 = {1: (1, 16, 10, 52, 1, 8), 2: (2, 8, 5, 103, 1, 8), 4: (4, 8, 2, 256, 1, 8)}   # P = 256: bit 31 of the packed word

PLAIN_CALLS = tuple(
    [Call(MAXK, "plain", dt, nested, M, _maxk_16bit(M), public=M <= 4)
     for dt, nested in ((BF, False), (FP, False), (BF, True), (FP, True)) for M in (1, 2, 3, 4, 7)]
    + [Call(MAXK, "plain", F32, False, M, _MAXK_FP32[M]) for M in (1, 2, 4)]
    + [Call(RAGGED, "plain", BF, False, 1, (1, 16, 16, 32, 1, 8)), Call(RAGGED, "plain", BF, False, 4, (4, 8, 5, 103, 1, 8)),
       Call(RAGGED, "plain", F32, False, 4, (4, 8, 2, 256, 1, 8))]
    # either side of the one-phase limit of 16 wavefronts (the second phase is one 32-column segment)
    + [Call(CASE["edge32768"], "plain", BF, False, 1, (1, 16, 16, 1, 1, 5)), Call(CASE["edge32800"], "plain", BF, False, 1, (1, 16, 16, 2, 1, 5))]
    # either side of the point where rows_waves drops two rows from 16 to 8 wavefronts
    + [Call(CASE["edge20480"], "plain", BF, False, 2, (2, 16, 10, 1, 1, 5)), Call(CASE["edge20512"], "plain", BF, False, 2, (2, 8, 8, 2, 1, 5))]
    # either side of the one-phase limit of the 4-row instance
    + [Call(CASE["edge10240"], "plain", BF, False, 4, (4, 8, 5, 1, 1, 5)), Call(CASE["edge10272"], "plain", BF, False, 4, (4, 8, 5, 2, 1, 5))]
    # r_cap = 1: R goes from ceil(258 / 256) = 2 to 1, 258 workgroups; one row: unclamped
    + [Call(RCAP1, "plain", BF, False, 4, (4, 8, 5, 103, 1, 258), public=False), Call(RCAP1, "plain", BF, False, 1, (1, 16, 16, 32, 2, 129))]
    # r_cap = 2: R goes from 3 to 2
    + [Call(RCAP2, "plain", BF, False, 4, (4, 8, 5, 70, 2, 257), public=False)]
    # the same clamp, 3 -> 2, on 8 rows under the rows-per-workgroup knob (the plain twin of the fused calls below)
    + [Call(S349, "plain", BF, False, 4, (4, 8, 5, 70, 2, 4), tuning=ROWS3)]
)
FUSED_CALLS = (
    Call(MAXK, "gated", BF, False, 1, (1, 16, 16, 32, 2, 4)), Call(MAXK, "gated", BF, False, 2, (2, 8, 8, 64, 2, 4)),
    Call(MAXK, "lora", BF, False, 1, _maxk_16bit(1)), Call(MAXK, "lora", BF, False, 4, _maxk_16bit(4)),
    Call(MAXK, "lora_ids", BF, False, 1, _maxk_16bit(1)), Call(MAXK, "lora_ids", BF, False, 4, _maxk_16bit(4)),
    # S = 349 at four activation rows, r_cap = 2, on the streaming kernel through the public ops. Gated at the defaults: the row split
    # gives R = 1, the pairs need 2 = r_cap - the last even R that fits. Under ROWS3 the split asks for 3 and the partial-sum slots clamp
    # it to 2, which stays even for the pairs: rcap2's regime (what the kernel is handed differs from rcap2's launch in grid_x alone).
    Call(S349, "gated", BF, False, 4, (4, 8, 5, 70, 2, 4)), Call(S349, "gated", BF, False, 4, (4, 8, 5, 70, 2, 4), tuning=ROWS3),
    Call(S349, "lora", BF, False, 4, (4, 8, 5, 70, 2, 4), tuning=ROWS3), Call(S349, "lora_ids", BF, False, 4, (4, 8, 5, 70, 2, 4), tuning=ROWS3),
)
# An extra, beside the s349 calls above: the fused forms on rcap2 ITSELF at four rows. The library's router sends fused calls of
# 514 x 714752 at M = 4 to the streaming MFMA kernel (csrc/c_api.hip: gated_family / lora_family follow the plain call's built-in route,
# and kernel = 3 cannot be asked of them). The geometry the streaming kernel would launch is asserted on the host; the GPU module holds
# whichever of the two families runs to the same reference.
RCAP2_FUSED = (Call(RCAP2, "gated", BF, False, 4, (4, 8, 5, 70, 2, 257), public=False), Call(RCAP2, "lora", BF, False, 4, (4, 8, 5, 70, 2, 257), public=False))
# a case whose exact-sum assertion cannot hold: the nested scales put the longest row at 6 * 10^5, outside fp16
EXCLUDED = tuple(c for c in PLAIN_CALLS if c.dtype == FP and c.nested)
CALLS = tuple(c for c in PLAIN_CALLS if c not in EXCLUDED)
# matmul_4bit_gated at three rows on maxk: no (gate, up) pair fits a workgroup beside the image - the query refuses, the composition runs
UNSUPPORTED_GATED = (MAXK, BF, 3)
LORA_IDS = {1: (1,), 4: (1, 0, 2, 1)}      # two adapters; id 2 is out of range: the plain row
LORA_SCALINGS = (0.5, 2.0)


# ------------------------------------------------------------------------------------------ statistics
def nested_stats(N: int, K: int, blocksize: int, device) -> L.Nested:
    """large_offset_cases.nested_stats with this module's narrow table: the entry of a block from the hash of its index (parity follows
    the block column: neighbours differ), absmax2 alternating over the groups."""
    span = len(NESTED_TABLE)
    bpr = K // blocksize
    blocks = N * bpr
    groups = -(blocks // -256)
    code2 = torch.tensor([NESTED_TABLE[i % span] for i in range(256)], dtype=torch.float32, device=device)
    absmax2 = torch.tensor(NESTED_ABSMAX2, dtype=torch.float32, device=device)[torch.arange(groups, device=device) & 1]
    offset = torch.tensor(NESTED_OFFSET, dtype=torch.float32, device=device)
    b = torch.arange(blocks, dtype=torch.int64, device=device)
    h = L.mix(b)
    sel = (2 * (h % (span // 2)) + ((b % bpr) & 1)) % span
    q = sel + span * ((h >> 8) % (256 // span))
    scale = code2[q] * absmax2[b >> 8] + offset
    return L.Nested(q.to(torch.uint8), code2, absmax2, offset, scale)


def unit_of(nested: bool) -> float:
    return UNIT_NESTED if nested else UNIT_PLAIN


# ------------------------------------------------------------------------------------------ one case, built
@dataclass
class Built:
    case: LongCase
    dtype: torch.dtype
    nested: bool
    packed: torch.Tensor
    scale: torch.Tensor
    unit: float
    x: torch.Tensor                  # [REF_ROWS, K] from {-1, 0, 1}
    bias: torch.Tensor               # [N] integers
    y64: Optional[torch.Tensor] = None   # [REF_ROWS, N] float64 x @ W.T, exact
    worst: float = 0.0
    nest: Optional[L.Nested] = None

    def stats_args(self):
        if not self.nested:
            return self.scale, None, None, None
        return self.nest.absmax2, self.nest.absmax_8bit, self.nest.absmax_code, self.nest.offset

    def ref(self, with_bias: bool, M: int) -> torch.Tensor:
        """float64 ``x @ W.T (+ bias)`` rounded once to the output dtype."""
        y = self.y64[:M]
        return (y + self.bias.double() if with_bias else y).to(self.dtype)


def worst_sum(packed, scale, N: int, K: int, blocksize: int, xmax: torch.Tensor, unit: float, chunk: int) -> float:
    """max over the weight rows of sum_k xmax[k] * |W[n, k]| - exact_inputs.assert_exact_sums' bound -, asserting on the way that every
    weight is a multiple of the unit (a nibble outside the construction decodes to NaN and fails here)."""
    worst = 0.0
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        w = L.rows64(packed, scale, K, blocksize, r0, r1)
        assert not bool((w / unit).frac().any()), "a weight is not a multiple of the unit (or a nibble outside the construction)"
        worst = max(worst, float((w.abs() @ xmax).max()))
    return worst


def worst_sum_upper(packed, scale, N: int, K: int, blocksize: int) -> float:
    """max over the weight rows of sum_k |W[n, k]| - ``worst_sum`` with every |x| taken as 1, an upper bound of it - in byte arithmetic
    (no float64 copy of the weights: the CPU test of the two large cases). |code| * 4 of a nibble n of the construction, with
    m = n & 7 in {0, 3, 5, 7}: 0 for m = 0, else 1 << ((7 - m) >> 1) = 4, 2, 1."""
    bpr = K // blocksize
    worst = 0.0
    rows = max(1, (1 << 26) // K)
    for r0 in range(0, N, rows):
        r1 = min(N, r0 + rows)
        b = packed[r0 * K // 2:r1 * K // 2]
        total = torch.zeros((r1 - r0) * bpr, dtype=torch.int32, device=packed.device)
        for m in ((b >> 4) & 7, b & 7):
            quarter = torch.where(m > 0, torch.bitwise_left_shift(torch.ones_like(m), (7 - m) >> 1), m)
            total += quarter.view(-1, blocksize // 2).sum(dim=1, dtype=torch.int32)
        per_row = (total.double() * 0.25 * scale[r0 * bpr:r1 * bpr].double()).view(r1 - r0, bpr).sum(dim=1)
        worst = max(worst, float(per_row.max()))
    return worst


def assert_exact(worst: float, unit: float, dtype: torch.dtype, extra: float) -> None:
    total = worst + extra
    assert total < 2.0 ** 24 * unit, f"sum of |products| {total} reaches 2^24 units ({2.0 ** 24 * unit}): fp32 partial sums may round"
    if dtype == torch.float16:
        assert total < X.FP16_MAX, f"sum of |products| {total} reaches the fp16 range"


def build(case: LongCase, device, dtype=BF, nested: bool = False, packed: Optional[torch.Tensor] = None, with_reference: bool = True,
          upper_bound: bool = False) -> Built:
    """Weights (or the ``packed`` bytes of an earlier build of the case), statistics, activations, bias and - ``with_reference`` - the
    float64 product of one case on ``device``, with the exact-sum bound asserted over every weight row: bias and the largest adapter
    term (lora_cases.ADAPTER_MAX, plain statistics) included. ``upper_bound``: the bound from ``worst_sum_upper`` (every |x| = 1)."""
    N, K, bs = case.N, case.K, case.blocksize
    if packed is None:
        packed = L.build_packed(N, K, bs, device, case.seed)
    assert packed.numel() == N * K // 2
    nest = None
    if nested:
        nest = nested_stats(N, K, bs, device)
        scale = nest.scale
        assert bool((nest.absmax2[1:] != nest.absmax2[:-1]).all()), "neighbouring groups of 256 blocks share an absmax2"
        sel = (nest.absmax_8bit.view(N, K // bs) % len(NESTED_TABLE))
        assert bool((sel[:, 1:] != sel[:, :-1]).all()), "neighbouring blocks share a table entry"
    else:
        scale = L.plain_scale(N, K, bs, EXPS, device)
        s2 = scale.view(N, K // bs)
        assert bool((s2[:, 1:] != s2[:, :-1]).all()), "neighbouring blocks share a scale"
    unit = unit_of(nested)
    x = L.int_rows(REF_ROWS, K, dtype, case.seed + 1, device, limit=X_LIMIT)
    gen = torch.Generator().manual_seed(case.seed + 2)
    bias = torch.randint(-X.BIAS_MAX, X.BIAS_MAX + 1, (N,), generator=gen).to(dtype).to(device)
    out = Built(case, dtype, nested, packed, scale, unit, x, bias, nest=nest)
    chunk = max(1, (1 << 24) // K)
    xmax = x.double().abs().amax(dim=0)
    assert not bool(x.double().frac().any()) and float(xmax.max()) <= X_LIMIT
    out.worst = worst_sum_upper(packed, scale, N, K, bs) if upper_bound else worst_sum(packed, scale, N, K, bs, xmax, unit, chunk)
    assert_exact(out.worst, unit, dtype, float(X.BIAS_MAX) + (0.0 if nested else LC.ADAPTER_MAX))
    if with_reference:
        xt = x.double().t().contiguous()
        out.y64 = torch.empty((REF_ROWS, N), dtype=torch.float64, device=packed.device)
        for r0 in range(0, N, chunk):
            r1 = min(N, r0 + chunk)
            out.y64[:, r0:r1] = (L.rows64(packed, scale, K, bs, r0, r1) @ xt).t()
    return out


def build_adapters(case: LongCase, dtype: torch.dtype, device):
    """(t [REF_ROWS, r], stack [2, N, r], scalings [2] fp32): lora_cases' exact adapter operands at r = LORA_R, two different adapters."""
    gen = torch.Generator().manual_seed(case.seed * 131 + LORA_R)
    values = torch.tensor(LC.B_VALUES, dtype=torch.float32)
    t = LC._distinct_rows(lambda n: torch.randint(-LC.T_MAX, LC.T_MAX + 1, (n, LORA_R), generator=gen).float(), REF_ROWS)
    stack = values[torch.randint(0, len(LC.B_VALUES), (2, case.N, LORA_R), generator=gen)]
    assert not torch.equal(stack[0], stack[1])
    assert float(max(LORA_SCALINGS) * LC.T_MAX * max(LC.B_VALUES) * LORA_R) <= LC.ADAPTER_MAX
    return t.to(dtype).to(device), stack.to(dtype).to(device), torch.tensor(LORA_SCALINGS, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------ the geometry query
class tuned:
    """``with tuned(lib, call.tuning):`` the calling thread's stream tuning for the block (None: nothing to set), the defaults afterwards."""

    def __init__(self, lib, tuning):
        self.lib, self.tuning = lib, tuning

    def __enter__(self):
        if self.tuning is not None:
            self.lib.bnb_mi355x_set_stream_tuning(*self.tuning)

    def __exit__(self, *exc):
        if self.tuning is not None:
            self.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)


def query(lib, form: str, dtype: torch.dtype, M: int, N: int, K: int, blocksize: int):
    """bnb_mi355x_stream_geometry as (mb, waves, SW, P, R, grid_x, G, lds) - None where the form's predicates refuse the call."""
    import ctypes as ct

    out = (ct.c_int32 * 8)()
    if lib.bnb_mi355x_stream_geometry(FORMS.index(form), DT_CODE[dtype], M, N, K, blocksize, ct.addressof(out)) != 1:
        return None
    R, SW, G, P, grid, lds, mb, waves = list(out)
    return mb, waves, SW, P, R, grid, G, lds
