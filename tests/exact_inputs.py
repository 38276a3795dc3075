"""Inputs for which ``x @ dequant(W).T (+ bias)`` is known to the last bit, whatever the order of summation.

A matmul test with a norm tolerance cannot see a row paired with the wrong activations, a k paired with the wrong weight or a block
scaled with its neighbour's absmax when it happens in one tile of one instance. With the operands built here it can, because the
right answer needs no tolerance:

* weights: FP4 codes from {0, +-1, +-0.5, +-0.25} (indices 0, 3, 5, 7, 11, 13, 15 of the FP4 table), code 1.0 at the head of every
  quantization block, times a per-block scale. Plain statistics: the scale is a power of two. Nested statistics: the caller hands the
  op its OWN second-level state - ``absmax_8bit`` codes into a 256-entry ``absmax_code`` table that holds NESTED_TABLE, a power-of-two
  ``absmax`` per 256 blocks and ``absmax_offset`` = 0.25 - so that ``code2[q] * absmax2 + offset`` is exact in fp32 (at most 7
  significant bits) and ``code4 * scale`` is exact in bf16 and fp16. Neighbouring blocks of a row never share a scale, neighbouring
  groups of 256 blocks never share an absmax2.
* activations / gradients: integers of magnitude <= 4, every row different from every other; an integer bias.
* reference: float64 matmul of the CONSTRUCTED operands (no library dequantize), rounded once to the output dtype.

"Exact" is asserted, not hoped for (:func:`check_quantization`, :func:`assert_exact_sums`): the quantizer returns the intended
absmax and the dequantizer returns W bit for bit; the nested reconstruction equals the intended scales bit for bit; and for the worst
output element the sum of the MAGNITUDES of its products (plus |bias|) stays below 2^24 times the power-of-two unit that every
product is a multiple of. Under that bound every fp32 partial sum - in any order, over any K split, through any slab reduction - is
an integer multiple of the unit below 2^24 units, hence exact; the float64 reference is exact for the same reason, so rounding it
once gives the only correct result.

The seven codes used here reach 49 of the 256 entries of a kernel's byte -> (code[hi], code[lo]) table and no NF4 entry; the other
codes, both tables and a caller-supplied one are read out bit for bit by tests/decode_probe_cases.py (one-hot rows, hand-packed bytes).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import torch

FP4_EXACT_VALUES = (0.0, 1.0, 0.5, 0.25, -1.0, -0.5, -0.25)  # FP4 indices 0, 3, 5, 7, 11, 13, 15
FP4_EXACT_INDICES = (0, 3, 5, 7, 11, 13, 15)
NESTED_TABLE = (0.25, 0.5, 1.0, 2.0, 3.0, 4.0)  # absmax_code[i] = NESTED_TABLE[i % 6]
NESTED_ABSMAX2_EXP = (-1, 0, 1, 0)              # absmax2 of group g = 2 ** NESTED_ABSMAX2_EXP[g % 4]
NESTED_OFFSET = 0.25
X_MAX = 4
BIAS_MAX = 8
FP16_MAX = 65504.0


@dataclass
class ExactInputs:
    N: int
    K: int
    blocksize: int
    dtype: torch.dtype
    nested: bool
    W: torch.Tensor            # [N, K] in `dtype`, CPU
    scale: torch.Tensor        # [N * K / blocksize] fp32: the intended absmax of every block
    unit: float                # every W[n, k] (and so every product with an integer) is an integer multiple of it
    x: torch.Tensor            # [rows, K] in `dtype`, integers, CPU
    bias: torch.Tensor         # [N] in `dtype`, integers, CPU
    # nested statistics (None for plain ones): what the op is handed as absmax_8bit, absmax_code, absmax (second level), absmax_offset
    absmax_8bit: Optional[torch.Tensor] = None
    absmax_code: Optional[torch.Tensor] = None
    absmax2: Optional[torch.Tensor] = None
    offset: Optional[torch.Tensor] = None

    def reference(self, with_bias: bool) -> torch.Tensor:
        """float64 ``x @ W.T (+ bias)`` of the constructed operands, rounded once to the output dtype."""
        if getattr(self, "_y64", None) is None or self._y64.shape[0] != self.x.shape[0]:
            self._y64 = self.x.double() @ self.W.double().t()   # (one float64 matmul per case)
        y = self._y64 + self.bias.double() if with_bias else self._y64
        return y.to(self.dtype)

    def stats_args(self, device):
        """(absmax, absmax_8bit, absmax_code, absmax_offset) as the gemm_4bit op takes them."""
        if not self.nested:
            return self.scale.to(device), None, None, None
        return self.absmax2.to(device), self.absmax_8bit.to(device), self.absmax_code.to(device), self.offset.to(device)


def int_rows(rows: int, cols: int, dtype: torch.dtype, gen: torch.Generator) -> torch.Tensor:
    """[rows, cols] integers in [-X_MAX, X_MAX], every row different from every other (asserted)."""
    x = torch.randint(-X_MAX, X_MAX + 1, (rows, cols), generator=gen, dtype=torch.int8)
    assert torch.unique(x, dim=0).shape[0] == rows, "two activation rows are equal"
    return x.to(dtype)


def build(N: int, K: int, blocksize: int, dtype: torch.dtype, nested: bool, seed: int, rows: int, exps=(-2, 3), bias_max: int = BIAS_MAX,
          allow_fp16_overflow: bool = False) -> ExactInputs:
    """Exactly representable weights, statistics, activations and bias (module docstring). ``exps``: the range of the power-of-two
    scales of plain statistics (inclusive; an even number of values). Asserts the bound for the forward product. ``bias_max`` = 0: a
    zero bias (windows of ``exps`` in which an integer is no multiple of the unit); ``allow_fp16_overflow``: see assert_exact_sums."""
    assert K % blocksize == 0, "a quantization block stays inside a row"
    gen = torch.Generator().manual_seed(seed)
    bpr = K // blocksize
    blocks = N * bpr
    col_parity = (torch.arange(bpr) & 1).expand(N, bpr)
    if nested:
        span = len(NESTED_TABLE)
        sel = (2 * torch.randint(0, span // 2, (N, bpr), generator=gen) + col_parity) % span   # parity follows the block column
        q8 = (sel + span * torch.randint(0, 256 // span, (N, bpr), generator=gen)).to(torch.uint8).reshape(-1)
        code2 = torch.tensor([NESTED_TABLE[i % span] for i in range(256)], dtype=torch.float32)
        groups = -(blocks // -256)
        absmax2 = torch.tensor([2.0 ** NESTED_ABSMAX2_EXP[g % 4] for g in range(groups)], dtype=torch.float32)
        offset = torch.tensor(NESTED_OFFSET, dtype=torch.float32)
        scale = code2[q8.long()] * absmax2.repeat_interleave(256)[:blocks] + offset   # (each step exact in fp32: <= 7 significant bits)
        unit = min(NESTED_TABLE) * 2.0 ** min(NESTED_ABSMAX2_EXP) * 0.25              # table x absmax2 granularity, x the smallest code
        assert NESTED_OFFSET % (unit / 0.25) == 0
    else:
        lo, hi = exps
        span = hi - lo + 1
        assert span % 2 == 0
        e = lo + (2 * torch.randint(0, span // 2, (N, bpr), generator=gen) + col_parity) % span
        scale = torch.ldexp(torch.ones(N, bpr), e).reshape(-1)   # (exact for subnormal powers of two as well)
        unit = 2.0 ** lo * 0.25
        q8 = code2 = absmax2 = offset = None
    s2 = scale.view(N, bpr)
    # (nested: neighbouring blocks never share a table entry, so inside a group of 256 blocks they never share a scale; across a group
    # boundary absmax2 changes as well and the two products may meet)
    differ = (sel[:, 1:] != sel[:, :-1]) if nested else (s2[:, 1:] != s2[:, :-1])
    assert bpr == 1 or bool(differ.all()), "neighbouring blocks share a scale"
    values = torch.tensor(FP4_EXACT_VALUES, dtype=torch.float32)
    W = torch.empty((N, K), dtype=dtype)
    for r0 in range(0, N, 1024):  # (in row slabs: the index tensor of a 8192 x 8192 matrix would be half a gigabyte)
        r1 = min(N, r0 + 1024)
        w = values[torch.randint(0, len(FP4_EXACT_VALUES), (r1 - r0, K), generator=gen)]
        w[:, ::blocksize] = 1.0   # code 1.0 at the head of every block: its absmax is the block's scale
        w32 = w * s2[r0:r1].repeat_interleave(blocksize, dim=1)
        W[r0:r1] = w32.to(dtype)
        assert torch.equal(W[r0:r1].float(), w32), "code x scale is not representable in the weight dtype"
    x = int_rows(rows, K, dtype, gen)
    bias = torch.randint(-bias_max, bias_max + 1, (N,), generator=gen).to(dtype)
    ex = ExactInputs(N, K, blocksize, dtype, nested, W, scale, unit, x, bias, q8, code2, absmax2, offset)
    assert_exact_sums(ex.W, ex.x, ex.unit, dtype, extra=float(bias_max), allow_fp16_overflow=allow_fp16_overflow)
    return ex


def assert_exact_sums(W: torch.Tensor, x: torch.Tensor, unit: float, dtype: torch.dtype, extra: float = 0.0, transposed: bool = False,
                      allow_fp16_overflow: bool = False) -> float:
    """The condition under which every fp32 partial sum of ``x @ W.T`` (``x @ W`` if ``transposed``) is exact in any order: all
    operands are multiples of their units, and the largest sum of product MAGNITUDES (+ ``extra``, the bias) is below 2^24 units -
    and below the largest fp16 value for fp16 results (``allow_fp16_overflow`` lifts that one condition: the top windows of
    tests/matmul_scale_range_cases.py, where the exact fp32 sum rounded once to fp16 may be +-inf and that is the wanted result). The
    bound used is sum_k max_m |x[m, k]| * |W[n, k]|, an upper bound of the worst (m, n). Returns it."""
    assert not bool(x.double().frac().any()) and float(x.abs().max()) <= X_MAX
    xmax = x.abs().amax(dim=0).double()
    worst_rows, col_sums = 0.0, torch.zeros(W.shape[1], dtype=torch.float64)
    for r0 in range(0, W.shape[0], 1024):  # (in row slabs: no float64 copy of a whole 8192 x 8192 matrix)
        a = W[r0:r0 + 1024].double().abs_()
        assert not bool((a / unit).frac_().any()), "a weight is not a multiple of the unit"
        if transposed:   # y[m, k] = sum_n x[m, n] W[n, k]
            col_sums += (a * xmax[r0:r0 + 1024, None]).sum(dim=0)
        else:            # y[m, n] = sum_k x[m, k] W[n, k]
            worst_rows = max(worst_rows, float((a @ xmax).max()))
    worst = float(col_sums.max()) if transposed else worst_rows
    worst += extra
    assert worst < 2.0 ** 24 * unit, f"sum of |products| {worst} reaches 2^24 units ({2.0 ** 24 * unit}): fp32 partial sums may round"
    if dtype == torch.float16 and not allow_fp16_overflow:
        assert worst < FP16_MAX, f"sum of |products| {worst} reaches the fp16 range"
    return worst


@dataclass
class QuantOps:
    """The three library calls the preconditions are checked through (the oracle's on the CPU, the product's on the GPU)."""
    quantize_4bit: Callable      # (W, blocksize) -> (packed, absmax)              FP4
    dequantize_4bit: Callable    # (packed, absmax, blocksize, shape, dtype) -> W   FP4
    dequantize_blockwise: Callable  # (codes uint8, absmax, code table, blocksize) -> fp32


def check_quantization(ex: ExactInputs, ops: QuantOps, device="cpu") -> torch.Tensor:
    """Quantize ``ex.W`` and assert that nothing was lost: the absmax returned is the intended scale, the dequantized weight is W
    bit for bit, and (nested) the library's own second-level reconstruction gives the intended scales bit for bit. Returns the
    packed weight on ``device``."""
    W = ex.W.to(device)
    packed, absmax = ops.quantize_4bit(W, ex.blocksize)
    assert absmax.dtype == torch.float32 and torch.equal(absmax.flatten().cpu(), ex.scale), "quantize_4bit: absmax is not the intended scale"
    back = ops.dequantize_4bit(packed, absmax, ex.blocksize, (ex.N, ex.K), ex.dtype)
    assert back.dtype == ex.dtype and torch.equal(back.cpu().view(torch.uint8), ex.W.view(torch.uint8)), "dequantize_4bit(quantize_4bit(W)) != W"
    if ex.nested:
        rec = ops.dequantize_blockwise(ex.absmax_8bit.to(device), ex.absmax2.to(device), ex.absmax_code.to(device), 256)
        rec = rec.float() + ex.offset.to(device)
        assert torch.equal(rec.flatten().cpu(), ex.scale), "nested statistics do not reconstruct the intended scales"
    return packed


# ------------------------------------------------------------------------------------------ the cases of the routed sweep
@dataclass(frozen=True)
class SweepCase:
    name: str
    N: int
    K: int
    blocksize: int = 64
    dtype: torch.dtype = torch.bfloat16
    nested: bool = False
    exps: tuple = (-2, 3)

    @property
    def seed(self) -> int:
        return (self.N * 31 + self.K * 7 + self.blocksize + (1 if self.nested else 0)) % (1 << 31)


# One case per branch of the routing tables (backends/hip.py: fused_max_m; csrc/gemm4_mfma.hip: gemm_4bit_route; csrc/gemm4_mfma.hip:
# sm_selected, kq_selected, rt_selected, make_plan). The comment names what the case is there for.
SWEEP_CASES = (
    SweepCase("4096x4096", 4096, 4096),                        # square-ish: fused to 640; sm 2-16, rt 17-48, pc, kq from 65, grid.z passes
    SweepCase("4096x4096-nested", 4096, 4096, nested=True),
    SweepCase("4096x10752", 4096, 10752),                      # long rows: fused to 1024; sm only to 8 rows
    SweepCase("11008x4096-nested", 11008, 4096, nested=True),  # wide: 512; kq from 17 rows with nested blocksize-64 statistics
    SweepCase("8192x8192", 8192, 8192),                        # above 48 M weights: 512; largest workspaces
    SweepCase("1376x4096", 1376, 4096),                        # fewer tiles than CUs (sm_selected's small-matrix table), K >= 2 N: 1024
    SweepCase("4096x2752", 4096, 2752),                        # K % 256 != 0: sm row passes to 128, unfused from 129
    SweepCase("4096x2752-nested", 4096, 2752, nested=True),
    SweepCase("1376x2752", 1376, 2752),
    SweepCase("1376x2752-nested", 1376, 2752, nested=True),
    SweepCase("96x2752-nested", 96, 2752, nested=True),        # below SM_MIN_ROWS: the streaming kernel's 4-row passes to 16
    SweepCase("4100x1024", 4100, 1024),                        # ragged N: a partial last tile in every family
    SweepCase("130x768", 130, 768),
    SweepCase("4096x4096-bs32", 4096, 4096, blocksize=32),     # the rt kernel's BS32 instances to 128
    SweepCase("4096x4096-bs32-nested", 4096, 4096, blocksize=32, nested=True),  # the streaming kernel to 16
    SweepCase("5120x5120-bs128-nested", 5120, 5120, blocksize=128, nested=True),  # nested outside the kq kernel's reach: pc keeps 512
    SweepCase("3200x4096-bs1024", 3200, 4096, blocksize=1024),  # blocksize above 256
    SweepCase("4096x4096-fp16", 4096, 4096, dtype=torch.float16, exps=(-2, 1)),  # the f16 instances of every family
    SweepCase("4096x4096-fp32", 4096, 4096, dtype=torch.float32),  # fp32 activations: fused to 4 rows only
)

FUSED_MAX_M_FP32 = 4  # (bnb_mi355x_gemm_4bit_fused_max_m at fp32)


def sweep_ms(fused_max: int):
    """Every M the sweep runs for a case: 1 ... fused_max + 1 without a gap, then the next multiple of 64 plus one, and one beyond
    1024 - rows that run dequantize + the library GEMM."""
    extra = sorted({(fused_max // 64 + 1) * 64 + 1, max(1030, fused_max + 6)})
    return list(range(1, fused_max + 2)) + [m for m in extra if m > fused_max + 1]


def first_mismatch(y: torch.Tensor, ref: torch.Tensor):
    """(row, column, got, want) of the first differing element of two [M, N] tensors (None if they agree)."""
    bad = (y != ref).nonzero()
    if bad.numel() == 0:
        return None
    r, c = int(bad[0, 0]), int(bad[0, 1])
    return r, c, float(y[r, c]), float(ref[r, c])


def grad_inputs(ex: ExactInputs, rows: int, seed: int):
    """Integer gradients [rows, N] for the fused backward and the float64 ``g @ W`` rounded once; asserts the exact-sum bound of the
    transposed product."""
    gen = torch.Generator().manual_seed(seed)
    g = int_rows(rows, ex.N, ex.dtype, gen)
    assert_exact_sums(ex.W, g, ex.unit, ex.dtype, transposed=True)
    return g, (g.double() @ ex.W.double()).to(ex.dtype)
