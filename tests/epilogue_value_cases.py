"""Builders shared by tests/test_epilogue_values_host.py (CPU) and tests/test_gpu_epilogue_values.py (GPU): the VALUE domain of the fused
epilogues - the gated activation ``T(T(silu(g)) * u)``, the final rounding ``T(acc + bias)``, the LoRA sum and the row scale. Pure
torch on the CPU.

The other exact suites (tests/exact_inputs.py) prove the kernels over shapes with a few thousand distinct values of modest magnitude;
the operands built here put chosen BIT PATTERNS into the epilogue instead:

* hand-packed weights (:func:`pack_one_hot`): every row holds code 1.0 at one or two columns and code 0.0 elsewhere, with a
  power-of-two fp32 absmax per block, packed directly (``quantize_4bit`` would give an all-zero block absmax 0). ``x @ W.T`` then
  copies activations into the accumulator: ``acc[m, n] = x[m, col(n)] * 2^p`` exactly, in any summation order.
* route 1 (:func:`gated_columns`, :func:`route1_rows`): gate row ``i`` one-hot at column ``i mod K``, up row ``i`` at a fixed
  permutation of it - ``g`` and ``u`` range over the finite 16-bit patterns (non-finite ones become zero: ``0 * inf`` would poison the
  row). Route 2: ``x = 0`` and the patterns arrive as the bias, so that +-inf, every NaN and -0 are gate values too.
* the comparison rule (:func:`differ`): equal NaN masks and equal integer views elsewhere - the sign of zero counts, NaN payloads do
  not.
* the anchor (:func:`silu_once`): float64 ``g / (1 + exp(-g))`` rounded ONCE to T, for every pattern (``.to(T)`` of a double
  rounds twice, through fp32: :func:`round_once` repairs it).
* the rounding grid (:func:`rounding_grid`): ``a * 2^p + b * 2^q + c`` for named (a, b, p, q, c) that land on ties, on the overflow
  threshold and among the subnormals of T, each term and every partial sum exactly representable in fp32 - the float64 sum rounded
  once is the only right answer.
* the LoRA reference in CPU float32 and the float64 emulation of a single-rounding fused multiply-add (:func:`lora_reference`,
  :func:`lora_fused_emulation`); the sample values of the row-scale sweep (:func:`scale_samples`).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

CODE_ONE = {"fp4": 3, "nf4": 15}
CODE_ZERO = {"fp4": 0, "nf4": 7}
DTYPES16 = (torch.bfloat16, torch.float16)
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
MANT_BITS = {torch.bfloat16: 7, torch.float16: 10}
K_STREAM, K_RT, K_PC, K_KQ, K_SM, K_EXPERTS = 1, 3, 4, 6, 7, 9
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
PATTERN_SEED = 20240607
LORA_SCALINGS = (1.0 / 3.0, 0.3, 16.0 / 24.0, 1.7)
LORA_RANKS = (8, 128)
LORA_MS = (1, 2, 9, 16)
# bf16 gate values at which the documented fp32 sequence leaves the real-valued function: expf(-g) overflows fp32, the quotient is -0,
# while g * exp(g) is still a bf16 normal or subnormal (-89 * e^-89 = -2e-37); below -97 the true value rounds to -0 as well
BF16_MINUS_ZERO_G = tuple(-89.0 - 0.5 * i for i in range(17))


# ------------------------------------------------------------------------------------------ patterns and comparison
def all_patterns(dtype: torch.dtype) -> torch.Tensor:
    """Every 16-bit pattern once, as T: index i holds the pattern whose unsigned value is i."""
    assert dtype in DTYPES16
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)   # (int32 -> int16 wraps: 0x8000 ... become negative)


def pattern_index(t: torch.Tensor) -> torch.Tensor:
    """The unsigned 16-bit pattern of every element of a 16-bit float tensor, as int64 (an index into :func:`all_patterns`)."""
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def shuffled_patterns(dtype: torch.dtype) -> torch.Tensor:
    """:func:`all_patterns` in a fixed random order: neighbouring (g, u) of route 1 are unrelated values."""
    gen = torch.Generator().manual_seed(PATTERN_SEED)
    return all_patterns(dtype)[torch.randperm(65536, generator=gen)]


def finite_count(dtype: torch.dtype) -> int:
    return int(torch.isfinite(all_patterns(dtype).float()).sum())


def differ(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Mask of the elements at which two results DISAGREE: one is a NaN and the other is not, or neither is and their bits differ
    (so +0 and -0 disagree, two NaNs of different payload agree)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    iv = INT_VIEW[a.dtype]
    return (na != nb) | (~na & ~nb & (a.contiguous().view(iv) != b.contiguous().view(iv)))


def values_differ(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """As :func:`differ`, but on values: -0 equals +0. A subnormal flushed to zero is a difference."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return (na != nb) | (~na & ~nb & (a.double() != b.double()))


def ordered_key(t: torch.Tensor) -> torch.Tensor:
    """A 16-bit float's position on the number line as an integer: neighbouring values differ by one, +-0 are both 0."""
    bits = pattern_index(t)
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


def from_key(key: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    bits = torch.where(key < 0, (-key) | 0x8000, key)
    return bits.to(torch.int32).to(torch.int16).view(dtype)


def round_once(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> T with ONE rounding to nearest even. torch converts a double through fp32; where that lands on the wrong side, one
    of the two neighbours of the result is strictly closer to ``v`` and is taken instead (an exact tie in float64 is exact in fp32
    too, and then the conversion is already right). Finite results of finite ``v`` only (no repair across the overflow threshold)."""
    assert v.dtype == torch.float64
    t = v.float().to(dtype)
    key = ordered_key(t)
    best, err = t.clone(), (t.double() - v).abs()
    top = 0x7F7F if dtype == torch.bfloat16 else 0x7BFF
    for step in (-1, 1):
        cand = from_key((key + step).clamp(-top, top), dtype)
        e = (cand.double() - v).abs()
        take = torch.isfinite(t.float()) & (e < err)
        best, err = torch.where(take, cand, best), torch.where(take, e, err)
    return best


@functools.lru_cache(maxsize=None)
def silu_once(dtype: torch.dtype) -> torch.Tensor:
    """[65536] T: float64 ``g / (1 + exp(-g))`` rounded once, indexed by g's pattern; NaN where g is not finite."""
    g = all_patterns(dtype).double()
    fin = torch.isfinite(g)
    gs = torch.where(fin, g, torch.zeros_like(g))
    out = round_once(gs / (1.0 + torch.exp(-gs)), dtype)
    return torch.where(fin, out, torch.full_like(out, float("nan")))


def silu_fp32_formula(g: torch.Tensor) -> torch.Tensor:
    """The documented sequence on the CPU: fp32 ``g / (1 + exp(-g))``, rounded to T."""
    gf = g.float()
    return (gf / (1.0 + torch.exp(-gf))).to(g.dtype)


def minus_zero_exception(g: torch.Tensor) -> torch.Tensor:
    """Mask of the gate values of the derived exception (bf16 only): -97 <= g <= -89."""
    if g.dtype != torch.bfloat16:
        return torch.zeros_like(g, dtype=torch.bool)
    gf = g.float()
    return (gf <= -89.0) & (gf >= -97.0)


def anchor_violations(g: torch.Tensor, got: torch.Tensor, table: torch.Tensor):
    """(mask of finite-g elements that miss the anchor, mask of finite-g elements that differ from the float64 value at all).
    ``got`` = T(silu(g)); ``table`` = :func:`silu_once` on g's device. The anchor: within one unit in the last place of the float64
    value rounded once; for the exception's gate values, exactly -0."""
    fin = torch.isfinite(g.float())
    want = table[pattern_index(g)]
    wsafe = torch.where(fin, want, torch.zeros_like(want))
    off = (ordered_key(got) - ordered_key(wsafe)).abs()
    exc = minus_zero_exception(g)
    bad = torch.where(exc, pattern_index(got) != 0x8000, torch.isnan(got) | (off > 1))
    diff = torch.isnan(got) | (off != 0) | ((off == 0) & (pattern_index(got) != pattern_index(wsafe)))
    return bad & fin, diff & fin


def u_list(dtype: torch.dtype) -> torch.Tensor:
    """The up values every gate pattern meets on route 2."""
    fi = torch.finfo(dtype)
    sub = 2.0 ** (-133 if dtype == torch.bfloat16 else -24)
    vals = [0.0, -0.0, sub, -sub, fi.tiny, -fi.tiny, 1.0, -1.0, fi.max, -fi.max, float("inf"), float("-inf"), float("nan"),
            0.5, -3.0, 1.0 / 3.0, 100.0, -0.007]
    if dtype == torch.float32:
        vals[2], vals[3] = 2.0 ** -149, -(2.0 ** -149)
    t = torch.tensor(vals, dtype=torch.float64).to(dtype)
    assert float(t[2]) == (2.0 ** -149 if dtype == torch.float32 else sub), "the smallest subnormal did not survive the conversion"
    return t


# ------------------------------------------------------------------------------------------ hand-packed weights
def pack_codes(codes: torch.Tensor, absmax: torch.Tensor) -> torch.Tensor:
    """Code indices uint8 [N, K] -> the packed bytes [N K / 2, 1]: ``(code[2 j] << 4) | code[2 j + 1]`` over the flat matrix."""
    flat = codes.reshape(-1)
    assert flat.numel() % 2 == 0 and absmax.dtype == torch.float32
    return ((flat[0::2] << 4) | flat[1::2]).reshape(-1, 1)


def pack_one_hot(N: int, K: int, blocksize: int, cols: torch.Tensor, exps: torch.Tensor, quant_type: str = "fp4"):
    """Rows with code 1.0 at ``cols[n, :]`` (int64 [N, C], C columns in C different blocks) and code 0.0 elsewhere; the block of
    ``cols[n, c]`` has absmax ``2 ** exps[n, c]``, every other block 1. Returns (packed uint8 [N K / 2, 1], absmax fp32 [N K / bs],
    W fp32 [N, K] - the matrix this must dequantize to)."""
    assert K % blocksize == 0 and K % 2 == 0 and cols.shape == exps.shape and cols.shape[0] == N
    blocks = cols // blocksize
    for c in range(1, cols.shape[1]):
        assert bool((blocks[:, c:] != blocks[:, c - 1:c]).all()), "two one-hot columns of a row share a quantization block"
    codes = torch.full((N, K), CODE_ZERO[quant_type], dtype=torch.uint8)
    codes.scatter_(1, cols, CODE_ONE[quant_type])
    absmax = torch.ones(N, K // blocksize, dtype=torch.float32)
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), exps.double()).float()
    absmax.scatter_(1, blocks, scale)
    W = torch.zeros(N, K, dtype=torch.float32)
    W.scatter_(1, cols, scale)
    return pack_codes(codes, absmax), absmax.reshape(-1), W


def up_perm(i: torch.Tensor, K: int, e: int = 0) -> torch.Tensor:
    """The fixed permutation of the columns that the up rows use (7 is coprime to every K here, asserted by gated_columns)."""
    return (7 * i + 3 + 5 * e) % K


def gated_columns(F: int, K: int, layout: str, E: int = 1):
    """(cols int64 [E * 2 F, 1] of the one-hot weight rows, gate_col [E, F], up_col [E, F]): gate row ``i`` of expert ``e`` at column
    ``(i + 11 e) mod K``, its up row at ``up_perm`` of ``i``. ``layout``: 'interleaved' (gate row 2 i, up row 2 i + 1) or 'chunked'
    (gate rows [0, F), up rows [F, 2 F))."""
    assert math.gcd(7, K) == 1
    i = torch.arange(F)
    gate = torch.stack([(i + 11 * e) % K for e in range(E)])
    up = torch.stack([up_perm(i, K, e) for e in range(E)])
    if layout == "interleaved":
        cols = torch.stack([gate, up], dim=2).reshape(E, 2 * F)
    else:
        assert layout == "chunked"
        cols = torch.cat([gate, up], dim=1)
    return cols.reshape(E * 2 * F, 1), gate, up


def bias_in_layout(bg: torch.Tensor, bu: torch.Tensor, layout: str) -> torch.Tensor:
    """[..., F] gate and up biases -> [..., 2 F] in the stack's row order."""
    if layout == "interleaved":
        return torch.stack([bg, bu], dim=-1).reshape(*bg.shape[:-1], -1)
    return torch.cat([bg, bu], dim=-1)


def route1_rows(pats: torch.Tensor, first: int, rows: int, K: int, stride: int, with_index: bool = False):
    """``rows`` activation rows [rows, K]: row m holds ``pats`` (cyclic) from position ``(first + m) * stride`` on, non-finite
    patterns replaced by +0. With ``stride`` = the number of distinct gate columns, consecutive rows continue the sweep.
    ``with_index``: also the position in ``pats`` of every element."""
    n = pats.numel()
    idx = ((first + torch.arange(rows))[:, None] * stride + torch.arange(K)[None, :]) % n
    x = pats[idx]
    x = torch.where(torch.isfinite(x.float()), x, torch.zeros_like(x))
    return (x, idx) if with_index else x


def fp32_sweep_values() -> torch.Tensor:
    """[131072] fp32: the 65536 values whose low 16 bits are zero, then 65536 random bit patterns from a fixed seed."""
    hi = (torch.arange(65536, dtype=torch.int64) << 16)
    gen = torch.Generator().manual_seed(PATTERN_SEED + 1)
    rnd = torch.randint(0, 1 << 32, (65536,), generator=gen, dtype=torch.int64)
    bits = torch.cat([hi, rnd])
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)


# ------------------------------------------------------------------------------------------ the final rounding
@dataclass(frozen=True)
class RoundingCase:
    name: str
    a: float
    p: int
    b: float
    q: int
    c: float

    @property
    def total(self) -> float:
        return self.a * 2.0 ** self.p + self.b * 2.0 ** self.q + self.c   # (float64; the host test asserts it is exact)


def _fits(v: float, dtype: torch.dtype) -> bool:
    return float(torch.tensor(v, dtype=torch.float64).to(dtype).double()) == v


@functools.lru_cache(maxsize=None)
def rounding_cases(dtype: torch.dtype):
    """The named (a, b, c, p, q) of a 16-bit type (module docstring; the issue's list). Two-term cases have c = 0; '-bias' variants
    carry the second term as the bias; '-neg' variants negate a, b and c."""
    mb = MANT_BITS[dtype]
    e = 10                                   # results in [1024, 2048): the fp32 ulp there, 2^-13, is a NORMAL value of both types
    U, u32 = 2.0 ** (e - mb), 2.0 ** (e - 23)
    hq = e - mb - 1                          # 2^hq = half a unit in the last place of T
    base = []
    for nm, a in (("tie-even", 1024 + 2 * U), ("tie-odd", 1024 + U)):
        base.append((nm, a, 0, 1.0, hq, 0.0))
        base.append((nm + "+ulp32", a, 0, 1.0, hq, u32))
        base.append((nm + "-ulp32", a, 0, 1.0, hq, -u32))
    mx = float(torch.finfo(dtype).max)
    if dtype == torch.float16:
        base += [("max+half-ulp", mx, 0, 1.0, 4, 0.0), ("max+quarter-ulp", mx, 0, 1.0, 3, 0.0), ("max+ulp", mx, 0, 1.0, 5, 0.0),
                 ("max+half-ulp-ulp32", mx, 0, 1.0, 4, -(2.0 ** -8)), ("max+half-ulp+ulp32", mx, 0, 1.0, 4, 2.0 ** -8)]
        s, sp, tiny_c = 2.0 ** -11, -14, 2.0 ** -24           # s * 2^sp = 2^-25: half the smallest subnormal
        fine = (2.0 ** -14, -14)                                # 2^-28
    else:
        base += [("max+half-ulp", mx, 0, 1.0, 119, 0.0), ("max+quarter-ulp", mx, 0, 1.0, 118, 0.0), ("max+3-quarter-ulp", mx, 0, 3.0, 118, 0.0),
                 ("max+half-ulp-ulp32", mx, 0, 1.0, 119, -(2.0 ** 104)), ("max+half-ulp+ulp32", mx, 0, 1.0, 119, 2.0 ** 104)]
        s, sp, tiny_c = 2.0 ** -100, -34, 2.0 ** -133         # s * 2^sp = 2^-134 (an fp32 subnormal accumulator)
        fine = (2.0 ** -100, -37)                               # 2^-137
    base += [("sub-exact", 10 * s, sp, 0.0, sp, 0.0), ("sub-tie-even", 5 * s, sp, 0.0, sp, 0.0), ("sub-tie-odd", 3 * s, sp, 0.0, sp, 0.0),
             ("zero-tie", s, sp, 0.0, sp, 0.0), ("zero-tie+", s, sp, fine[0], fine[1], 0.0), ("zero-tie-", s, sp, -fine[0], fine[1], 0.0),
             ("zero-tie+min-sub", s, sp, 0.0, sp, tiny_c),
             ("normal-boundary-tie", s * 2.0 ** (11 if dtype == torch.float16 else 8), sp, -s, sp, 0.0)]
    out = []
    for nm, a, p, b, q, c in base:
        variants = [(nm, a, p, b, q, c)]
        if c == 0.0 and b != 0.0 and _fits(b * 2.0 ** q, dtype):
            variants.append((nm + "-bias", a, p, 0.0, q, b * 2.0 ** q))
        for v in variants:
            out.append(RoundingCase(*v))
            out.append(RoundingCase(v[0] + "-neg", -v[1], v[2], -v[3], v[4], -v[5]))
    return tuple(out)


@dataclass
class RoundingGrid:
    dtype: torch.dtype
    ab: torch.Tensor        # [A, 2] T: the (a, b) of an activation row
    pq: torch.Tensor        # [R, 2] int64: the exponents of a weight row's two scales
    c: torch.Tensor         # [R] T: the bias of a weight row
    total: torch.Tensor     # [A, R] float64: a 2^p + b 2^q + c
    want: torch.Tensor      # [A, R] T: total rounded once (meaningful where `exact`)
    exact: torch.Tensor     # [A, R] bool: every term and every partial sum is an fp32 value, a, b, c are T values
    exact_nobias: torch.Tensor   # [A, R]: as `exact`, for the call without bias - only where c == 0
    want_nobias: torch.Tensor
    named: dict             # case name -> (row of ab, row of pq / c)


def _is_f32(v: torch.Tensor) -> torch.Tensor:
    return torch.isfinite(v) & (v.float().double() == v)


@functools.lru_cache(maxsize=None)
def rounding_grid(dtype: torch.dtype) -> RoundingGrid:
    """The cross product of the named cases' activation pairs and weight rows: every cell that qualifies is checked, the named
    ones are required to qualify (tests/test_epilogue_values_host.py)."""
    cases = rounding_cases(dtype)
    abs_, rows, named = [], [], {}
    for cs in cases:
        ab, r = (cs.a, cs.b), (cs.p, cs.q, cs.c)
        if ab not in abs_:
            abs_.append(ab)
        if r not in rows:
            rows.append(r)
        named[cs.name] = (abs_.index(ab), rows.index(r))
    ab64 = torch.tensor(abs_, dtype=torch.float64)
    pq = torch.tensor([[p, q] for p, q, _ in rows], dtype=torch.int64)
    c64 = torch.tensor([c for _, _, c in rows], dtype=torch.float64)
    ab, c = ab64.to(dtype), c64.to(dtype)
    assert torch.equal(ab.double(), ab64) and torch.equal(c.double(), c64), "a, b or c is not a value of T"
    two = torch.tensor(2.0, dtype=torch.float64)
    t1 = ab64[:, 0:1] * torch.pow(two, pq[:, 0].double())[None, :]
    t2 = ab64[:, 1:2] * torch.pow(two, pq[:, 1].double())[None, :]
    cc = c64[None, :].expand_as(t1)
    total = t1 + t2 + cc
    # (float64 adds of fp32-representable terms of these magnitudes are exact or far from fp32-representable: checked per subset)
    exact = _is_f32(t1) & _is_f32(t2) & _is_f32(t1 + t2) & _is_f32(t1 + cc) & _is_f32(t2 + cc) & _is_f32(total)
    nobias = _is_f32(t1) & _is_f32(t2) & _is_f32(t1 + t2) & (cc == 0)
    return RoundingGrid(dtype, ab, pq, c, total, total.float().to(dtype), exact, nobias, (t1 + t2).float().to(dtype), named)


def rounding_weights(grid: RoundingGrid, N: int, K: int, blocksize: int, quant_type: str = "fp4"):
    """(packed, absmax, W fp32 [N, K], row_of [N]): weight row n carries grid row ``n % R``: code 1.0 at k = 0 and k = K - blocksize
    (different blocks, different K quarters) with scales 2^p and 2^q."""
    R = grid.pq.shape[0]
    row_of = torch.arange(N) % R
    cols = torch.tensor([[0, K - blocksize]], dtype=torch.int64).expand(N, 2).contiguous()
    packed, absmax, W = pack_one_hot(N, K, blocksize, cols, grid.pq[row_of], quant_type)
    return packed, absmax, W, row_of


def rounding_weights_transposed(grid: RoundingGrid, N: int, blocksize: int, quant_type: str = "fp4"):
    """For ``grad_out @ W`` (gemm_4bit_grad_input, no bias): the two terms of output column ``j * blocksize`` sit in weight rows 0 and
    N - 1 of that column, with scales 2^p and 2^q of the j-th grid row that has c = 0. Returns (packed, absmax, W fp32 [N, K], rows - the
    grid row of every such column); K = the number of those rows in whole chunks of 256."""
    rows = torch.nonzero(grid.c.double() == 0).flatten()
    K = -(-(rows.numel() * blocksize) // 256) * 256
    codes = torch.full((N, K), CODE_ZERO[quant_type], dtype=torch.uint8)
    absmax = torch.ones(N, K // blocksize, dtype=torch.float32)
    W = torch.zeros(N, K, dtype=torch.float32)
    j = torch.arange(rows.numel())
    for n, which in ((0, 0), (N - 1, 1)):
        scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), grid.pq[rows, which].double()).float()
        codes[n, j * blocksize] = CODE_ONE[quant_type]
        absmax[n, j] = scale
        W[n, j * blocksize] = scale
    return pack_codes(codes, absmax), absmax.reshape(-1), W, rows


def rounding_activations(grid: RoundingGrid, K: int, blocksize: int, rows: int):
    """Activation chunks of exactly ``rows`` rows ([rows, K] T each, zero rows as padding) with x[m, 0] = a, x[m, K - bs] = b, and the
    grid row of every activation row (-1 = padding)."""
    A = grid.ab.shape[0]
    chunks = []
    for first in range(0, A, rows):
        n = min(rows, A - first)
        x = torch.zeros(rows, K, dtype=grid.dtype)
        x[:n, 0] = grid.ab[first:first + n, 0]
        x[:n, K - blocksize] = grid.ab[first:first + n, 1]
        idx = torch.full((rows,), -1, dtype=torch.int64)
        idx[:n] = torch.arange(first, first + n)
        chunks.append((x, idx))
    return chunks


# ------------------------------------------------------------------------------------------ LoRA, row scale
def lora_reference(vb64: torch.Tensor, lv64: torch.Tensor, scaling: float, dtype: torch.dtype) -> torch.Tensor:
    """The documented sequence in CPU float32: ``vb = acc + bias`` (exact), ``pr = float32(s) * lv`` (one rounding),
    ``T(vb + pr)`` (one rounding, then one to T)."""
    vb, lv = vb64.float(), lv64.float()
    assert torch.equal(vb.double(), vb64) and torch.equal(lv.double(), lv64), "acc + bias or lora is not exact in fp32"
    pr = torch.tensor(scaling, dtype=torch.float32) * lv
    return (vb + pr).to(dtype)


def lora_fused_emulation(vb64: torch.Tensor, lv64: torch.Tensor, scaling: float, dtype: torch.dtype) -> torch.Tensor:
    """What one fused multiply-add in place of the product and the sum would give: ``T(fp32(vb + float32(s) * lv))`` with the inner
    expression exact (float64 holds it: a 24-bit scaling times at most 14 bits, plus a value within 2^40 of its last place)."""
    s32 = float(torch.tensor(scaling, dtype=torch.float32))
    return (vb64 + s32 * lv64).float().to(dtype)


def scale_samples(dtype: torch.dtype, n: int) -> torch.Tensor:
    """[n] values of T for ``acc + b`` of the row-scale sweep: zeros, every kind of edge, all subnormals of a 16-bit type (a spread of
    them for fp32), then random finite bit patterns from a fixed seed."""
    fi = torch.finfo(dtype)
    gen = torch.Generator().manual_seed(PATTERN_SEED + 2)
    edge = torch.tensor([0.0, -0.0, fi.tiny, -fi.tiny, fi.max, -fi.max, 1.0, -1.0, 1.0 / 3.0, -255.0], dtype=torch.float64).to(dtype)
    if dtype == torch.float32:
        sub = torch.randint(1, 1 << 23, (254,), generator=gen, dtype=torch.int32).view(torch.float32)
        sub = torch.cat([sub, -sub, torch.tensor([2.0 ** -149, -(2.0 ** -149)])])
        rnd = torch.randint(-(1 << 31), 1 << 31, (4 * n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    else:
        pats = all_patterns(dtype)
        f = pats.float()
        sub = pats[(f != 0) & (f.abs() < fi.tiny)]
        rnd = pats[torch.randperm(65536, generator=gen)]
    rnd = rnd[torch.isfinite(rnd.float())]
    out = torch.cat([edge, sub, rnd])[:n]
    assert out.numel() == n and bool(torch.isfinite(out.float()).all())
    return out


def scale_weights(dtype_w: torch.dtype, n: int, seed: int) -> torch.Tensor:
    """[n] routing weights in ``dtype_w``: +-0, +-subnormal, +-inf, NaN, +-1, then random bit patterns OF ``dtype_w`` (32 random bits
    for fp32, 16 for a 16-bit type: an fp32 pattern rounded to fp16 is 0 or inf five times out of six)."""
    gen = torch.Generator().manual_seed(PATTERN_SEED + 3 + seed)
    if dtype_w == torch.float32:
        rnd = torch.randint(-(1 << 31), 1 << 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    else:
        rnd = torch.randint(-(1 << 15), 1 << 15, (n,), generator=gen, dtype=torch.int32).to(torch.int16).view(dtype_w)
    sub = 2.0 ** {torch.float32: -149, torch.float16: -24, torch.bfloat16: -133}[dtype_w]
    special = torch.tensor([0.0, -0.0, sub, -sub, float("inf"), float("-inf"), float("nan"), 1.0, -1.0], dtype=torch.float64)
    w = rnd.to(dtype_w).clone()
    w[:special.numel()] = special.to(dtype_w)
    return w


def scale_reference(vb: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """CPU float32 ``((acc + b) * w).to(T)``: vb [E, N] T, w [P] -> [P, N] for pairs that alternate over the experts."""
    E = vb.shape[0]
    e = torch.arange(w.numel()) % E
    return ((0.0 + vb.float()[e]) * w.float()[:, None]).to(vb.dtype)      # (acc = +0: a bias of -0 arrives as +0)


# ------------------------------------------------------------------------------------------ the sweeps' geometry
STREAM_SITES = ((4096, 4096), (2816, 2048))      # 2 F x K at M = 1: the exact-geometry instance and a general one
SM_SITE, SM_MS = (4096, 4096), (2, 4, 8, 16)     # the 4-, 8- and 16-row instances of the streaming MFMA kernel
EXPERTS_SITE = dict(E=2, N=2048, K=1024, blocksize=64, pairs=64)   # I = K = 1024: one pair carries 1024 patterns
QUANT_OF = {torch.bfloat16: "nf4", torch.float16: "fp4", torch.float32: "fp4"}
ROUNDING_SHAPE = (256, 1024, 64)                 # N x K, blocksize: in the geometry lists of every forced MFMA family
LORA_SHAPE = (4096, 4096, 64)                    # served by the streaming kernel (M = 1) and the streaming MFMA kernel


def route1_launches(F: int, K: int, rows: int, patterns: int = 65536) -> int:
    """Launches of ``rows`` activation rows after which every pattern has been a gate value (min(F, K) per row)."""
    per = rows * min(F, K)
    return (patterns + per - 1) // per


def lora_terms(ex, t: torch.Tensor, b: torch.Tensor):
    """(acc float64 [rows, N], lora float64 [rows, N]) of a tests/lora_cases.py case and adapter: both exact in any order."""
    return ex.x.double() @ ex.W.double().t(), t.double() @ b.double().t()
