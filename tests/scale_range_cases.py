"""Inputs, references and the comparator for the scale-range tests of the STANDALONE kernels (quantize_4bit, dequantize_4bit and
its forced forms, dequantize_4bit_rows, the nested-statistics dequantize, quantize_blockwise / dequantize_blockwise). Pure torch /
numpy on the CPU; tests/test_scale_range_host.py asserts the properties the inputs are built for, tests/test_gpu_scale_range.py
shows them to the kernels.

The older tests keep every block scale in about [2^-6, 2^1]. Here the scale walks the whole fp32 range - subnormal scales, scales
whose reciprocal is subnormal, inf and NaN on the dequantize side - and, for the quantizers, every finite 16-bit value is the absmax
of some block whose other elements sit on the decision bounds scaled by it.

The references are restatements in float64 / separate fp32 torch operations:
  dequantize : T(fp32(code * scale))            - the product of two fp32 values is exact in float64, so `.float()` is ONE rounding
  quantize   : bitsandbytes/backends/default/ops.py:233-259 of the reference (reciprocal-multiply in full blocks, a true division in
               the ragged tail block), csrc/cpu_ops.cpp:496-665 for the 8-bit rule
The oracle (oracle/bnb4_oracle.c, pinned to the live reference by tests/test_oracle_pinning.py) is what the GPU tests compare
against; the host tests show that it equals these restatements on every input built here.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import oracle as O

MANTISSAS = (0x000000, 0x000001, 0x2AAAAA, 0x400000, 0x555555, 0x7FFFFF)
OFFSETS = (0.0, 0.03, -0.03, 2.0**-130, 2.0**100)
DT16 = (torch.bfloat16, torch.float16)
OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
TINY = 1e-38  # the reference's clamp of absmax (ops.py:245, :247); an fp32 subnormal

# Where the reference's own CPU paths disagree with each other:
#   * sign of zero: FP4 code 8 is +0 in the AVX512 table and -0 in the scalar one (csrc/cpu_ops.cpp:271-276 vs :279-282) - same_bits
#     accepts either zero where the wanted value is zero, nothing else;
#   * bf16 results below 2^-126: vcvtneps2bf16 (csrc/cpu_ops.cpp:386) flushes them, the scalar path (:139-144) and the oracle keep
#     them. The scalar rule is followed: such results must MATCH, they are not forgiven.
# Cases in which the kernels deviate from the scalar rule would be listed here as data; the sweep found none.
KNOWN_DEVIATIONS: tuple = ()


def _int_dtype(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


def f32_from_bits(bits) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).view(np.float32).copy())


def from_bits16(bits, dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits).astype(np.uint16)).view(np.int16).copy()).view(dtype)


def bits_of(t: torch.Tensor) -> np.ndarray:
    """Unsigned integer view of a float tensor."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------ the scale sets
@lru_cache(maxsize=None)
def _scale_bits() -> np.ndarray:
    exps = np.arange(255, dtype=np.uint32)[:, None] << 23
    body = (exps | np.asarray(MANTISSAS, dtype=np.uint32)[None, :]).reshape(-1)
    return np.concatenate([body, np.asarray([0x7F800000, 0x7FC00000], dtype=np.uint32)])


def scales() -> torch.Tensor:
    """Every biased fp32 exponent 0 ... 254 x six mantissas, then +inf and NaN: 1532 values, all with the sign bit clear."""
    return f32_from_bits(_scale_bits())


def finite_scales() -> torch.Tensor:
    s = scales()
    return s[torch.isfinite(s)]


def reciprocal_finite_scales() -> torch.Tensor:
    """Nonzero finite scales whose fp32 reciprocal is finite. (The reference's 8-bit rule casts NaN = 0 * inf to uint16_t where the
    reciprocal overflows: undefined behaviour in C, nothing to pin.)"""
    s = finite_scales()
    s = s[s != 0]
    return s[torch.isfinite(1.0 / s)]


# ------------------------------------------------------------------------------------------ comparator
def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit for bit. Forgiven: NaN against NaN (any payload), and either zero where the wanted value is a zero (conftest.same_values:
    the reference's own paths disagree on the sign of FP4's second zero). Nothing else - subnormals must match."""
    return first_mismatch(got, want) is None


def _mismatches(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    if got.dtype.is_floating_point:
        it = _int_dtype(got.dtype)
        bad = got.contiguous().view(it) != want.contiguous().view(it)
        bad &= ~(torch.isnan(got) & torch.isnan(want))
        bad &= ~((want == 0) & (got == 0))
    else:
        bad = got != want
    return bad


def first_mismatch(got: torch.Tensor, want: torch.Tensor, blocksize: Optional[int] = None,
                   scale: Optional[torch.Tensor] = None) -> Optional[str]:
    """None when same_bits holds, else a line that names the first wrong element: index, block, the block's scale (bits), got, want."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    bad = _mismatches(got, want)
    count = int(bad.sum())
    if count == 0:
        return None
    i = int(bad.nonzero()[0])
    g, w = got.detach().cpu().reshape(-1)[i], want.detach().cpu().reshape(-1)[i]
    if got.dtype.is_floating_point:
        gb, wb = int(bits_of(g.reshape(1))[0]), int(bits_of(w.reshape(1))[0])
        text = f"got {float(g)!r} (0x{gb:X}), want {float(w)!r} (0x{wb:X})"
    else:
        text = f"got {int(g)}, want {int(w)}"
    where = f"element {i}"
    if blocksize:
        where += f", block {i // blocksize}"
        if scale is not None:
            s = scale.detach().cpu().reshape(-1)[i // blocksize].float().reshape(1)
            where += f", scale {float(s[0])!r} (0x{int(bits_of(s)[0]):08X})"
    return f"{count} of {bad.numel()} differ; first: {where}: {text}"


def census(want: torch.Tensor) -> str:
    """Element count and the special wants a case covers (printed by the GPU tests)."""
    w = want.float().reshape(-1)
    lim = {torch.float32: 2.0**-126, torch.float16: 2.0**-14, torch.bfloat16: 2.0**-126}[want.dtype]
    sub = int(((w != 0) & (w.abs() < lim)).sum())
    return f"{w.numel()} elements, {sub} subnormal, {int(torch.isinf(w).sum())} inf, {int(torch.isnan(w).sum())} NaN wants"


# ------------------------------------------------------------------------------------------ dequantize_4bit
LINES_TILE = 8192  # the largest tile of the line-contiguous fp32 form (8 units per lane); a multiple of the 4096-element tile


def _all_bytes_every_block() -> torch.Tensor:
    """The 256 byte values in an order in which ANY 16 consecutive bytes carry all 16 nibbles in the high and in the low position
    (so every block of 32 elements or more decodes every code from both halves of a byte)."""
    j = torch.arange(256)
    hi = j & 15
    lo = (hi + (j >> 4)) & 15
    return ((hi << 4) | lo).to(torch.uint8)


class Dequant4Input(NamedTuple):
    packed: torch.Tensor  # uint8 [n / 2]
    absmax: torch.Tensor  # fp32 [n / blocksize]
    n: int
    blocksize: int
    quant_type: str


def dequant4_input(quant_type: str, blocksize: int, scale_set: torch.Tensor) -> Dequant4Input:
    """Per scale a group of max(512, blocksize) elements = the 256 byte values (repeated for the large blocksize), every block of the
    group under that scale; then blocks of zero bytes under scale 1 up to a whole number of LINES_TILE elements, so that every forced
    form of the line-contiguous fp32 kernel takes its own path."""
    group = max(512, blocksize)
    body = _all_bytes_every_block().repeat(group // 512)
    packed = body.repeat(scale_set.numel())
    absmax = scale_set.float().repeat_interleave(group // blocksize)
    n = scale_set.numel() * group
    pad = (-n) % LINES_TILE
    packed = torch.cat([packed, torch.zeros(pad // 2, dtype=torch.uint8)])
    absmax = torch.cat([absmax, torch.ones(pad // blocksize)])
    return Dequant4Input(packed.contiguous(), absmax.contiguous(), n + pad, blocksize, quant_type)


def _round_to(v64: torch.Tensor, dtype) -> torch.Tensor:
    """round_T(round_f32(v)) of an exactly known float64 value."""
    return v64.float().to(dtype)


def dequant4_want_from(packed: torch.Tensor, scale_per_block: torch.Tensor, n: int, blocksize: int, quant_type: str, dtype) -> torch.Tensor:
    code = O.get_4bit_code(quant_type).double()
    q = packed.reshape(-1).long()
    nib = torch.stack([q >> 4, q & 15], dim=1).reshape(-1)[:n]
    s = scale_per_block.double().repeat_interleave(blocksize)[:n]
    return _round_to(code[nib] * s, dtype)


def dequant4_want(inp: Dequant4Input, dtype) -> torch.Tensor:
    return dequant4_want_from(inp.packed, inp.absmax, inp.n, inp.blocksize, inp.quant_type, dtype)


# ------------------------------------------------------------------------------------------ dequantize_blockwise
def dynamic_map() -> torch.Tensor:
    import bitsandbytes_amd.functional as F

    return F.create_dynamic_map().float().cpu()


class Dequant8Input(NamedTuple):
    codes: torch.Tensor   # uint8 [n]
    absmax: torch.Tensor  # fp32 [n / blocksize]
    code: torch.Tensor    # fp32 [256]
    n: int
    blocksize: int


def dequant8_input(blocksize: int, scale_set: torch.Tensor) -> Dequant8Input:
    """Per scale a group of max(256, blocksize) elements = the 256 codes (repeated for the large blocksize)."""
    group = max(256, blocksize)
    codes = torch.arange(256, dtype=torch.uint8).repeat(group // 256).repeat(scale_set.numel())
    absmax = scale_set.float().repeat_interleave(group // blocksize)
    return Dequant8Input(codes.contiguous(), absmax.contiguous(), dynamic_map(), codes.numel(), blocksize)


def dequant8_want(inp: Dequant8Input, dtype) -> torch.Tensor:
    s = inp.absmax.double().repeat_interleave(inp.blocksize)
    return _round_to(inp.code.double()[inp.codes.long()] * s, dtype)


# ------------------------------------------------------------------------------------------ nested statistics
class NestedInput(NamedTuple):
    packed: torch.Tensor   # uint8 [n / 2]
    absmax8: torch.Tensor  # uint8 [n / blocksize]: every q8 in every group of 256 blocks
    absmax2: torch.Tensor  # fp32 [n / blocksize / 256]
    code2: torch.Tensor    # fp32 [256]
    n: int
    blocksize: int
    quant_type: str

    def scale(self, offset: float) -> torch.Tensor:
        """code2[q] * absmax2, rounded to fp32, then + offset, rounded again: two separate fp32 operations on the CPU
        (bitsandbytes/functional.py:1002-1006 of the reference: dequantize_blockwise, then `absmax += offset`)."""
        prod = self.code2[self.absmax8.long()] * self.absmax2.repeat_interleave(256)
        return prod + torch.tensor(offset, dtype=torch.float32)

    def want(self, offset: float, dtype) -> torch.Tensor:
        return dequant4_want_from(self.packed, self.scale(offset), self.n, self.blocksize, self.quant_type, dtype)

    def state(self, offset: float, dtype, device):
        import bitsandbytes_amd.functional as F

        s2 = F.QuantState(absmax=self.absmax2.to(device), code=self.code2.to(device), blocksize=256, dtype=torch.float32)
        return F.QuantState(absmax=self.absmax8.to(device), shape=torch.Size((self.n,)), code=O.get_4bit_code(self.quant_type).to(device),
                            blocksize=self.blocksize, quant_type=self.quant_type, dtype=dtype,
                            offset=torch.tensor(offset, dtype=torch.float32, device=device), state2=s2)


def nested_absmax2() -> torch.Tensor:
    """The positive finite part of scales(), every fourth exponent."""
    bits = _scale_bits()[:-2].reshape(255, len(MANTISSAS))[0::4].reshape(-1)
    return f32_from_bits(bits[bits != 0])


def nested_input(quant_type: str, blocksize: int) -> NestedInput:
    am2 = nested_absmax2()
    blocks = am2.numel() * 256
    n = blocks * blocksize
    packed = _all_bytes_every_block().repeat(n // 512)
    q8 = torch.arange(256, dtype=torch.uint8).repeat(am2.numel())
    return NestedInput(packed.contiguous(), q8.contiguous(), am2.contiguous(), dynamic_map(), n, blocksize, quant_type)


# ------------------------------------------------------------------------------------------ quantize_4bit
FP4_ORDER = (11, 10, 13, 12, 15, 14, 9, 0, 8, 1, 6, 7, 4, 5, 2, 3)  # ascending FP4 nibbles, +0 (nibble 0) before the second zero


@lru_cache(maxsize=None)
def bounds4(quant_type: str):
    """(the 15 fp32 midpoints of the sorted code, sorted position -> nibble)."""
    code = O.get_4bit_code(quant_type)
    order = torch.arange(16) if quant_type == "nf4" else torch.tensor(FP4_ORDER)
    srt = code[order]
    assert bool((srt[1:] >= srt[:-1]).all())
    return (srt[:-1] + srt[1:]) / 2, order


def positive_bounds(quant_type: str) -> torch.Tensor:
    b, _ = bounds4(quant_type)
    return b[b > 0]


def scaled_multiply(x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """The full-block rule: x * (1 / max(a, 1e-38)), clamped to [-1, 1]; separate fp32 operations."""
    return torch.clamp(x.float() * (1.0 / a.float().clamp(min=TINY)), -1, 1)


def scaled_divide(x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """The tail-block rule: x / max(a, 1e-38), clamped."""
    return torch.clamp(x.float() / a.float().clamp(min=TINY), -1, 1)


def position(s: torch.Tensor, quant_type: str) -> torch.Tensor:
    """Number of bounds strictly below s (torch.bucketize, right=False)."""
    b, _ = bounds4(quant_type)
    return torch.bucketize(s.contiguous(), b)


def quantize4_restated(A: torch.Tensor, blocksize: int, quant_type: str):
    """The reference's CPU quantize_4bit in plain torch: (packed uint8 [(n + 1) // 2, 1], absmax fp32). Finite inputs only."""
    _, order = bounds4(quant_type)
    x = A.reshape(-1).float()
    n = x.numel()
    full = n - n % blocksize
    body = x[:full].reshape(-1, blocksize)
    absmax = body.abs().amax(dim=1) if full else torch.empty(0)
    s = scaled_multiply(body, absmax[:, None]).reshape(-1)
    if n > full:
        am = x[full:].abs().max().clamp(min=TINY)
        absmax = torch.cat([absmax, am.reshape(1)])
        s = torch.cat([s, scaled_divide(x[full:], am)])
    if n % 2:
        s = torch.cat([s, torch.zeros(1)])
    q = order[position(s, quant_type)].to(torch.uint8)
    return ((q[0::2] << 4) | q[1::2]).reshape(-1, 1), absmax


def _top16(dtype16) -> int:
    return 0x7F80 if dtype16 == torch.bfloat16 else 0x7C00  # the bit pattern of +inf


def all_absmax16(dtype16) -> np.ndarray:
    """Bit patterns of every finite positive value of the type (bf16: 32 639, fp16: 31 743)."""
    return np.arange(1, _top16(dtype16), dtype=np.int64)


def absmax16_subset(dtype16) -> np.ndarray:
    """Every 16th finite positive value, and all of the two lowest and the two highest exponents."""
    a = all_absmax16(dtype16)
    shift = 7 if dtype16 == torch.bfloat16 else 10
    e = a >> shift
    top = (_top16(dtype16) >> shift) - 1
    keep = (np.arange(a.size) % 16 == 0) | (e <= 1) | (e >= top - 1)
    return a[keep]


def frontier_candidates(dtype16, quant_type: str, k: int = 3, absmax_bits: Optional[np.ndarray] = None):
    """(absmax bit patterns [A], candidate bit patterns [A, bounds, 2 k + 1]): around the representable value nearest to a * b,
    for every positive bound b, the k values on either side; nothing above a, nothing below zero."""
    a_bits = all_absmax16(dtype16) if absmax_bits is None else np.asarray(absmax_bits, dtype=np.int64)
    a = from_bits16(a_bits, dtype16).double()
    b = positive_bounds(quant_type).double()
    centre = bits_of((a[:, None] * b[None, :]).to(dtype16)).astype(np.int64)
    cand = centre[:, :, None] + np.arange(-k, k + 1, dtype=np.int64)[None, None, :]
    return a_bits, np.clip(cand, 0, a_bits[:, None, None])


def _blocks_with_head(head_bits: np.ndarray, vals: np.ndarray, blocksize: int) -> np.ndarray:
    """vals [A, V] laid out in blocks of `blocksize` with head_bits[a] as the first element of each; zero fill."""
    per = blocksize - 1
    nblk = -(-vals.shape[1] // per)
    fill = np.zeros((vals.shape[0], nblk * per - vals.shape[1]), dtype=vals.dtype)
    body = np.concatenate([vals, fill], axis=1).reshape(vals.shape[0], nblk, per)
    head = np.broadcast_to(head_bits[:, None, None], (vals.shape[0], nblk, 1)).astype(vals.dtype)
    return np.concatenate([head, body], axis=2).reshape(-1, blocksize)


def quant4_frontier(dtype16, quant_type: str, k: int = 3, blocksize: int = 64, absmax_bits: Optional[np.ndarray] = None) -> torch.Tensor:
    """Blocks [B, blocksize]: for every finite positive absmax a of the type (or the given ones) the candidates above, both signs, and
    a zero, with a itself at the head of every block (so the block's absmax is a)."""
    a_bits, cand = frontier_candidates(dtype16, quant_type, k, absmax_bits)
    pos = cand.reshape(cand.shape[0], -1)
    vals = np.concatenate([pos, pos | 0x8000, np.zeros((pos.shape[0], 1), dtype=np.int64)], axis=1)
    return from_bits16(_blocks_with_head(a_bits, vals, blocksize), dtype16)


def quant4_frontier_f32(quant_type: str, k: int = 8, blocksize: int = 64) -> torch.Tensor:
    """Blocks [B, blocksize] of fp32: for every nonzero finite scale a, the values within k ulps of a * b for all 15 bounds b, clipped
    to |x| <= a, a at the head of every block."""
    a = finite_scales()
    a = a[a != 0]
    a_bits = bits_of(a).astype(np.int64)
    b, _ = bounds4(quant_type)
    c = bits_of((a.double()[:, None] * b.double()[None, :]).float()).astype(np.int64)
    key = np.where(c & 0x80000000, -(c & 0x7FFFFFFF), c)  # sign-magnitude -> an integer line on which one step is one ulp
    key = key[:, :, None] + np.arange(-k, k + 1, dtype=np.int64)[None, None, :]
    key = np.clip(key, -a_bits[:, None, None], a_bits[:, None, None]).reshape(a_bits.size, -1)
    vals = np.where(key < 0, (-key) | 0x80000000, key)
    return f32_from_bits(_blocks_with_head(a_bits, vals, blocksize).astype(np.uint32))


def flips(blocks: torch.Tensor, quant_type: str, same_divisor: bool = False) -> torch.Tensor:
    """bool [B, blocksize]: elements whose code differs between the full-block rule x * (1 / max(a, 1e-38)) and a plain true division
    x / a by the block's absmax a (the first element of the block) - what a kernel that divides where it should multiply would
    compute. Two kinds of element flip:
      * a >= 1e-38: the two quotients differ in the last bit and a bound lies between them (FP4's bounds are small rationals, so
        ratios of 8- and 11-bit significands hit them; no such ratio lies within an ulp of an NF4 bound);
      * a < 1e-38 (bf16 only: 108 subnormal absmax values): the clamp changes the divisor itself.
    same_divisor=True keeps the first kind only: x * (1 / max(a, 1e-38)) against x / max(a, 1e-38), the tail block's rule. In a tail
    block the second kind tells a kernel that forgot the clamp (in the divisor or in the stored absmax) from a right one."""
    a = blocks[:, :1].float()
    other = scaled_divide(blocks, a) if same_divisor else torch.clamp(blocks.float() / a, -1, 1)
    return position(scaled_multiply(blocks, a), quant_type) != position(other, quant_type)


class TailCase(NamedTuple):
    A: torch.Tensor  # three full blocks of ordinary values, then the ragged tail
    tail: int        # elements in the tail
    j: int           # index, inside the tail, of an element whose code tells the two arithmetics apart


def tail_cases(dtype16, quant_type: str, limit: int = 256, blocksize: int = 64) -> list:
    """Up to `limit` frontier blocks (spread evenly over those that have one) with a flipping element at index j, each cut to a ragged
    tail of r elements, j < r < blocksize, behind three ordinary full blocks."""
    blocks = quant4_frontier(dtype16, quant_type, blocksize=blocksize)
    f = flips(blocks, quant_type)
    f[:, blocksize - 1] = False  # a tail is shorter than a block
    f[:, 0] = False              # (the absmax itself flips below the clamp: a * 1e38 < 1 = a / a; take an element behind it)
    rows = f.any(dim=1).nonzero().reshape(-1)
    if rows.numel() > limit:
        rows = rows[torch.linspace(0, rows.numel() - 1, limit).long()]
    g = torch.Generator().manual_seed(7)
    head = (torch.randn(3 * blocksize, generator=g) * 0.3).to(dtype16)
    out = []
    for i, r in enumerate(rows.tolist()):
        j = int(f[r].nonzero()[0])
        tail = j + 1 + i % (blocksize - 1 - j)
        out.append(TailCase(torch.cat([head, blocks[r, :tail]]).contiguous(), tail, j))
    return out


# ------------------------------------------------------------------------------------------ quantize_blockwise
def quantize8_restated(A: torch.Tensor, code: torch.Tensor, blocksize: int):
    """csrc/cpu_ops.cpp:496-665 of the reference in torch: the 65536-bin rule with the fused multiply-add the pinned binary uses
    (t * 65535 + 0.5 is exact in float64, so `.float()` rounds once). Whole blocks, nonzero finite absmax with a finite reciprocal."""
    x = A.reshape(-1, blocksize).float()
    am = x.abs().amax(dim=1)
    v = torch.clamp(x * (1.0 / am)[:, None], -1, 1)
    t = (v + 1.0) * 0.5
    u = (t.double() * 65535.0 + 0.5).float().to(torch.int32).float()
    val = -1.0 + (2.0 * u) / 65535.0
    mid = 0.5 * (code[:-1] + code[1:])
    return torch.bucketize(val.contiguous(), mid.contiguous()).to(torch.uint8).reshape(A.shape), am


def quant8_absmax(dtype) -> torch.Tensor:
    """reciprocal_finite_scales() as far as `dtype` holds them (rounded to it, duplicates, zeros and infinities dropped)."""
    a = reciprocal_finite_scales().to(dtype).float()
    a = torch.unique(a[torch.isfinite(a) & (a != 0)])
    return a[torch.isfinite(1.0 / a)]


def quant8_edges(code: torch.Tensor) -> torch.Tensor:
    """float64 [255]: where the 8-bit rule really decides. Midpoint i is compared with the VALUE OF A BIN, val(u) = -1 + 2 u / 65535,
    so the code changes where x / absmax crosses into the first bin T_i whose value lies above the midpoint: at
    (T_i - 0.5) * 2 / 65535 - 1, up to half a bin (1.5e-5) away from the midpoint itself - hundreds of fp32 ulps."""
    u = torch.arange(65536, dtype=torch.float32)
    val = -1.0 + (2.0 * u) / 65535.0
    mid = 0.5 * (code[:-1] + code[1:])
    first_above = torch.searchsorted(val.contiguous(), mid.contiguous(), right=True).double()
    return (first_above - 0.5) * 2.0 / 65535.0 - 1.0


def quant8_flips(blocks: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """bool [B, blocksize]: elements whose code differs between x * (1 / absmax) (the rule) and a true division x / absmax."""
    x = blocks.float()
    a = x[:, :1]
    mid = (0.5 * (code[:-1] + code[1:])).contiguous()

    def encode(v):
        t = (torch.clamp(v, -1, 1) + 1.0) * 0.5
        u = (t.double() * 65535.0 + 0.5).float().to(torch.int32).float()
        return torch.bucketize((-1.0 + (2.0 * u) / 65535.0).contiguous(), mid)

    return encode(x * (1.0 / a)) != encode(x / a)


def quant8_frontier(dtype, blocksize: int = 256) -> torch.Tensor:
    """Blocks [B, 256] of `dtype`: for every absmax a of quant8_absmax, the representable values within 2 ulps of a * m for the 255
    midpoints m of the dynamic map and of a * e for the 255 bin edges e where the code changes (quant8_edges), clipped to
    |x| <= a, a at the head of every block."""
    a = quant8_absmax(dtype)
    code = dynamic_map()
    m = torch.cat([(0.5 * (code[:-1] + code[1:])).double(), quant8_edges(code)])
    near = (a.double()[:, None] * m[None, :]).float().to(dtype)
    c = bits_of(near).astype(np.int64)
    a_bits = bits_of(a.to(dtype)).astype(np.int64)
    sign, mag = (0x80000000, 0x7FFFFFFF) if dtype == torch.float32 else (0x8000, 0x7FFF)
    key = np.where(c & sign, -(c & mag), c)
    key = key[:, :, None] + np.arange(-2, 3, dtype=np.int64)[None, None, :]
    key = np.clip(key, -a_bits[:, None, None], a_bits[:, None, None]).reshape(a_bits.size, -1)
    vals = _blocks_with_head(a_bits, np.where(key < 0, (-key) | sign, key), blocksize)
    return f32_from_bits(vals.astype(np.uint32)) if dtype == torch.float32 else from_bits16(vals, dtype)
