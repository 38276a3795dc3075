"""Builders shared by tests/test_matmul_scale_range_host.py (CPU) and tests/test_gpu_matmul_scale_range.py (GPU): the FUSED 4-bit
matmul kernels under block scales from the whole fp32 range. Pure torch on the CPU.

tests/scale_range_cases.py walks the scale through the standalone quantize / dequantize kernels; the bit-exact matmul suites
(exact_inputs, decode_probe_cases, epilogue values, large offsets, CU counts) keep every scale in 2^-2 ... 2^3. Three parts:

1. One-hot probe under every scale (:func:`build`, :func:`want_forward`, :func:`want_backward`). The construction of the decode probe -
   one-hot activation rows, hand-packed bytes, N = 1040 - with the per-block scale taken from ``scale_range_cases.scales()``. One
   non-zero term per output, so the result does not depend on the summation order; it DOES depend on where the kernel rounds, and the
   families do not share one arithmetic. :data:`ORDER` is the ledger, taken from the kernel sources, and
   :func:`restate` is each order in separate CPU fp32 operations (torch honours fp32 subnormals).
2. Dense exact sums at the ends of the range (:data:`WINDOWS`, :func:`window_inputs`): ``exact_inputs.build`` with its power-of-two
   scales moved to the bottom and to the top of what the type holds, where every order gives the same answer (asserted on the host).
3. Non-finite operands (:func:`clean_inputs`, :func:`poison_blocks`, :func:`poison_activations`): one block scale, activation or bias
   element set to inf / NaN in an otherwise clean dense case; its own row or column must turn non-finite, every other output keeps the
   bits of the clean call.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace
from typing import Optional

import torch

import decode_probe_cases as P
import exact_inputs as X
import scale_range_cases as R

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
N_FWD = P.N_FWD
GENERIC_ID = 2     # bnb_mi355x_last_gemm_kernel(): the generic scalar kernel
FAMILY_ID = dict(P.FAMILY_ID, generic=GENERIC_ID)

# ------------------------------------------------------------------------------------------ the order ledger
# Where a family rounds, read from its source (not from what the GPU returns). c = the fp32 code value, s = the fp32 block scale,
# v = the one activation of the probe row, T = the activations' type; fl32 = one fp32 rounding.
#   'A'   T(fl32(fl32(T(c) * v) * s))   the decode table holds T(c) (pack2<T>), the MFMA sums T(c) * x in fp32, the scale is applied to
#                                       a block's partial sum: fmaf(scale, part, acc) (gemm4_mfma.hip, _sm, _rt), v_pk_fma_f32 (_kq)
#   'A32' T(fl32(fl32(c * v) * s))      the same order with the table in fp32 - "the code values are not rounded to bf16 on the way"
#                                       (gemv4_stream.hip, 16-bit instances: sum * scale_u; gemm4_experts.hip: (...) * scale; the generic
#                                       kernel: fmaf(block_scale, run, acc))
#   'B16' T(fl32(T(fl32(c * s))) * v)   the operand of the MFMA is the dequantized weight, rounded to fp32 and then to T
#                                       (gemm4_mfma_tall.hip: pack(rounded_f32(pr * scale)); gemm4_grad_input.hip)
#   'B32' fl32(fl32(c * s) * v)         gemv4_stream.hip, fp32 instances: the PRESCALE branch
# For T = fp32 'A' and 'A32' are one order.
ORDER = {
    "stream": {BF: "A32", HF: "A32", F32: "B32"},
    "generic": {BF: "A32", HF: "A32", F32: "A32"},
    "experts": {BF: "A32", HF: "A32", F32: "A32"},
    "sm": {BF: "A", HF: "A"},
    "rt": {BF: "A", HF: "A"},
    "kq": {BF: "A", HF: "A"},
    "pc": {BF: "A", HF: "A"},
    "tall": {BF: "B16", HF: "B16"},
    "grad_input": {BF: "B16", HF: "B16"},
}
ORDERS = ("A", "A32", "B16", "B32")
# The post-scaled orders multiply a PARTIAL SUM by the scale: the products of GRANULE consecutive k are summed first. Under a one-hot
# row that is invisible for a finite scale (the other terms are zeros) and visible for a non-finite one: a zero partial sum times
# inf is NaN, the probed partial sum times inf is +-inf. 32: the 32-nibble run of a lane (gemv4_stream.hip, gemm4_experts.hip, whose
# other lanes' runs share the block from blocksize 64 on); 64: the 64-k partial tile of the MFMA kernels (the blocksize-32 instances
# of the rt kernel: one 32-k MFMA step); 1: the generic kernel, whose lanes stride the row by 64. The pre-scaled orders have no granule.
GRANULE = {"stream": 32, "experts": 32, "generic": 1, "sm": 64, "rt": 64, "kq": 64, "pc": 64}


def granule(family: str, blocksize: int) -> int:
    return min(GRANULE[family], blocksize)


def restate(order: str, c: torch.Tensor, s: torch.Tensor, v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """One order of :data:`ORDER` on broadcastable fp32 tensors (code value, scale, activation), every step a separate fp32 torch
    operation; the result in ``dtype``."""
    assert c.dtype == s.dtype == v.dtype == torch.float32
    if order == "A":
        return ((c.to(dtype).float() * v) * s).to(dtype)
    if order == "A32":
        return ((c * v) * s).to(dtype)
    if order == "B16":
        return ((c * s).to(dtype).float() * v).to(dtype)
    assert order == "B32" and dtype == torch.float32
    return (c * s) * v


def order_of(family: str, dtype: torch.dtype) -> str:
    return ORDER[family][dtype]


# ------------------------------------------------------------------------------------------ part 1: the cases
def _coprime_stride(n: int, near: float = 0.381) -> int:
    """A stride coprime to n, about ``near`` * n: consecutive multiples are far apart modulo n."""
    s = max(1, int(n * near))
    while math.gcd(s, n) != 1:
        s += 1
    return s


ProbeCase = P.ProbeCase
SPARSE_ABOVE = 1024   # cases with longer rows probe a subset of the k positions (:func:`probe_ks`)


def _fwd(family, K, combos, **kw):
    return [ProbeCase(family, dt, qt, bs, nested, N_FWD, K, fill="scales", **kw) for (dt, qt, bs, nested) in combos]


K_NESTED = 6144       # 1040 x 6144 / 64 / 256 = 390 groups of 256 blocks: one per second-level scale of nested_absmax2() and 7 to spare


def _cases():
    c = {}
    p16 = [(BF, "nf4", 64, False), (BF, "fp4", 64, False), (HF, "nf4", 64, False), (HF, "fp4", 64, False)]
    n16 = [(BF, "nf4", 64, True), (HF, "fp4", 64, True)]
    big = lambda combo: [(combo[0], combo[1], 4096, False)]
    # streaming kernel (kernel=1): K = two 256-k segments and a 64-k remainder; one row per call (the decode instance) and all rows in
    # one call (the 4-row passes)
    c["stream"] = (_fwd("stream", 576, [p16[0], p16[3], (F32, "nf4", 64, False)], rows=1) +
                   _fwd("stream", 576, [p16[1], p16[2], (F32, "fp4", 64, False)]) +
                   _fwd("stream", 4096, big(p16[0]) + big((F32, "fp4")), fills=2) +
                   _fwd("stream", K_NESTED, n16 + [(F32, "nf4", 64, True)]) + _fwd("stream", K_NESTED, n16[:1], rows=1))
    # the generic scalar kernel: reached as test_gemm_fp32_and_generic_fallbacks reaches it (kernel=1 and a K the streaming kernel
    # refuses: K % 32 != 0); blocks follow the flat index and span rows
    # (1040 x 80 / 64 = 1300 blocks a fill, three fills: a dedicated non-finite block spans two rows and takes their other blocks with it; 1040 x 6160 / 4096 = 1565 blocks a fill, a block longer than half a row)
    c["generic"] = (_fwd("generic", 80, p16 + [(F32, "nf4", 64, False), (F32, "fp4", 64, False)], fills=3) +
                    _fwd("generic", 6160, big(p16[2]), fills=2) + _fwd("generic", 6160, [(BF, "nf4", 64, True)]))
    # streaming MFMA kernel: 2 ... 16 rows per call
    c["sm"] = (_fwd("sm", 576, p16, knob=5000, rows=16) + _fwd("sm", 576, p16[:1], knob=5000, rows=2) + _fwd("sm", 576, p16[3:], knob=5000, rows=5) +
               _fwd("sm", 4096, big(p16[1]), knob=5000, rows=16, fills=2) + _fwd("sm", K_NESTED, n16, knob=5000, rows=16))
    # register-transposed kernel, its blocksize-32 instances (plain statistics) and the two-slice form
    c["rt"] = (_fwd("rt", 512, p16 + [(BF, "nf4", 32, False), (HF, "fp4", 32, False)], knob=2001) +
               _fwd("rt", 4096, big(p16[2]), knob=2002, fills=2) + _fwd("rt", K_NESTED, n16, knob=2001))
    # K-quarter kernel: nested statistics at blocksize 64 and K <= 16384 only
    c["kq"] = (_fwd("kq", 512, p16, knob=4001) + _fwd("kq", 4096, big(p16[3]), knob=4002, fills=2) + _fwd("kq", K_NESTED, n16, knob=4001))
    # producer/consumer kernel: geometry 11 for the four combinations, 12 - 14 once each at their own row counts
    c["pc"] = (_fwd("pc", 512, p16, knob=1101) + _fwd("pc", 512, p16[3:], knob=1201, rows=48) + _fwd("pc", 512, p16[1:2], knob=1301, rows=32) +
               _fwd("pc", 512, p16[2:3], knob=1401, rows=16) + _fwd("pc", 4096, big(p16[0]), knob=1102, fills=2) +
               _fwd("pc", K_NESTED, n16, knob=1101))
    # tall-tile kernel (knob cfg 60)
    c["tall"] = _fwd("tall", 512, p16, knob=6000) + _fwd("tall", 4096, big(p16[1]), knob=6000, fills=2) + _fwd("tall", K_NESTED, n16, knob=6000)
    # experts kernel, E = 3: [272, 576] for the plain scales, [1040, 2048] for the nested ones (3120 rows x 32 blocks = 390 groups),
    # [272, 4096] for blocksize 4096 (816 blocks a fill)
    ex = lambda combos, N, K, **kw: [ProbeCase("experts", dt, qt, bs, nested, N, K, fill="scales", E=3, **kw) for (dt, qt, bs, nested) in combos]
    c["experts"] = (ex([p16[0], p16[3], (F32, "nf4", 64, False), (BF, "fp4", 32, False)], 272, 576) + ex(big(p16[2]), 272, 4096, fills=2) +
                    ex(n16 + [(F32, "fp4", 64, True)], 1040, 2048))
    # fused backward, plans 'single' and 'sliced': [320, 640] (N = 5 kGiNAlign, K = 5 kGiCols), [320, 16384] for blocksize 4096 (four
    # block columns, the last one the poisoned one: two fills of 960 checked blocks), [960, 6656] for the nested scales (390
    # groups). The backward contracts over the weight ROWS, so one non-finite weight turns its k column into NaN in every probe row:
    # the non-finite scales stay in the last block column(s) (:func:`poison_columns`), and the nested cases carry no non-finite
    # second-level scale at all (a group of 256 blocks spans every block column of a 104-block row) - part 3 sets those, one per
    # call, at a shape whose rows are longer than a group (NESTED_DENSE).
    gi = lambda combos, N, K, plan, **kw: [ProbeCase("grad_input", dt, qt, bs, nested, N, K, fill="scales", plan=plan, **kw)
                                          for (dt, qt, bs, nested) in combos]
    c["grad_input"] = (gi(p16, 320, 640, "single") + gi(p16, 320, 640, "sliced") + gi(big(p16[0]), 320, 16384, "single", fills=2) +
                       gi(n16[:1], 960, 6656, "single") + gi(n16[1:], 960, 6656, "sliced"))
    return c


CASES = _cases()
ALL_CASES = tuple(cs for fam in CASES.values() for cs in fam)
# A family without a blocksize-4096 case, and why (none: every family has one)
NO_BS4096 = {}


def probe_ks(cs: ProbeCase) -> torch.Tensor:
    """The k positions a forward case probes. Rows up to SPARSE_ABOVE: every k. Longer rows: two (the generic kernel, whose blocks
    start at any multiple of 16: four) per group of 64 k, the position inside the group moving with the group, so that every block of
    every row is probed and every position inside a 64-group - even and odd: both nibbles - is probed in some group."""
    K = cs.K
    if K <= SPARSE_ABOVE:
        return torch.arange(K)
    g = torch.arange(-(K // -64))
    if cs.family == "generic":
        ks = torch.stack([64 * g + (g % 16) + 16 * i for i in range(4)], dim=1).reshape(-1)
    else:
        ks = torch.stack([64 * g + (2 * g) % 64, 64 * g + (2 * g + 33) % 64], dim=1).reshape(-1)
    return ks[ks < K]


# ------------------------------------------------------------------------------------------ part 1: bytes and scales
@functools.lru_cache(maxsize=2)
def build_bytes(cs: ProbeCase) -> torch.Tensor:
    """uint8 [weight rows, K / 2]. Byte (n, j): high nibble (j + n) mod 16, low nibble (high + j / 16 + n / 16) mod 16. Every aligned run
    of 16 bytes - so every quantization block of 32 elements or more - holds all 16 codes in the high and in the low nibble, every
    column meets all 16 codes in 16 consecutive rows, and all 256 byte values occur."""
    R_, J = cs.weight_rows, cs.K // 2
    n, j = torch.arange(R_)[:, None], torch.arange(J)[None, :]
    hi = (j + n) & 15
    lo = (hi + (j >> 4) + (n >> 4)) & 15
    b = ((hi << 4) | lo).to(torch.uint8)
    assert torch.bincount(b.reshape(-1).long(), minlength=256).min() > 0, "a byte value does not occur"
    return b


def nonfinite_rows(cs: ProbeCase) -> dict:
    """Plain statistics: weight row -> (block of the row, scale) of the dedicated non-finite rows: the first block of a row, a
    middle block, the first block of a row of the ragged last tile and the last block of the matrix. The fused backward contracts
    over the weight rows - a non-finite weight costs its k column in every probe row - so there the four stay in one block column."""
    R_ = cs.weight_rows
    inf, nan = float("inf"), float("nan")
    if cs.family == "grad_input":    # (the same rows, all in the last block column: poison_columns)
        return {7: ("last", inf), R_ // 2 + 1: ("last", nan), R_ - 9: ("last", nan), R_ - 1: ("last", inf)}
    return {7: ("first", inf), R_ // 2 + 1: ("middle", nan), R_ - 9: ("first", nan), R_ - 1: ("last", inf)}


def poison_columns(cs: ProbeCase) -> torch.Tensor:
    """Fused backward, plain statistics: bool [blocks per row], the block columns that hold every non-finite weight of the case - the
    dedicated non-finite scales and the finite scales T does not hold (fp16: 2^16 and up, 44 % of the scales: T(code * scale) is
    inf). The last column, or as many of the last columns as the share of those scales."""
    bpr = cs.K // cs.blocksize
    assert cs.K % cs.blocksize == 0 and bpr > 1
    fin = R.finite_scales()
    held = int(torch.isfinite(fin.to(cs.dtype).float()).sum())
    share = 0.0 if fin.numel() - held < 16 else (fin.numel() - held) / fin.numel()
    return torch.arange(bpr) >= bpr - max(1, int(round(bpr * share)))


def absmax_code_table() -> torch.Tensor:
    """[256] fp32: the caller-supplied second-level code: fixed-seed values of (-1, 1) with full mantissas, and 0, -1, 2^-20 and 1."""
    gen = torch.Generator().manual_seed(P.PROBE_SEED + 256)
    t = torch.rand(256, generator=gen, dtype=torch.float32) * 2 - 1
    t[0], t[1], t[2], t[255] = 0.0, -1.0, 2.0 ** -20, 1.0
    return t


@dataclass
class ScaleProbe:
    case: ProbeCase
    bytes: torch.Tensor                 # uint8 [R, K / 2]
    packed: torch.Tensor                # uint8 [R K / 2, 1]
    code16: torch.Tensor                # [16] fp32
    scale: torch.Tensor                 # fp32 [blocks]: the scale the kernel must reconstruct for every block of the flat tensor
    absmax: torch.Tensor                # what the op takes as absmax (plain: scale; nested: absmax2 per 256 blocks)
    absmax_8bit: Optional[torch.Tensor] = None
    absmax_code: Optional[torch.Tensor] = None
    offset: Optional[torch.Tensor] = None

    @functools.cached_property
    def nibbles(self) -> torch.Tensor:
        return torch.stack([self.bytes >> 4, self.bytes & 15], dim=2).reshape(self.bytes.shape[0], -1)

    @functools.cached_property
    def code_full(self) -> torch.Tensor:
        """fp32 [R, K]: the code value of every weight."""
        return self.code16[self.nibbles.long()]

    @functools.cached_property
    def scale_full(self) -> torch.Tensor:
        """fp32 [R, K]: the scale of every weight (blocks follow the flat index)."""
        R_, K = self.nibbles.shape
        return self.scale.repeat_interleave(self.case.blocksize)[:R_ * K].view(R_, K)

    def stats_args(self, device="cpu"):
        if not self.case.nested:
            return self.absmax.to(device), None, None, None
        return self.absmax.to(device), self.absmax_8bit.to(device), self.absmax_code.to(device), self.offset.to(device)


def plain_scales(cs: ProbeCase, fill_index: int = 0) -> torch.Tensor:
    """fp32 [blocks]. The finite scales of scale_range_cases.scales() in two classes - those T holds (T(s) finite: a family that rounds
    code * scale to T keeps finite weights) in front, the others behind, so that a weight row is of one class - and inside a class by
    a stride coprime to its size: neighbouring blocks are ~97 exponents apart. Then the dedicated non-finite rows."""
    R_, K, bs = cs.weight_rows, cs.K, cs.blocksize
    blocks = -((R_ * K) // -bs)
    fin = R.finite_scales()
    small = torch.isfinite(fin.to(cs.dtype).float())
    # (bf16: one scale, 2^128 - 2^104, whose weights overflow; it poisons the few rows it falls in - in the fused backward it would
    # poison k columns for every probe row, so there it stays a class of its own and fills the poisoned block column)
    if int((~small).sum()) < 16 and cs.family != "grad_input":
        small = torch.ones_like(small)
    classes = [fin[small], fin[~small]]
    dedicated = {}
    for row, (where, value) in nonfinite_rows(cs).items():
        first, last = (row * K) // bs, ((row + 1) * K - 1) // bs
        dedicated[{"first": first, "middle": (first + last) // 2, "last": last}[where]] = value
    free = torch.ones(blocks, dtype=torch.bool)
    free[list(dedicated)] = False
    nfree = int(free.sum())
    # (the class T does not hold gets its share of the blocks, and at least what it needs to be covered by the case's fills)
    n1 = 0 if classes[1].numel() == 0 else max(int(round(nfree * classes[1].numel() / fin.numel())), -(classes[1].numel() // -cs.fills))
    if cs.family == "grad_input":
        # the backward contracts over the weight ROWS: the dedicated blocks and the class T does not hold take whole block columns,
        # the last ones; where T holds every scale, the rest of the poisoned column repeats scales (they are not counted)
        large = poison_columns(cs)[torch.arange(blocks) % (K // bs)]
        if not n1:
            classes[1] = classes[0]
    else:
        large = (torch.cumsum(free, 0) - 1) >= nfree - n1
    out = torch.empty(blocks, dtype=torch.float32)
    for counted, cl, mask in ((True, classes[0], free & ~large), (bool(n1) or cs.family != "grad_input", classes[1], free & large)):
        count = int(mask.sum())
        assert cs.fills * count >= cl.numel() or not counted, "the case's fills do not cover a class of scales"
        if count:
            pos = torch.cumsum(mask, 0)[mask] - 1 + fill_index * count   # the finite scales run over the blocks that are not dedicated
            out[mask] = cl[(pos * _coprime_stride(cl.numel())) % cl.numel()]
    for block, value in dedicated.items():
        out[block] = value
    return out


def nested_absmax2(groups: int, nonfinite: bool = True, within: Optional[torch.dtype] = None) -> torch.Tensor:
    """fp32 [groups]: the 383 second-level scales of scale_range_cases.nested_absmax2() in ascending order, one per group of 256
    blocks; the groups to spare take +inf (the first of them), NaN (the third) and repeats of finite values (``nonfinite`` = False,
    the fused backward: repeats only). ``within`` (the fused backward): a type T; where 16 or more of the second-level scales make
    weights that T does not hold (fp16: 2^15 and up), they are replaced by repeats of the others - such a group turns every k column
    of the backward into NaN, and the call would compare nothing."""
    am2 = R.nested_absmax2()
    if within is not None:
        held = torch.isfinite((2 * am2).to(within).float())
        if int((~held).sum()) >= 16:
            am2 = torch.where(held, am2, am2[held][(17 * torch.arange(am2.numel())) % int(held.sum())])
    assert groups >= am2.numel() + 3, "no group to spare for the non-finite second-level scales"
    spare = am2[(17 * torch.arange(groups - am2.numel())) % am2.numel()].clone()
    if nonfinite:
        spare[0], spare[2] = float("inf"), float("nan")
    return torch.cat([am2, spare])


def build(cs: ProbeCase, fill_index: int = 0, offset: float = 0.0) -> ScaleProbe:
    R_, K, bs = cs.weight_rows, cs.K, cs.blocksize
    assert K % 2 == 0
    by = build_bytes(cs)
    blocks = -((R_ * K) // -bs)
    if cs.nested:
        b = torch.arange(blocks)
        group = b // 256
        q8 = ((b * 77 + group * 13) % 256).to(torch.uint8)          # every code in every group; neighbouring blocks differ
        code2 = absmax_code_table()
        absmax2 = nested_absmax2(-(blocks // -256), nonfinite=cs.family != "grad_input", within=cs.dtype if cs.family == "grad_input" else None)
        off = torch.tensor(offset, dtype=torch.float32)
        scale = code2[q8.long()] * absmax2[group] + off            # two separate fp32 operations: fl32(fl32(c2 * a2) + offset)
        stats = dict(absmax=absmax2, absmax_8bit=q8, absmax_code=code2, offset=off)
    else:
        scale = plain_scales(cs, fill_index)
        stats = dict(absmax=scale)
    return ScaleProbe(cs, by, by.reshape(-1, 1), P.code_table(cs.quant), scale, **stats)


# ------------------------------------------------------------------------------------------ part 1: the wants
def want_forward(pr: ScaleProbe, ks: torch.Tensor, v: torch.Tensor, expert: int = 0, overlay: bool = False):
    """[len(ks), N] in the case's dtype: the family's own order for the one non-zero term, NaN where the row of the weight holds
    ANOTHER term that is non-finite in that order (a zero times inf, or a NaN). Order B16: another weight T(code * scale) that is
    non-finite - an overflow of T included. Order B32: another weight under a non-finite scale. Orders A / A32: a non-finite scale
    outside the probe's own granule (:data:`GRANULE`); inside it the restated order itself gives +-inf (NaN for a zero code).
    ``overlay``: return (want, bool mask of the cells that were overlaid with NaN - they compare nothing of the probe's own term)."""
    cs = pr.case
    order = order_of(cs.family, cs.dtype)
    rows = slice(expert * cs.N, (expert + 1) * cs.N)
    c, s = pr.code_full[rows][:, ks].t(), pr.scale_full[rows][:, ks].t()             # [P, N]
    want = restate(order, c, s, v.float()[:, None], cs.dtype)
    if order == "B16":
        bad = ~torch.isfinite((pr.code_full[rows] * pr.scale_full[rows]).to(cs.dtype).float())   # [N, K]
        own = bad[:, ks]
    else:
        bad = ~torch.isfinite(pr.scale_full[rows])
        g = 1 if order == "B32" else granule(cs.family, cs.blocksize)
        pad = (-cs.K) % g
        per_granule = torch.nn.functional.pad(bad, (0, pad)).view(bad.shape[0], -1, g).sum(dim=2)
        own = per_granule[:, ks // g]
    poisoned = ((bad.sum(dim=1, keepdim=True) - own.long()) > 0).t()
    want = torch.where(poisoned, torch.full_like(want, float("nan")), want)
    return (want, poisoned) if overlay else want


def want_backward(pr: ScaleProbe, ns: torch.Tensor, v: torch.Tensor, overlay: bool = False):
    """[len(ns), K]: row m = v_m * W[n_m, :] in the backward's order (B16); NaN where another weight row's T(code * scale) is
    non-finite in that column. ``overlay``: as want_forward."""
    cs = pr.case
    assert order_of(cs.family, cs.dtype) == "B16"
    want = restate("B16", pr.code_full[ns], pr.scale_full[ns], v.float()[:, None], cs.dtype)
    bad = ~torch.isfinite((pr.code_full * pr.scale_full).to(cs.dtype).float())
    poisoned = (bad.sum(dim=0, keepdim=True) - bad[ns].long()) > 0
    want = torch.where(poisoned, torch.full_like(want, float("nan")), want)
    return (want, poisoned) if overlay else want


def nonfinite_columns(pr: ScaleProbe, expert: int = 0) -> torch.Tensor:
    """Weight rows (output columns of the forward) that hold a block with a non-finite SCALE: non-finite in every probe row (NaN,
    but for the probes of the block itself in a family that scales partial sums: want_forward)."""
    cs = pr.case
    return (~torch.isfinite(pr.scale_full[expert * cs.N:(expert + 1) * cs.N])).any(dim=1)


def experts_probe(cs: ProbeCase, ks: torch.Tensor):
    """decode_probe_cases.experts_probe for a chosen set of k: (x [T, S, K], ids int32 [T, S], v [T, S]), T = len(ks) tokens of
    S = E + 1 slots, every slot of token t probes ks[t], slot s selects expert (t + s) mod S, the value E standing for a masked slot."""
    T, S = ks.numel(), cs.E + 1
    x, v = P.one_hot_rows(ks.repeat_interleave(S), cs.K, cs.dtype)
    sel = (torch.arange(T)[:, None] + torch.arange(S)[None, :]) % S
    ids = torch.where(sel == cs.E, torch.where(torch.arange(T)[:, None] % 2 == 0, -1, cs.E), sel).to(torch.int32)
    return x.view(T, S, cs.K), ids, v.view(T, S)


def experts_want(pr: ScaleProbe, ks: torch.Tensor, ids: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    cs = pr.case
    T, S = ids.shape
    out = torch.zeros(T, S, cs.N, dtype=cs.dtype)
    t = torch.arange(T)
    for e in range(cs.E):
        s = (ids == e).long().argmax(dim=1)
        out[t, s] = want_forward(pr, ks, v[t, s], expert=e)
    return out


def first_mismatch(pr: ScaleProbe, got: torch.Tensor, want: torch.Tensor, probed: torch.Tensor, backward: bool = False, expert=None):
    """decode_probe_cases.first_mismatch under same_bits semantics: NaN against NaN (any payload) passes, either zero passes where a
    zero is wanted, everything else is compared bit for bit."""
    got = torch.where(torch.isnan(got) & torch.isnan(want), want, got)
    return P.first_mismatch(pr, got, want, probed, backward=backward, expert=expert)


def census(want: torch.Tensor) -> str:
    return R.census(want)


# ------------------------------------------------------------------------------------------ parts 2 and 3: dense cases
@dataclass(frozen=True)
class DenseCase:
    family: str
    dtype: torch.dtype
    M: int                      # activation rows (experts: tokens x slots; fused backward: gradient rows)
    N: int
    K: int
    blocksize: int = 64
    knob: int = 0               # forward MFMA families: bnb_mi355x_set_tuning knob1 = 100 * cfg + K slices
    E: int = 1
    plan: str = ""              # fused backward: 'single' or 'sliced'
    nested: bool = False
    k_boundary: int = 0         # a k at which the launch cuts K (a K slice of the forced plan, a segment of the streaming kernel)

    @property
    def name(self) -> str:
        parts = [P.DT_IDS[self.dtype], f"M{self.M}", f"{self.N}x{self.K}", f"bs{self.blocksize}"]
        parts += [f"knob{self.knob}"] if self.knob else []
        parts += [self.plan] if self.plan else []
        parts += ["nested"] if self.nested else []
        return "-".join(parts)

    @property
    def weight_rows(self) -> int:
        return self.E * self.N

    @property
    def split(self) -> bool:
        """The launch goes through a workspace and a finalize launch (K slices of the forward, N slices of the backward)."""
        return self.knob % 100 > 1 or self.plan == "sliced"


def _dense(ms_by_family):
    """One list of dense cases per family: the forced launches of test_gpu_decode_probe.py at small shapes; every family that splits
    its contraction over workgroups (rt, kq, pc: K slices, knob % 100 = 2; the fused backward: plan 'sliced') has such a case."""
    c = {}
    two = lambda fam: ms_by_family[fam]
    for dt in (BF, HF, F32):
        c.setdefault("stream", []).extend(DenseCase("stream", dt, m, N_FWD, 576, k_boundary=256) for m in two("stream"))
        # blocksize 16 (the streaming kernel starts at 32) keeps whole blocks in the 80-wide rows that the generic kernel is reached with
        c.setdefault("generic", []).extend(DenseCase("generic", dt, m, 260, 80, blocksize=16, k_boundary=32) for m in two("generic"))
        c.setdefault("experts", []).extend(DenseCase("experts", dt, m, 272, 576, E=3, k_boundary=256) for m in two("experts"))
    for dt in (BF, HF):
        c.setdefault("sm", []).extend(DenseCase("sm", dt, m, N_FWD, 576, knob=5000, k_boundary=256) for m in two("sm"))
        m0, m1 = two("rt")
        # (the two-slice form of the rt kernel needs 8 chunks of 256 k a slice: K = 4096, with fewer weight rows)
        c.setdefault("rt", []).extend([DenseCase("rt", dt, m0, N_FWD, 512, knob=2001, k_boundary=256),
                                       DenseCase("rt", dt, m1, 528, 4096, knob=2002, k_boundary=2048)])
        c.setdefault("kq", []).extend([DenseCase("kq", dt, m0, N_FWD, 512, knob=4001, k_boundary=256),
                                       DenseCase("kq", dt, m1, N_FWD, 1024, knob=4002, k_boundary=512)])
        c.setdefault("pc", []).extend([DenseCase("pc", dt, m0, N_FWD, 512, knob=1101, k_boundary=256),
                                       DenseCase("pc", dt, m1, N_FWD, 1024, knob=1102, k_boundary=512)])
        c.setdefault("tall", []).extend(DenseCase("tall", dt, m, N_FWD, 512, knob=6000, k_boundary=256) for m in two("tall"))
        c.setdefault("grad_input", []).extend([DenseCase("grad_input", dt, m0, 320, 640, plan="single", k_boundary=128),
                                               DenseCase("grad_input", dt, m1, 320, 640, plan="sliced", k_boundary=128)])
    return c


# rows per call: M chosen so that the family has padded rows (4-row passes of the streaming kernel, 16-row tiles of the MFMA kernels)
DENSE_ROWS = {"stream": (3, 13), "generic": (3, 3), "experts": (12, 12), "sm": (3, 13), "rt": (17, 33), "kq": (17, 33), "pc": (17, 33),
              "tall": (17, 33), "grad_input": (17, 33)}
DENSE = {fam: list(dict.fromkeys(cases)) for fam, cases in _dense(DENSE_ROWS).items()}
ALL_DENSE = tuple(dc for fam in DENSE.values() for dc in fam)
# part 3 also runs nested statistics once per family that serves them at these shapes
NESTED_DENSE = {fam: replace(DENSE[fam][-1], nested=True, dtype=BF) for fam in ("stream", "sm", "rt", "kq", "pc", "tall", "experts", "grad_input")}
# (the fused backward: a second-level scale reaches 256 consecutive blocks, every block column of a row of up to 256 blocks; rows of
# 320 blocks keep 64 block columns clean per poisoned group)
NESTED_DENSE["grad_input"] = DenseCase("grad_input", BF, 33, 320, 20480, plan="sliced", nested=True, k_boundary=128)
NESTED_DENSE["generic"] = None   # nested statistics need blocksize >= 32 x 256 blocks a group: its 80-wide blocksize-16 case has no second group

# ------------------------------------------------------------------------------------------ part 2: windows of exact sums
# (lo, hi) exponents of exact_inputs.build's power-of-two scales. Bottom: the unit 2^(lo - 2) is the smallest subnormal of the type
# (fp32: 2^-149; bf16: 2^-133; fp16: 2^-24), so every weight is a subnormal of the type or just above it and every fp32 partial sum of
# an fp32 case is a subnormal multiple. Top: the sum of the product magnitudes stays below 2^128 (asserted: no fp32 partial sum
# overflows in any order). fp16 (10, 15): float64 rounded once overflows to +-inf for many outputs - the wanted result.
WINDOWS = {
    F32: {"bottom": (-147, -142), "top": (110, 115)},
    BF: {"bottom": (-131, -126), "top": (110, 115)},
    HF: {"bottom": (-22, -17), "top": (4, 9), "top-inf": (10, 15)},
}
FP16_LIFTED = ("top", "top-inf")     # the windows for which assert_exact_sums' "below the largest fp16 value" condition is lifted


@dataclass
class DenseInputs:
    case: DenseCase
    ex: X.ExactInputs               # W [E N, K], x [M, K] (forward), scales, statistics, bias
    packed: torch.Tensor            # uint8 [E N K / 2, 1], packed by hand
    g: Optional[torch.Tensor]       # fused backward: integer gradients [M, N]
    ids: Optional[torch.Tensor]     # experts: int32 [T, S]
    worst: float                    # the bound of assert_exact_sums

    def reference(self, with_bias: bool = False) -> torch.Tensor:
        """float64 product of the constructed operands, rounded once: [M, N] (forward), [M, K] (backward), [T, S, N] (experts)."""
        ex, dc = self.ex, self.case
        if dc.family == "grad_input":
            return (self.g.double() @ ex.W.double()).to(dc.dtype)
        if dc.family != "experts":
            return ex.reference(with_bias)
        T, S = self.ids.shape
        x64, out = ex.x.double().view(T, S, dc.K), torch.zeros(T, S, dc.N, dtype=torch.float64)
        for e in range(dc.E):
            sel = self.ids == e
            y = x64[sel] @ ex.W[e * dc.N:(e + 1) * dc.N].double().t()
            out[sel] = y + ex.bias[e * dc.N:(e + 1) * dc.N].double() if with_bias else y
        return out.to(dc.dtype)


EXPERT_SLOTS = 4


def expert_ids(dc: DenseCase) -> torch.Tensor:
    """int32 [T, S = 4]: slot s of token t selects expert (t + s) mod 4, the value E = 3 standing for a masked slot (-1 / E)."""
    T = dc.M // EXPERT_SLOTS
    sel = (torch.arange(T)[:, None] + torch.arange(EXPERT_SLOTS)[None, :]) % EXPERT_SLOTS
    return torch.where(sel == dc.E, torch.where(torch.arange(T)[:, None] % 2 == 0, -1, dc.E), sel).to(torch.int32)


def pack_exact(ex: X.ExactInputs) -> torch.Tensor:
    """uint8 [N K / 2, 1]: the FP4 nibbles of ``ex.W`` packed by hand (the quantizer is not the subject here, and the reference's
    rule clamps an absmax below 1e-38)."""
    s = ex.scale.double().view(ex.N, -1).repeat_interleave(ex.blocksize, dim=1)
    code = ex.W.double() / s
    idx = torch.full(code.shape, -1, dtype=torch.long)
    for value, index in zip(X.FP4_EXACT_VALUES, X.FP4_EXACT_INDICES):
        idx[code == value] = index
    assert bool((idx >= 0).all()), "a weight is not one of the exact FP4 codes times its block's scale"
    flat = idx.reshape(-1)
    return ((flat[0::2] << 4) | flat[1::2]).to(torch.uint8).reshape(-1, 1)


def _dense_inputs(dc: DenseCase, exps, lifted: bool, bias_max: int) -> DenseInputs:
    seed = (dc.N * 31 + dc.K * 7 + dc.blocksize + dc.M + exps[0] * 1009) % (1 << 31)
    ex = X.build(dc.weight_rows, dc.K, dc.blocksize, dc.dtype, dc.nested, seed, dc.M, exps=exps, bias_max=bias_max, allow_fp16_overflow=lifted)
    g = ids = None
    worst = X.assert_exact_sums(ex.W, ex.x, ex.unit, dc.dtype, extra=float(bias_max), allow_fp16_overflow=lifted)
    if dc.family == "grad_input":
        g = X.int_rows(dc.M, dc.N, dc.dtype, torch.Generator().manual_seed(seed + 1))
        worst = X.assert_exact_sums(ex.W, g, ex.unit, dc.dtype, transposed=True, allow_fp16_overflow=lifted)
    if dc.family == "experts":
        ids = expert_ids(dc)
    return DenseInputs(dc, ex, pack_exact(ex), g, ids, worst)


@functools.lru_cache(maxsize=None)
def window_inputs(dc: DenseCase, window: str) -> DenseInputs:
    """exact_inputs.build at a window of :data:`WINDOWS`, without a bias (an integer is no multiple of the unit at the bottom and
    vanishes below the unit at the top). The exact-sum bound is asserted with the fp16 condition lifted where the window calls for
    it, and the no-overflow bound is asserted: the sum of the product magnitudes of the worst output is below 2^128."""
    lifted = dc.dtype == HF and window in FP16_LIFTED
    di = _dense_inputs(dc, WINDOWS[dc.dtype][window], lifted, bias_max=0)
    assert di.worst < 2.0 ** 128, f"{dc.name} {window}: sum of |products| {di.worst} reaches 2^128: an fp32 partial sum may overflow"
    return di


def orders_agree(ex: X.ExactInputs) -> bool:
    """Every order of :data:`ORDER` gives every product x * W[n, k] of the case the same fp32 value, the exact one (so the sums, exact
    in any order of summation under assert_exact_sums' bound, are the same in every family; an order that scales a block's partial
    sum multiplies a multiple of the unit below 2^24 units by a power of two: exact as well). Checked over the distinct triples."""
    c = torch.tensor(X.FP4_EXACT_VALUES, dtype=torch.float32)[:, None, None]
    s = torch.unique(ex.scale)[None, :, None]
    v = torch.arange(-X.X_MAX, X.X_MAX + 1, dtype=torch.float32)[None, None, :]
    exact = c.double() * s.double() * v.double()
    products = {"A": (c.to(ex.dtype).float() * v) * s, "A32": (c * v) * s, "B16": (c * s).to(ex.dtype).float() * v}
    if ex.dtype == F32:
        products["B32"] = (c * s) * v
    return all(torch.equal(p.double(), exact) for p in products.values())


# ------------------------------------------------------------------------------------------ part 3: one non-finite operand per call
@functools.lru_cache(maxsize=None)
def clean_inputs(dc: DenseCase) -> DenseInputs:
    """The clean dense case of part 3: the ordinary window of tests/exact_inputs.py, with its integer bias."""
    return _dense_inputs(dc, P.PLAIN_EXPS[dc.dtype], False, bias_max=X.BIAS_MAX)


def poison_blocks(dc: DenseCase) -> dict:
    """name -> flat block index: the first and the last block of a row, the last block of the matrix, a block on either side of the
    case's K cut and a block in a row of the ragged last N tile (the last row but one: N = 1040, 528, 272 and 260 are ragged against
    every tile height)."""
    bpr = dc.K // dc.blocksize
    R_ = dc.weight_rows
    row = R_ // 3
    kb = dc.k_boundary // dc.blocksize
    assert 0 < kb < bpr
    return {"first-of-row": row * bpr, "last-of-row": row * bpr + bpr - 1, "last-of-matrix": R_ * bpr - 1,
            "before-k-cut": (row + 1) * bpr + kb - 1, "after-k-cut": (row + 2) * bpr + kb, "ragged-tile": (R_ - 2) * bpr + bpr // 2}


def poison_activations(dc: DenseCase) -> list:
    """(m, k, value): m the first row, the last row and a row of the second row pass where M has one (row 5 of the streaming kernel's
    4-row passes, row 16 of the 16-row tiles) x k in the first segment, behind the middle of the row (its last whole segment, the
    second K slice) and the last k (the tail); +inf, -inf and NaN in turn.
    The fused backward reads it as g[m, n]: n in the first 32-row block, the last one and the last row."""
    width = dc.N if dc.family == "grad_input" else dc.K
    ms = sorted({0, dc.M - 1} | ({5} if dc.M > 5 else set()) | ({16} if dc.M > 16 else set()))
    cols = sorted({3, width // 2 + 5, width - 1})
    values = (float("inf"), float("-inf"), float("nan"))
    return [(m, c, values[(i + j) % 3]) for i, m in enumerate(ms) for j, c in enumerate(cols)]


def rows_of_blocks(dc: DenseCase, blocks: torch.Tensor) -> torch.Tensor:
    """Weight rows that hold one of ``blocks`` (flat indices; K % blocksize == 0)."""
    return torch.unique(blocks // (dc.K // dc.blocksize))
