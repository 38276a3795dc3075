"""Builders shared by tests/test_decode_probe_host.py (CPU) and tests/test_gpu_decode_probe.py (GPU): a matmul that reads a packed
weight out BIT FOR BIT, for any code table, through the decode table of every fused 4-bit kernel. Pure torch on the CPU.

Every fused kernel turns a packed byte into the pair ``(code[hi], code[lo])`` through a table it builds in LDS (32 or 64 bank- or
lane-private copies, :data:`COPIES`). The exact suites (tests/exact_inputs.py) reach 49 of its 256 entries and no NF4 entry; everything
else is judged by a whole-matrix norm. The operands built here need no tolerance:

* activations (for the backward: gradients) whose rows are ONE-HOT (:func:`one_hot_rows`): row ``m`` is zero except
  ``x[m, k_m] = v_m``, a signed power of two. ``y[m, n] = v_m * W[n, k_m]`` has a single non-zero term: exact in any order, over any K
  split, through any slab reduction.
* weights packed by hand (no quantizer: no 1.0 is needed in a block): byte ``(n, j)`` is a fixed-seed pseudo-random function of the
  position, or ``(n + j) mod 256`` (the structured fill: a failure names its position). All 256 byte values occur in every case.
* a power-of-two scale per quantization block, different in neighbouring blocks of a row (the ``col_parity`` rule of
  tests/exact_inputs.py). Nested statistics are the case's own: ``absmax_code`` holds ``NESTED_TARGETS`` and their halves, ``absmax2``
  alternates between 1 and 2 from one group of 256 blocks to the next, so that ``code2[q] * absmax2 + offset`` is a power of two with
  every step exact in fp32; a block that took its neighbour group's absmax2 or another table entry gets another scale.
* the only correct answer (:func:`Probe.want_forward`): ``round_T(code[nibble(n, k_m)] * s(n, k_m) * v_m)``, float64, rounded once. It
  is the answer of every form a kernel may use - decode to T then scale in fp32, scale then round to T, all fp32 - because
  ``round_T(round_T(code) * s * v) == round_T(code * s * v)`` for a power of two ``s * v`` and a normal result; that condition is
  asserted for every (code, scale, v) a case uses (:func:`assert_rounding_precondition`), not assumed.
* the comparison (:func:`mismatches`): equal integer views; where the want is zero either sign of zero passes (FP4 nibbles 0 and 8 are
  both zeros, and the reference's own paths disagree on the sign: conftest.same_values). :func:`first_mismatch` names n, k, the byte,
  the nibble, the code index, got and want.
* coverage is a condition on the inputs (:func:`expected_reads_per_cell`): under a uniform model every (copy, entry) cell of the
  family's table is read at least :data:`READS_FLOOR` times; where one fill of the stated shape does not give that, the case runs
  several fills (other seeds).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import torch

NF4_CODE = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
            -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
            0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
FP4_TWELFTHS = (0.0, 0.0625, 8.0, 12.0, 4.0, 6.0, 2.0, 3.0, 0.0, -0.0625, -8.0, -12.0, -4.0, -6.0, -2.0, -3.0)  # x / 12 in fp32
V_CYCLE = (1.0, -1.0, 2.0, -0.5, 4.0, -2.0, 0.5, -4.0)
PLAIN_EXPS = {torch.bfloat16: (-2, 3), torch.float16: (-2, 1), torch.float32: (-2, 3)}   # as tests/exact_inputs.py
NESTED_TARGETS = (0.375, 0.875, 1.875, 3.875)      # + NESTED_OFFSET = 0.5, 1, 2, 4
NESTED_OFFSET = 0.125
NESTED_ABSMAX2 = (1.0, 2.0)                         # absmax2 of group g = NESTED_ABSMAX2[g % 2]
READS_FLOOR = 16
PROBE_SEED = 20250117
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
DT_IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
# copies of the 256-entry table each kernel keeps (csrc/*.hip: kLutBytes / kRtLut / kKqLut / kSmLut / kTallLut / kGiLut and the
# producer/consumer kernel's 256 * 32 * 4): the cells the reads of a case spread over
COPIES = {"stream": 32, "pc": 32, "rt": 32, "kq": 64, "sm": 64, "tall": 32, "experts": 32, "grad_input": 32}
# kernel families as bnb_mi355x_last_gemm_kernel() reports them (include/bnb_mi355x.h); the fused backward reports none
FAMILY_ID = {"stream": 1, "rt": 3, "pc": 4, "kq": 6, "sm": 7, "tall": 8, "experts": 9}


@functools.lru_cache(maxsize=None)
def code_table(quant: str) -> torch.Tensor:
    """[16] fp32: the NF4 / FP4 code values (the host test holds them to the oracle's, bit for bit); 'code16': sixteen arbitrary fp32
    values of a caller-supplied table - distinct, normal, of mixed sign and magnitude."""
    if quant == "nf4":
        return torch.tensor(NF4_CODE, dtype=torch.float32)
    if quant == "fp4":
        return torch.tensor(FP4_TWELFTHS, dtype=torch.float32) / torch.tensor(12.0, dtype=torch.float32)
    assert quant == "code16"
    gen = torch.Generator().manual_seed(PROBE_SEED + 16)
    t = torch.randn(16, generator=gen, dtype=torch.float32) * torch.pow(torch.tensor(2.0), torch.randint(-6, 7, (16,), generator=gen).float())
    assert torch.unique(t).numel() == 16 and bool((t.abs() > 2.0 ** -20).all())
    return t


# ------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class ProbeCase:
    family: str                 # a key of COPIES
    dtype: torch.dtype
    quant: str                  # 'nf4', 'fp4' or 'code16' (NF4 bytes decoded through a caller-supplied table)
    blocksize: int
    nested: bool
    N: int
    K: int
    fill: str = "random"        # or 'structured'
    knob: int = 0               # forward MFMA families: bnb_mi355x_set_tuning knob1 = 100 * cfg + K slices
    rows: int = 0               # probe rows per call; 0 = all of them in one call
    E: int = 1                  # experts
    plan: str = ""              # fused backward: 'single' or 'sliced'
    fills: int = 1              # random fills (seeds) the case runs: see expected_reads_per_cell

    @property
    def name(self) -> str:
        parts = [DT_IDS[self.dtype], self.quant, f"bs{self.blocksize}", "nested" if self.nested else "plain", f"{self.N}x{self.K}"]
        if self.knob:
            parts.append(f"knob{self.knob}")
        if self.rows:
            parts.append(f"rows{self.rows}")
        if self.plan:
            parts.append(self.plan)
        if self.fill != "random":
            parts.append(self.fill)
        return "-".join(parts)

    @property
    def weight_rows(self) -> int:
        return self.E * self.N


BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
N_FWD = 1040   # ragged against 16-, 32-, 64- and 128-row tiles: the last tile of every family is partial


def _fwd(family, K, combos, **kw):
    return [ProbeCase(family, dt, qt, bs, nested, N_FWD, K, **kw) for (dt, qt, bs, nested) in combos]


def _cases():
    c = {}
    # streaming kernel: K = two 256-k segments and a 64-k remainder; M = 1 per call (the decode instance) and all rows in one call
    # (the 4-row passes); blocksize 128 and 4096 do not divide K: a block spans rows
    stream = [(BF, "nf4", 64, False), (BF, "fp4", 64, True), (HF, "fp4", 64, False), (HF, "nf4", 64, True), (F32, "nf4", 64, False),
              (F32, "fp4", 64, True), (BF, "fp4", 32, False), (HF, "nf4", 32, False), (BF, "nf4", 128, True), (HF, "fp4", 128, True),
              (BF, "nf4", 4096, False), (F32, "fp4", 4096, False), (F32, "code16", 32, False)]
    c["stream"] = (_fwd("stream", 576, stream, rows=1) + _fwd("stream", 576, stream[:4] + stream[-1:]) +
                   _fwd("stream", 576, stream[:1], fill="structured"))
    # streaming MFMA kernel: 16 rows per call; blocksize 1024 does not divide K
    sm = [(BF, "nf4", 64, False), (BF, "fp4", 64, True), (HF, "fp4", 64, False), (HF, "nf4", 64, True), (BF, "nf4", 1024, False)]
    c["sm"] = _fwd("sm", 576, sm, knob=5000, rows=16) + _fwd("sm", 576, sm[1:2], knob=5000, rows=16, fill="structured")
    # register-transposed kernel: as sm, plus the blocksize-32 instances (plain statistics); one call of K rows (row passes of 64), one
    # case of 8 rows per call (directly loaded activation fragments); K slices need 8 chunks each: K = 4096 for the two-slice form
    # (blocksize 64: the blocksize-32 instances take no forced slice count)
    rt = sm + [(BF, "nf4", 32, False), (HF, "fp4", 32, False)]
    c["rt"] = (_fwd("rt", 512, rt, knob=2001) + _fwd("rt", 512, rt[:1], knob=2001, rows=8) + _fwd("rt", 4096, rt[:2], knob=2002) +
               _fwd("rt", 512, rt[2:3], knob=2001, fill="structured"))
    # K-quarter kernel: nested statistics at blocksize 64 only (gemm_4bit_kq_serves); K slices need two chunks each: K = 1024
    kq = [(BF, "nf4", 64, False), (BF, "fp4", 64, True), (HF, "fp4", 64, False), (HF, "nf4", 64, True), (HF, "nf4", 256, False)]
    c["kq"] = _fwd("kq", 512, kq, knob=4001) + _fwd("kq", 1024, kq[:2], knob=4002) + _fwd("kq", 512, kq[3:4], knob=4001, fill="structured")
    # producer/consumer kernel: the four geometries 11 - 14, each at another row-tile count (64-, 48-, 32- and 16-row calls: geometry
    # 13 exists up to 32 rows); two K slices need two chunks each: K = 1024
    pc = []
    for cfg, rows, combo in ((11, 0, (BF, "nf4", 64, False)), (12, 48, (HF, "fp4", 64, True)), (13, 32, (BF, "fp4", 128, True)),
                             (14, 16, (HF, "nf4", 256, False))):
        pc += _fwd("pc", 512, [combo], knob=cfg * 100 + 1, rows=rows) + _fwd("pc", 1024, [combo], knob=cfg * 100 + 2, rows=rows)
    c["pc"] = pc + _fwd("pc", 512, [(BF, "nf4", 64, True)], knob=1101, fill="structured")
    # tall-tile kernel (knob cfg 60): the forced MFMA request is honoured for whole 256-k chunks only, so K = 512
    tall = [(BF, "nf4", 64, False), (BF, "fp4", 64, True), (HF, "fp4", 128, False), (HF, "nf4", 64, True)]
    c["tall"] = _fwd("tall", 512, tall, knob=6000) + _fwd("tall", 512, tall[:1], knob=6000, fill="structured")
    # experts kernel: E = 3 experts of [272, 576], one probe row per slot
    ex = [(dt, qt, bs, nested) for dt in (BF, HF, F32) for qt in ("nf4", "fp4") for bs in (32, 64) for nested in (False, True)]
    c["experts"] = ([ProbeCase("experts", dt, qt, bs, nested, 272, 576, E=3) for (dt, qt, bs, nested) in ex] +
                    [ProbeCase("experts", BF, "fp4", 64, False, 272, 576, E=3, fill="structured")])
    # fused backward: one-hot gradient rows return whole weight rows; N = 5 kGiNAlign, K = 5 kGiCols, M = N; two fills for the floor
    gi = [(dt, qt, bs, nested) for dt in (BF, HF) for qt in ("nf4", "fp4") for (bs, nested) in ((64, False), (64, True), (256, False))]
    c["grad_input"] = ([ProbeCase("grad_input", dt, qt, bs, nested, 320, 640, plan=plan, fills=2) for (dt, qt, bs, nested) in gi
                        for plan in ("single", "sliced")] +
                       [ProbeCase("grad_input", BF, "nf4", 64, False, 320, 640, plan="single", fill="structured", fills=1)])
    return c


CASES = _cases()
ALL_CASES = tuple(cs for fam in CASES.values() for cs in fam)


def expected_reads_per_cell(cs: ProbeCase) -> float:
    """Bytes a full probe of the case decodes and checks, over the cells (copies x 256 entries) of the family's table: what every
    cell is read under a uniform model. (Each byte counts once, though both of its nibbles are checked.)"""
    fills = cs.fills if cs.fill == "random" else 1
    return fills * cs.weight_rows * (cs.K // 2) / (256.0 * COPIES[cs.family])


# ------------------------------------------------------------------------------------------ bytes, scales, nested state
def build_bytes(cs: ProbeCase, fill_index: int = 0) -> torch.Tensor:
    """uint8 [weight rows, K / 2]: byte (n, j) = (code[n, 2 j] << 4) | code[n, 2 j + 1]."""
    R, J = cs.weight_rows, cs.K // 2
    if cs.fill == "structured":
        b = ((torch.arange(R)[:, None] + torch.arange(J)[None, :]) % 256).to(torch.uint8)
    else:
        gen = torch.Generator().manual_seed(PROBE_SEED + 7919 * fill_index + 31 * R + J)
        b = torch.randint(0, 256, (R, J), generator=gen, dtype=torch.uint8)
    assert torch.bincount(b.reshape(-1).long(), minlength=256).min() > 0, "a byte value does not occur"
    return b


@dataclass
class Probe:
    case: ProbeCase
    bytes: torch.Tensor                 # uint8 [R, K / 2]
    packed: torch.Tensor                # uint8 [R K / 2, 1]: what the ops take
    code16: torch.Tensor                # [16] fp32
    scale: torch.Tensor                 # fp32 [blocks]: the intended scale of every block of the flat tensor
    absmax: torch.Tensor                # what the op takes as absmax (plain: scale; nested: absmax2 per 256 blocks)
    absmax_8bit: Optional[torch.Tensor] = None
    absmax_code: Optional[torch.Tensor] = None
    offset: Optional[torch.Tensor] = None

    @functools.cached_property
    def nibbles(self) -> torch.Tensor:
        """uint8 [R, K]: the code index of every weight."""
        return torch.stack([self.bytes >> 4, self.bytes & 15], dim=2).reshape(self.bytes.shape[0], -1)

    @functools.cached_property
    def W64(self) -> torch.Tensor:
        """float64 [R, K]: code[nibble] * scale - exact (a 24-bit code times a power of two), an fp32 value."""
        R, K = self.nibbles.shape
        s = self.scale.double().repeat_interleave(self.case.blocksize)[:R * K].view(R, K)
        w = self.code16.double()[self.nibbles.long()] * s
        assert torch.equal(w.float().double(), w), "code x scale is not an fp32 value"
        return w

    def want_forward(self, ks: torch.Tensor, v: torch.Tensor, expert: int = 0) -> torch.Tensor:
        """[len(ks), N] in the case's dtype: ``round_T(code[nibble(n, k_m)] * s(n, k_m) * v_m)``."""
        N = self.case.N
        w = self.W64[expert * N:(expert + 1) * N].t()[ks] * v.double()[:, None]
        assert torch.equal(w.float().double(), w)       # (so the conversion below rounds once, from fp32)
        return w.float().to(self.case.dtype)

    def want_backward(self, ns: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """[len(ns), K]: ``round_T(v_m * W[n_m, :])``."""
        w = self.W64[ns] * v.double()[:, None]
        assert torch.equal(w.float().double(), w)
        return w.float().to(self.case.dtype)

    def stats_args(self, device="cpu"):
        """(absmax, absmax_8bit, absmax_code, absmax_offset) as the gemm_4bit ops take them."""
        if not self.case.nested:
            return self.absmax.to(device), None, None, None
        return self.absmax.to(device), self.absmax_8bit.to(device), self.absmax_code.to(device), self.offset.to(device)


def nested_code_table() -> torch.Tensor:
    """[256] fp32: entry i holds NESTED_TARGETS[j] (j = i % 8 < 4: for groups whose absmax2 is 1) or NESTED_TARGETS[j - 4] / 2."""
    j = torch.arange(256) % 8
    t = torch.tensor(NESTED_TARGETS, dtype=torch.float32)
    return torch.where(j < 4, t[j % 4], t[j % 4] / 2)


def build(cs: ProbeCase, fill_index: int = 0) -> Probe:
    R, K, bs = cs.weight_rows, cs.K, cs.blocksize
    assert K % 2 == 0 and (R * K) % 2 == 0
    by = build_bytes(cs, fill_index)
    blocks = -((R * K) // -bs)
    gen = torch.Generator().manual_seed(PROBE_SEED + 1 + fill_index + bs + K)
    b = torch.arange(blocks)
    # neighbouring blocks of a row differ in parity, so in scale; a block that spans rows (K % blocksize != 0) follows the flat index
    parity = ((b % (K // bs)) & 1) if K % bs == 0 else (b & 1)
    if cs.nested:
        sel = (2 * torch.randint(0, 2, (blocks,), generator=gen) + parity) % 4
        group = b // 256
        q8 = (sel + 4 * (group % 2) + 8 * torch.randint(0, 32, (blocks,), generator=gen)).to(torch.uint8)
        code2 = nested_code_table()
        absmax2 = torch.tensor([NESTED_ABSMAX2[g % 2] for g in range(-(blocks // -256))], dtype=torch.float32)
        offset = torch.tensor(NESTED_OFFSET, dtype=torch.float32)
        prod = code2[q8.long()] * absmax2[group]
        scale = prod + offset
        # each step exact in fp32: the products are the targets (<= 5 significant bits), the sums powers of two
        assert torch.equal(prod.double(), code2[q8.long()].double() * absmax2[group].double())
        assert torch.equal(scale.double(), prod.double() + NESTED_OFFSET)
        stats = dict(absmax=absmax2, absmax_8bit=q8, absmax_code=code2, offset=offset)
    else:
        lo, hi = PLAIN_EXPS[cs.dtype]
        span = hi - lo + 1
        assert span % 2 == 0
        e = lo + (2 * torch.randint(0, span // 2, (blocks,), generator=gen) + parity) % span
        scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).float()
        stats = dict(absmax=scale)
    m, ex = torch.frexp(scale)
    assert bool((m == 0.5).all()), "a scale is not a power of two"
    if K % bs == 0 and K // bs > 1:
        s2 = scale[:R * (K // bs)].view(R, K // bs)
        assert bool((s2[:, 1:] != s2[:, :-1]).all()), "neighbouring blocks of a row share a scale"
    return Probe(cs, by, by.reshape(-1, 1), code_table(cs.quant), scale, **stats)


def op_quant_type(cs: ProbeCase) -> str:
    """The quant_type string an op is called with (a caller-supplied table rides on an NF4 call)."""
    return "nf4" if cs.quant == "code16" else cs.quant


# ------------------------------------------------------------------------------------------ probe rows
def one_hot_rows(ks: torch.Tensor, width: int, dtype: torch.dtype):
    """(x [len(ks), width] in ``dtype``, v [len(ks)] float64): row m is zero except ``x[m, ks[m]] = v_m``, v cycling through V_CYCLE."""
    ks = torch.as_tensor(ks, dtype=torch.int64)
    v = torch.tensor(V_CYCLE, dtype=torch.float64)[torch.arange(ks.numel()) % len(V_CYCLE)]
    x = torch.zeros(ks.numel(), width, dtype=dtype)
    x[torch.arange(ks.numel()), ks] = v.to(dtype)
    assert torch.equal(x.double().sum(dim=1), v) and int((x != 0).sum()) == ks.numel()
    return x, v


def experts_probe(cs: ProbeCase):
    """(x [T, S, K], ids int32 [T, S], v [T, S] float64): T = K tokens of S = E + 1 slots; every slot of token t probes k = t; slot s
    selects expert (t + s) mod (E + 1), the value E standing for a masked slot - an id of -1 for even t, of E for odd t. Every expert is
    probed at every k, and every token carries one masked slot."""
    T, S = cs.K, cs.E + 1
    x, v = one_hot_rows(torch.arange(T).repeat_interleave(S), cs.K, cs.dtype)
    sel = (torch.arange(T)[:, None] + torch.arange(S)[None, :]) % S
    ids = torch.where(sel == cs.E, torch.where(torch.arange(T)[:, None] % 2 == 0, -1, cs.E), sel).to(torch.int32)
    for e in range(cs.E):
        assert bool(((ids == e).sum(dim=1) == 1).all())
    assert bool((((ids < 0) | (ids >= cs.E)).sum(dim=1) == 1).all())
    return x.view(T, S, cs.K), ids, v.view(T, S)


def experts_want(pr: Probe, ids: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    cs = pr.case
    T, S = ids.shape
    out = torch.zeros(T, S, cs.N, dtype=cs.dtype)
    t = torch.arange(T)
    for e in range(cs.E):
        s = (ids == e).long().argmax(dim=1)
        out[t, s] = pr.want_forward(t, v[t, s], expert=e)
    return out


def host_sample(n: int, chunk: int = 64, count: int = 40) -> torch.Tensor:
    """A subsample of the probe rows for the scalar oracle: both ends of the row and a stride that visits every residue of 8."""
    step = max(1, n // count) | 1
    return torch.unique(torch.cat([torch.arange(0, min(8, n)), torch.arange(max(0, n - 8), n), torch.arange(0, n, step)]))


# ------------------------------------------------------------------------------------------ preconditions and comparison
def assert_rounding_precondition(code16: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype) -> int:
    """For every one of the 16 codes, every scale of ``scales`` and every v of V_CYCLE: ``round_T(round_T(code) * s * v)`` equals
    ``round_T(code * s * v)`` (so decoding to T first, scaling first or staying in fp32 all give the want), and the result is zero or
    a NORMAL number of T. Returns the number of triples checked."""
    c = code16.double()[:, None, None]
    s = torch.unique(scales).double()[None, :, None]
    v = torch.tensor(V_CYCLE, dtype=torch.float64)[None, None, :]
    exact = c * s * v
    assert torch.equal(exact.float().double(), exact)
    once = exact.float().to(dtype)
    pre = (code16.to(dtype).double()[:, None, None] * s * v)
    assert torch.equal(pre.float().double(), pre)
    twice = pre.float().to(dtype)
    assert torch.equal(once.view(INT_VIEW[dtype]), twice.view(INT_VIEW[dtype])), "rounding the code first changes the result"
    mag = once.double().abs()
    fi = torch.finfo(dtype)
    assert bool(((mag == 0) | ((mag >= fi.tiny) & (mag <= fi.max))).all()), "a result is not a normal number of T"
    assert bool(((exact == 0) == (once.double() == 0)).all()), "a non-zero product rounds to zero"
    return exact.numel()


def mismatches(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Mask of the elements that differ: integer views must be equal, except that where the want is zero either zero passes."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    iv = INT_VIEW[got.dtype]
    both_zero = (want == 0) & (got == 0)
    return (got.contiguous().view(iv) != want.contiguous().view(iv)) & ~both_zero


def first_mismatch(pr: Probe, got: torch.Tensor, want: torch.Tensor, probed: torch.Tensor, backward: bool = False, expert=None):
    """None, or a description of the first differing element of a [rows, N] result (forward: row m probes k = probed[m]; expert: the
    expert of every row) or a [rows, K] result (backward: row m probes weight row probed[m])."""
    bad = mismatches(got, want).nonzero()
    if bad.numel() == 0:
        return None
    r, c = int(bad[0, 0]), int(bad[0, 1])
    n, k = (int(probed[r]), c) if backward else (c, int(probed[r]))
    row = n + (int(expert[r]) * pr.case.N if expert is not None else 0)
    byte = int(pr.bytes[row, k // 2])
    half = "hi" if k % 2 == 0 else "lo"
    idx = byte >> 4 if k % 2 == 0 else byte & 15
    block = (row * pr.case.K + k) // pr.case.blocksize
    return Mismatch(int(bad.shape[0]), r, n, k, int(expert[r]) if expert is not None else None, byte, half, idx, float(pr.code16[idx]),
                    float(pr.scale[block]), float(got[r, c]), float(want[r, c]))


@dataclass(frozen=True)
class Mismatch:
    count: int
    row: int
    n: int
    k: int
    expert: Optional[int]
    byte: int
    nibble: str
    index: int
    code: float
    scale: float
    got: float
    want: float

    def __str__(self) -> str:
        return (f"{self.count} mismatches; first at probe row {self.row}: n={self.n} k={self.k}" +
                (f" expert={self.expert}" if self.expert is not None else "") +
                f" byte=0x{self.byte:02x} nibble={self.nibble} code index={self.index} (code {self.code!r}, scale {self.scale!r}) "
                f"got={self.got!r} want={self.want!r}")
