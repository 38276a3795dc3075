"""Exact operands for weights past the 2^31 and 2^32 ELEMENT offsets, built in place on any device.

``quantize_4bit`` stops at 2^31 - 1 elements, so nothing here is quantized: the packed bytes and the statistics are WRITTEN, with the
construction of tests/exact_inputs.py restated in plain torch (tests/test_large_offsets_host.py holds the two against each other):

* weights: FP4 nibble indices from ``FP4_EXACT_INDICES`` (codes 0, +-1, +-0.5, +-0.25), index 3 (code 1.0) at the head of every
  quantization block, element 2 i of the flat tensor in the HIGH nibble of byte i;
* plain statistics: one power-of-two scale per block. Neighbouring blocks of a row never share a scale (the column-parity rule of
  ``exact_inputs.build``), and the pattern is seeded from a hash of the BLOCK INDEX, so it does NOT repeat with any power-of-two
  period - in particular not with 2^32 / blocksize blocks, the distance by which a block index computed in 32 bits from an element
  index lands short. A kernel that wraps such an index reads bytes of the right row and the scale of a row at the start of the
  tensor: wrong, finite, and visible only because the two scales differ. :func:`assert_not_periodic` asserts it: no power-of-two
  shift maps the pattern onto itself, and every row past the wrap has a block whose scale differs from the one 2^32 / blocksize
  blocks before it;
* nested statistics: ``NESTED_TABLE`` / ``NESTED_ABSMAX2_EXP`` / ``NESTED_OFFSET`` of exact_inputs; the table entry of a block and the
  absmax2 of a group of 256 blocks come from the same hash (the even groups draw 2^-1 or 2^1, the odd ones hold 2^0: neighbours differ);
* activations: integers of magnitude <= 4, every row different; an integer bias;
* reference: by rows in chunks with nothing of this project's in it - table look-up of the two nibbles, times the constructed scale,
  in float64; the chunk times ``x.double().t()``, plus the bias, rounded ONCE to the output dtype. Computed once per case for
  ``REF_ROWS`` activation rows, kept on the device, sliced per M. The exact-sum bound of ``exact_inputs.assert_exact_sums`` is asserted
  on the way (K = 8192: products are multiples of 2^-4 and their magnitudes sum to at most 2^18 = 2^22 units), so every fp32 partial sum
  in any order is exact and the comparison is bit for bit on the WHOLE output.

Everything is built in pieces of at most ``PIECE`` = 2^27 elements with uint8 draws: no int64 temporary of a whole tensor.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import torch

import exact_inputs as X

PIECE = 1 << 27
REF_ROWS = 64
MS = (1, 2, 4, 8, 16, 17, 64)
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
EXPS = {torch.bfloat16: (-2, 3), torch.float16: (-2, 1)}

# FP4 code value of a nibble index; the indices the construction never writes are NaN, so a wrong nibble cannot pass for data
_FP4 = [float("nan")] * 16
for _i, _v in zip(X.FP4_EXACT_INDICES, X.FP4_EXACT_VALUES):
    _FP4[_i] = _v
FP4_TABLE = tuple(_FP4)


@dataclass(frozen=True)
class LargeCase:
    name: str
    N: int
    K: int
    blocksize: int = 64

    @property
    def elements(self) -> int:
        return self.N * self.K

    @property
    def seed(self) -> int:
        return (self.N * 31 + self.K * 7 + self.blocksize) % (1 << 31)


# An N that is no multiple of the row tiles is deliberate (a partial last tile in every family).
CASES = (
    LargeCase("below31", 262143, 8192),     # just under 2^31: the last shape the K-quarter kernel may take
    LargeCase("mid", 393219, 8192),         # 3 * 2^30 + ...: past every `int` element index
    LargeCase("below32", 524287, 8192),     # just under 2^32: the last shape of the sm / rt kernels, the last byte offsets under 2^31
    LargeCase("above32", 524418, 8192),     # 2^32 + 130 rows: no MFMA kernel
    LargeCase("above32_k", 1048706, 4096),  # the same at another K: a wrap lands on another row
)
CASE = {c.name: c for c in CASES}
# blocksize 32: the one way into the register-transposed kernel past 2^31 elements (its BS32 instances serve any M; the K-quarter
# kernel stops at 2^31, and the built-in route never picks the blocksize >= 64 instances for more than 96 M weights)
BELOW32_BS32 = LargeCase("below32-bs32", 524287, 8192, 32)
# the expert stack: 520 experts of 1024 x 8192 = 2^32 elements plus 8 experts
EXPERTS_E, EXPERTS_N, EXPERTS_K = 520, 1024, 8192
EXPERTS = LargeCase("experts", EXPERTS_E * EXPERTS_N, EXPERTS_K)


# ------------------------------------------------------------------------------------------ the hash the patterns are seeded from
def mix(index: torch.Tensor) -> torch.Tensor:
    """24 well-mixed bits (int64, non-negative) of an int64 index tensor: splitmix64's finalizer (int64 products wrap)."""
    h = index * -7046029254386353131            # 0x9E3779B97F4A7C15
    h = (h ^ ((h >> 30) & 0x3FFFFFFFF)) * -4658895280553007687   # 0xBF58476D1CE4E5B9
    h = (h ^ ((h >> 27) & 0x1FFFFFFFFF)) * -7723592293110705685  # 0x94D049BB133111EB
    return (h >> 33) & 0xFFFFFF


def _pieces(total: int, step: int):
    for s0 in range(0, total, step):
        yield s0, min(total, s0 + step)


# ------------------------------------------------------------------------------------------ weights
def build_packed(N: int, K: int, blocksize: int, device, seed: int) -> torch.Tensor:
    """[N * K / 2] uint8: two FP4 indices per byte, element 2 i in the high nibble, index 3 at the head of every block."""
    assert K % blocksize == 0 and K % 2 == 0 and blocksize % 2 == 0
    gen = torch.Generator(device=device).manual_seed(seed)
    packed = torch.empty(N * K // 2, dtype=torch.uint8, device=device)
    rows = max(1, PIECE // K)
    for r0, r1 in _pieces(N, rows):
        j = torch.randint(0, len(X.FP4_EXACT_INDICES), (r1 - r0, K), generator=gen, dtype=torch.uint8, device=device)
        nib = (2 * j + 1) * (j > 0) + 2 * (j > 3)   # 0 .. 6 -> 0, 3, 5, 7, 11, 13, 15 (FP4_EXACT_INDICES), all in uint8
        nib[:, ::blocksize] = 3                     # code 1.0 at the head of every block: its absmax is the block's scale
        packed[r0 * K // 2:r1 * K // 2] = ((nib[:, 0::2] << 4) | nib[:, 1::2]).reshape(-1)
    return packed


# ------------------------------------------------------------------------------------------ statistics
def plain_scale(N: int, K: int, blocksize: int, exps, device, pattern=mix) -> torch.Tensor:
    """[N * K / blocksize] fp32 powers of two, exponent lo + (2 r + column parity) % span with r drawn from ``pattern(block index)``."""
    lo, hi = exps
    span = hi - lo + 1
    assert span % 2 == 0
    bpr = K // blocksize
    blocks = N * bpr
    scale = torch.empty(blocks, dtype=torch.float32, device=device)
    for b0, b1 in _pieces(blocks, PIECE // 8):   # (int64 temporaries of 2^24 entries)
        b = torch.arange(b0, b1, dtype=torch.int64, device=device)
        e = lo + (2 * (pattern(b) % (span // 2)) + ((b % bpr) & 1)) % span
        scale[b0:b1] = torch.exp2(e.float())
    return scale


@dataclass
class Nested:
    absmax_8bit: torch.Tensor   # [blocks] uint8 codes into absmax_code
    absmax_code: torch.Tensor   # [256] fp32: NESTED_TABLE[i % 6]
    absmax2: torch.Tensor       # [ceil(blocks / 256)] fp32
    offset: torch.Tensor        # [] fp32
    scale: torch.Tensor         # [blocks] fp32: absmax_code[absmax_8bit] * absmax2[block >> 8] + offset, exact in fp32


def nested_stats(N: int, K: int, blocksize: int, device, pattern=mix) -> Nested:
    span = len(X.NESTED_TABLE)
    bpr = K // blocksize
    blocks = N * bpr
    groups = -(blocks // -256)
    code2 = torch.tensor([X.NESTED_TABLE[i % span] for i in range(256)], dtype=torch.float32, device=device)
    exp2 = torch.tensor(X.NESTED_ABSMAX2_EXP, dtype=torch.float32, device=device)
    g = torch.arange(groups, dtype=torch.int64, device=device)
    absmax2 = torch.exp2(exp2[(2 * (pattern(g + (1 << 40)) % 2) + (g & 1)) % 4])   # even groups: 2^-1 or 2^1; odd groups: 2^0
    q8 = torch.empty(blocks, dtype=torch.uint8, device=device)
    scale = torch.empty(blocks, dtype=torch.float32, device=device)
    offset = torch.tensor(X.NESTED_OFFSET, dtype=torch.float32, device=device)
    for b0, b1 in _pieces(blocks, PIECE // 8):
        b = torch.arange(b0, b1, dtype=torch.int64, device=device)
        h = pattern(b)
        sel = (2 * (h % (span // 2)) + ((b % bpr) & 1)) % span     # parity follows the block column: neighbours differ
        q = sel + span * ((h >> 8) % (256 // span))
        q8[b0:b1] = q.to(torch.uint8)
        scale[b0:b1] = code2[q] * absmax2[b >> 8] + offset          # (each step exact in fp32: <= 7 significant bits)
    return Nested(q8, code2, absmax2, offset, scale)


def assert_not_periodic(scale: torch.Tensor, K: int, blocksize: int, what: str = "scale", wrap_elements: int = 1 << 32) -> None:
    """The pattern does not map onto itself under ANY power-of-two shift (so under no period that divides 2^32 / blocksize), and - where
    the tensor reaches past 2^32 elements - every row past the wrap has a block whose scale differs from the one 2^32 / blocksize
    blocks before it: a block index that lost its bit 32 is then visible in every such row. (``wrap_elements``: the host test runs the
    second rule at a size a CPU holds.)"""
    n = scale.numel()
    p = 1
    while p < n:
        assert not torch.equal(scale[p:], scale[:n - p]), f"{what}: the pattern repeats with a period of {p} blocks"
        p *= 2
    wrap = wrap_elements // blocksize
    bpr = K // blocksize
    if n > wrap:
        differ = scale[wrap:] != scale[:n - wrap]
        if wrap % bpr == 0 and (n - wrap) % bpr == 0:
            differ = differ.view(-1, bpr).any(dim=1)
        else:   # (second-level statistics: one entry per 256 blocks, no rows - some entry past the wrap differs)
            differ = differ.any()
        assert bool(differ.all()), f"{what}: a row past 2^32 elements has the scales of the row 2^32 elements before it"


# ------------------------------------------------------------------------------------------ the constructed W, in float64
def _decode64(b: torch.Tensor, s: torch.Tensor, blocksize: int) -> torch.Tensor:
    """Packed rows [R, K / 2] and their scales [R, K / blocksize] -> float64 [R, K]: nibble look-up times the constructed scale."""
    R, K = b.shape[0], b.shape[1] * 2
    table = torch.tensor(FP4_TABLE, dtype=torch.float64, device=b.device)
    w = torch.empty((R, K), dtype=torch.float64, device=b.device)
    w[:, 0::2] = table[(b >> 4).long()]
    w[:, 1::2] = table[(b & 15).long()]
    return (w.view(R, K // blocksize, blocksize) * s.double().unsqueeze(2)).view(R, K)


def rows64(packed: torch.Tensor, scale: torch.Tensor, K: int, blocksize: int, r0: int, r1: int) -> torch.Tensor:
    """Rows r0 ... r1 - 1 of the constructed W as float64 [r1 - r0, K]."""
    bpr = K // blocksize
    return _decode64(packed[r0 * K // 2:r1 * K // 2].view(r1 - r0, K // 2), scale[r0 * bpr:r1 * bpr].view(r1 - r0, bpr), blocksize)


def gather_rows64(packed: torch.Tensor, scale: torch.Tensor, K: int, blocksize: int, rows) -> torch.Tensor:
    """The listed rows of the constructed W as float64 [len(rows), K]."""
    idx = torch.as_tensor(rows, dtype=torch.long, device=packed.device)
    return _decode64(packed.view(-1, K // 2)[idx], scale.view(-1, K // blocksize)[idx], blocksize)


def int_rows(rows: int, cols: int, dtype: torch.dtype, seed: int, device, limit: int = X.X_MAX) -> torch.Tensor:
    """[rows, cols] integers in [-limit, limit], every row different from every other (asserted)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-limit, limit + 1, (rows, cols), generator=gen, dtype=torch.int8)
    assert torch.unique(x, dim=0).shape[0] == rows, "two activation rows are equal"
    return x.to(dtype).to(device)


def reference(packed, scale, N: int, K: int, blocksize: int, x, bias, dtype, unit: float, chunk_rows: Optional[int] = None):
    """(y, y + bias, worst): float64 ``x @ W.T`` by row chunks of the constructed W, rounded once to ``dtype`` - both [rows of x, N] on the
    device - and the largest sum of product magnitudes (+ |bias|), for which the exact-sum bound is asserted."""
    chunk = chunk_rows or max(1, (1 << 24) // K)
    xt = x.double().t().contiguous()
    xmax = x.double().abs().amax(dim=0)
    assert not bool(x.double().frac().any()) and float(x.abs().max()) <= X.X_MAX
    M = x.shape[0]
    y = torch.empty((M, N), dtype=dtype, device=packed.device)
    yb = torch.empty((M, N), dtype=dtype, device=packed.device)
    worst = 0.0
    for r0, r1 in _pieces(N, chunk):
        w = rows64(packed, scale, K, blocksize, r0, r1)
        assert not bool((w / unit).frac().any()), "a weight is not a multiple of the unit (or a nibble outside the construction)"
        y64 = (w @ xt).t()
        worst = max(worst, float((w.abs() @ xmax).max()))
        y[:, r0:r1] = y64.to(dtype)
        yb[:, r0:r1] = (y64 + bias[r0:r1].double()).to(dtype)
    worst += float(X.BIAS_MAX)
    assert worst < 2.0 ** 24 * unit, f"sum of |products| {worst} reaches 2^24 units ({2.0 ** 24 * unit}): fp32 partial sums may round"
    if dtype == torch.float16:
        assert worst < X.FP16_MAX, f"sum of |products| {worst} reaches the fp16 range"
    return y, yb, worst


# ------------------------------------------------------------------------------------------ one case, built
@dataclass
class Built:
    case: LargeCase
    dtype: torch.dtype
    nested: bool
    packed: torch.Tensor
    scale: torch.Tensor              # the intended absmax of every block (plain statistics: what the op is handed)
    unit: float
    x: torch.Tensor                  # [REF_ROWS, K]
    bias: torch.Tensor               # [N]
    ref: dict = field(default_factory=dict)   # {with_bias: [REF_ROWS, N]}
    worst: float = 0.0
    nest: Optional[Nested] = None

    def stats_args(self):
        """(absmax, absmax_8bit, absmax_code, absmax_offset) as the gemm_4bit op takes them."""
        if not self.nested:
            return self.scale, None, None, None
        return self.nest.absmax2, self.nest.absmax_8bit, self.nest.absmax_code, self.nest.offset


def unit_of(dtype: torch.dtype, nested: bool) -> float:
    if nested:
        return min(X.NESTED_TABLE) * 2.0 ** min(X.NESTED_ABSMAX2_EXP) * 0.25
    return 2.0 ** EXPS[dtype][0] * 0.25


def build(case: LargeCase, device, dtype=torch.bfloat16, nested: bool = False, packed: Optional[torch.Tensor] = None, rows: int = REF_ROWS,
          with_reference: bool = True, chunk_rows: Optional[int] = None, pattern=mix) -> Built:
    """Weights (or the ``packed`` bytes of an earlier build of the same case), statistics, activations, bias and the reference of one
    case on ``device``. Asserts the non-periodicity of the statistics and the exact-sum bound."""
    N, K, bs = case.N, case.K, case.blocksize
    if packed is None:
        packed = build_packed(N, K, bs, device, case.seed)
    assert packed.numel() == N * K // 2
    nest = None
    if nested:
        nest = nested_stats(N, K, bs, device, pattern)
        scale = nest.scale
        assert_not_periodic(nest.absmax_8bit, K, bs, "absmax_8bit")
        if nest.absmax2.numel() > 8:
            assert_not_periodic(nest.absmax2, K * 256, bs * 256, "absmax2")   # (one entry per 256 blocks: the same rule one level up)
    else:
        scale = plain_scale(N, K, bs, EXPS[dtype], device, pattern)
    assert_not_periodic(scale, K, bs)
    if K // bs > 1 and not nested:
        s2 = scale.view(N, K // bs)
        assert bool((s2[:, 1:] != s2[:, :-1]).all()), "neighbouring blocks share a scale"
    unit = unit_of(dtype, nested)
    x = int_rows(rows, K, dtype, case.seed + 1, device)
    gen = torch.Generator().manual_seed(case.seed + 2)
    bias = torch.randint(-X.BIAS_MAX, X.BIAS_MAX + 1, (N,), generator=gen).to(dtype).to(device)
    out = Built(case, dtype, nested, packed, scale, unit, x, bias, nest=nest)
    if with_reference:
        y, yb, out.worst = reference(packed, scale, N, K, bs, x, bias, dtype, unit, chunk_rows)
        out.ref = {False: y, True: yb}
    return out


def first_wrong_row(y: torch.Tensor, ref: torch.Tensor):
    """(weight row n, activation row m, got, want) of the wrong element with the smallest n of two [M, N] tensors (None: bit-equal)."""
    bad = (y != ref).any(dim=0).nonzero()
    if bad.numel() == 0:
        return None
    n = int(bad[0, 0])
    m = int((y[:, n] != ref[:, n]).nonzero()[0, 0])
    return n, m, float(y[m, n]), float(ref[m, n])


# ------------------------------------------------------------------------------------------ the ledger: the source predicates, restated
KC = 256                # csrc/gemm4_mfma.hip: kKC, the MFMA kernels' k chunk
STREAM_MAX_M = 4        # csrc/gemm4_mfma.hip: kStreamMaxM
SM_MIN_ROWS = 128       # csrc/gemm4_mfma.hip: kSmMinRows
DEFAULT_CUS = 256       # csrc/bnb_common.h: device_cu_count_or_default without a device; the MI355X has as many


def sm_supported(M: int, N: int, K: int, bs: int) -> bool:
    """csrc/gemm4_mfma_sm.hip: gemm_4bit_sm_supported for 16-bit activations and aligned pointers."""
    return M >= 1 and N >= 1 and K >= 64 and K % 64 == 0 and bs >= 64 and N * K < 2 ** 32 and M * K < 2 ** 30


def sm_selected(M: int, N: int, K: int, cus: int = DEFAULT_CUS) -> bool:
    """csrc/gemm4_mfma.hip: sm_selected with no tuning knob set."""
    if M < 2 or N < SM_MIN_ROWS:
        return False
    if K % KC:
        return M <= 128
    if N >= 12 * cus:
        return M <= 16 and not (M > 8 and K > 2 * N)
    if M == 2:
        return K <= 5120
    if M <= 4:
        return True
    if M <= 8:
        return K >= 2560 and (N >= 1024 or K <= 4096)
    return M <= 16 and (K <= 4096 or K <= 2 * N)


def rt_supported(M: int, N: int, K: int, bs: int) -> bool:
    """csrc/gemm4_mfma_rt.hip: gemm_4bit_rt_supported's size terms for 16-bit activations, K % 256 == 0 and aligned pointers."""
    return M >= 1 and N >= 1 and K % KC == 0 and bs >= 32 and N * K < 2 ** 32 and M * K < 2 ** 30


def mfma_supported(M: int, N: int, K: int, bs: int) -> bool:
    """csrc/gemm4_mfma.hip: gemm_4bit_mfma_supported for 16-bit activations, plain statistics and aligned pointers."""
    if N * K >= 2 ** 32:
        return False   # no MFMA kernel is claimed at or past 2^32 elements
    if bs == 32:
        return rt_supported(M, N, K, bs)
    return M >= 1 and N >= 1 and K % KC == 0 and bs >= 64


def expected_route(M: int, N: int, K: int, bs: int, cus: int = DEFAULT_CUS) -> int:
    """csrc/gemm4_mfma.hip: gemm_4bit_route (kernel 0) for 16-bit activations: 1 = an MFMA kernel, 0 = the streaming / generic kernel."""
    sm = bs >= 64 and K % 64 == 0 and sm_selected(M, N, K, cus) and sm_supported(M, N, K, bs)
    big = N * K >= (12 << 20)
    return int(sm or ((M > STREAM_MAX_M or (M >= 3 and big)) and mfma_supported(M, N, K, bs)))


def expected_experts(E: int, N: int, K: int, bs: int) -> int:
    """csrc/gemm4_experts.hip: gemm_4bit_experts_supported (kMaxSegs = 32 segments of 2048 k)."""
    ok = E > 0 and N > 0 and K > 0 and bs >= 32 and bs & (bs - 1) == 0 and K % bs == 0
    return int(ok and E <= 65535 and N <= 2 ** 30 and K <= 32 * 2048 and E * N < 2 ** 31)


def expected_grad_input(M: int, N: int, K: int, bs: int) -> int:
    """csrc/gemm4_grad_input.hip: gemm_4bit_grad_input_supported: whole 32-n blocks of 64 rows, 128-column tiles - and no size term."""
    return int(M >= 1 and N >= 64 and N % 64 == 0 and K >= 128 and K % 128 == 0 and bs >= 64 and bs & (bs - 1) == 0)
