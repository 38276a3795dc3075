"""The routed sweep itself (GPU): every M of a case through the PUBLIC ``bitsandbytes::gemm_4bit`` op - no tuning knob, no kernel
argument - on the inputs of tests/exact_inputs.py, one record per call. Shared by tests/test_gpu_routed_sweep.py (which asserts on
the records) and tests/checks/routed_census.py (which prints them)."""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import torch

import exact_inputs as X

DEV = "cuda"
# kernel families as bnb_mi355x_last_gemm_kernel() reports them (include/bnb_mi355x.h)
K_STREAM, K_GENERIC, K_RT, K_PC, K_KQ, K_SM = 1, 2, 3, 4, 6, 7
FAMILY = {0: "none", K_STREAM: "stream", K_GENERIC: "generic", K_RT: "rt", K_PC: "pc", K_KQ: "kq", K_SM: "sm"}
ROUTED_FAMILIES = (K_STREAM, K_SM, K_RT, K_PC, K_KQ)
MFMA_FAMILIES = (K_RT, K_PC, K_KQ, K_SM)
DT_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


def gpu_ops() -> X.QuantOps:
    ops = torch.ops.bitsandbytes
    return X.QuantOps(
        quantize_4bit=lambda W, bs: ops.quantize_4bit.default(W, bs, "fp4", torch.uint8),
        dequantize_4bit=lambda q, absmax, bs, shape, dtype: ops.dequantize_4bit.default(q, absmax, bs, "fp4", list(shape), dtype),
        dequantize_blockwise=lambda codes, absmax, table, bs: ops.dequantize_blockwise.default(codes, absmax, table, bs, torch.float32),
    )


class Sentinel:
    """A tiny call of a family the call under test cannot take, made right before it: if ``bnb_mi355x_last_gemm_kernel()`` still names
    the sentinel's family afterwards, the call launched NO fused kernel (dequantize + library GEMM). ``generic``: K = 33 is outside
    every other kernel's preconditions (the scalar kernel; no aligned call with K % 32 == 0 runs it). ``stream``: one row."""

    def __init__(self, family: int):
        from bitsandbytes_amd.backends import hip

        self.family = family
        gen = torch.Generator().manual_seed(9)
        if family == K_GENERIC:
            N, K, bs, dtype = 10, 33, 32, torch.float16
        else:
            assert family == K_STREAM
            N, K, bs, dtype = 64, 64, 64, torch.bfloat16
        W = (torch.randn(N, K, generator=gen) / 4).to(dtype).to(DEV)
        q, absmax = torch.ops.bitsandbytes.quantize_4bit.default(W, bs, "nf4", torch.uint8)
        x = torch.randn(1, K, generator=gen).to(dtype).to(DEV)
        self.call = lambda: hip._gemm_4bit_fused(x, q, (N, K), absmax, bs, "nf4", None, None, None, None, kernel=1)
        self()

    def __call__(self):
        self.call()
        ran = _lib().bnb_mi355x_last_gemm_kernel()
        assert ran == self.family, f"the sentinel call ran family {FAMILY.get(ran, ran)}, not {FAMILY[self.family]}"


def fused_limit(case: X.SweepCase) -> int:
    from bitsandbytes_amd.backends import hip

    if case.dtype == torch.float32:
        return X.FUSED_MAX_M_FP32
    return hip.fused_max_m(case.N, case.K, case.blocksize, case.nested)


def expected_route(case: X.SweepCase, M: int) -> int:
    """What ``bnb_mi355x_gemm_4bit_route`` says for the call: 0 = streaming kernel, 1 = an MFMA kernel. The query sees shapes only and
    assumes plain statistics; the one class where the kind of statistics changes the answer is blocksize 32 (nested: no MFMA kernel)."""
    if case.blocksize == 32 and case.nested:
        return 0
    return int(_lib().bnb_mi355x_gemm_4bit_route(0, DT_CODE[case.dtype], M, case.N, case.K, case.blocksize))


@dataclass
class Record:
    M: int
    bias: bool
    fused: bool          # M <= fused_max_m: a fused kernel must have been launched
    route: int           # bnb_mi355x_gemm_4bit_route's answer
    family: int          # what ran (0: no fused launch)
    mismatch: tuple | None  # first wrong (row, column, got, want); None: bit-equal to the float64 reference
    rel_rows: float = 0.0   # largest per-row relative error (0 when bit-equal)


@dataclass
class CaseResult:
    case: X.SweepCase
    fused_max: int
    records: list = field(default_factory=list)
    seconds: float = 0.0


def describe(case_name: str, r: Record) -> str:
    where = "bit-equal" if r.mismatch is None else "first wrong (row %d, column %d): got %r, want %r" % r.mismatch
    return f"{case_name} M={r.M} bias={int(r.bias)} family={FAMILY.get(r.family, r.family)} route={r.route}: {where}"


def max_row_rel_err(y: torch.Tensor, ref: torch.Tensor) -> float:
    y, ref = y.double(), ref.double()
    return float(((y - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())


def run_case(case: X.SweepCase, index: int) -> CaseResult:
    """All M of ``X.sweep_ms`` for one case. Bias on the calls where M + index is even, so that a family that serves a single M
    (the producer/consumer kernel at 64 rows of a 4096^2 weight) meets both forms across the cases."""
    lib = _lib()
    t0 = time.time()
    fmax = fused_limit(case)
    ms = X.sweep_ms(fmax)
    ex = X.build(case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=ms[-1] + 3, exps=case.exps)
    packed = X.check_quantization(ex, gpu_ops(), DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    x = ex.x.to(DEV)
    bias = ex.bias.to(DEV)
    ref = {b: ex.reference(b).to(DEV) for b in (False, True)}
    sentinel = Sentinel(K_GENERIC)
    res = CaseResult(case, fmax)
    for M in ms:
        with_bias = (M + index) % 2 == 0
        sentinel()
        y = torch.ops.bitsandbytes.gemm_4bit.default(x[:M], packed, [case.N, case.K], absmax, case.blocksize, "fp4",
                                                     bias if with_bias else None, a8, code, off)
        family = lib.bnb_mi355x_last_gemm_kernel()
        if family == K_GENERIC:
            family = 0   # (still the sentinel's: nothing fused was launched)
        want = ref[with_bias][:M]
        assert y.shape == want.shape and y.dtype == want.dtype
        rec = Record(M, with_bias, M <= fmax, expected_route(case, M), family, None)
        if not torch.equal(y, want):
            rec.mismatch = X.first_mismatch(y.cpu(), want.cpu())
            rec.rel_rows = max_row_rel_err(y, want)
        res.records.append(rec)
    res.seconds = time.time() - t0
    return res


def family_ranges(records) -> str:
    """'1: stream, 2-16: sm, ...' - runs of equal (family, bit-equal) over the M of a case."""
    out, start, prev = [], None, None
    for r in records:
        key = (FAMILY.get(r.family, str(r.family)) if r.family else "dequantize+GEMM", r.mismatch is None)
        if prev is not None and key == prev[0] and r.M == prev[1] + 1:
            prev = (key, r.M)
            continue
        if prev is not None:
            out.append((start, prev[1], prev[0]))
        start, prev = r.M, (key, r.M)
    out.append((start, prev[1], prev[0]))
    return ", ".join(f"{a}{'' if a == b else '-' + str(b)}: {k[0]}{'' if k[1] else ' (NOT bit-equal)'}" for a, b, k in out)
