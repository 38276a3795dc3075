"""GPU (-m gpu): the launch plans of other CU counts, run on this device, bit for bit.

An MI355X in DPX / QPX / CPX partition mode presents 128 / 64 / 32 compute units; every launch plan of the library reads that count
(tests/test_cu_count_host.py names the plan functions). ``bnb_mi355x_set_cu_count`` makes the calling thread's plans for such a
device, and the kernels then run those geometries here: other rows per workgroup, tiles per workgroup, K and N slices, workspace
sizes, row tiles, wavefront counts - and other families at the same (M, N, K). Nothing else is forced. Inputs are those of
tests/exact_inputs.py (float64 is the only right answer; check_quantization as in the routed sweep); every output element must equal
the reference, and ``bnb_mi355x_last_gemm_kernel()`` must name the family the plan query named.

The cells are not the workload's shapes but the smallest at which a plan differs from the 256-CU plan: tests/cu_count_cases.py, picked
by tests/checks/cu_count_census.py on the host (tests/test_cu_count_host.py fails when a committed cell stops differing); the fused
forms, the grouped launch and the quantizers run hand-picked small shapes and assert here that the plan under the override differs.
An override above the device's real count is skipped. The peer-chain kernels are not run under an override: they poll across
workgroups. Performance under an override is not measured anywhere.
"""
import ctypes as ct
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import cu_count_cases as Cases
import exact_inputs as X
import lora_cases as L
import routed_sweep as S
from conftest import gpu_ready
from routed_sweep import DEV, FAMILY, K_GENERIC, K_SM, K_STREAM

pytestmark = pytest.mark.gpu
OVERRIDES = (32, 64, 128)
BF16 = 2
_T0 = time.time()


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_leave_the_knob_at_rest():
    import os

    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    assert _lib(), "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield
    real = torch.cuda.get_device_properties(0).multi_processor_count
    assert _plan(1, 4096, 4096, 64, False)[10] == -(-4096 // real), "the CU-count override was left set"
    print(f"\ntest_gpu_cu_count.py: {time.time() - _T0:.1f} s wall")


class override:
    """``with override(cus):`` - the calling thread's plans are made for `cus` compute units; always back to 0."""

    def __init__(self, cus):
        self.cus = cus

    current = 0

    def __enter__(self):
        if self.cus > torch.cuda.get_device_properties(0).multi_processor_count:
            pytest.skip(f"the device has fewer than {self.cus} compute units")
        _lib().bnb_mi355x_set_cu_count(self.cus)
        override.current = self.cus

    def __exit__(self, *exc):
        _lib().bnb_mi355x_set_cu_count(0)
        override.current = 0


def _plan(M, N, K, bs, nested):
    out = np.zeros(16, dtype=np.int32)
    ok = _lib().bnb_mi355x_gemm_4bit_plan(0, BF16, M, N, K, bs, int(nested), out.ctypes.data)
    return tuple(int(v) for v in out) if ok == 1 else None


def _form_plan(form, M, N, K, bs, nested, heights=None):
    out = np.zeros(16, dtype=np.int32)
    ns = (ct.c_int * len(heights))(*heights) if heights else None
    ok = _lib().bnb_mi355x_gemm_4bit_sm_form_plan(form, BF16, M, len(heights) if heights else N, ns, K, bs, int(nested), out.ctypes.data)
    return tuple(int(v) for v in out) if ok == 1 else None


def _stream_geometry(form, M, N, K, bs):
    out = np.zeros(8, dtype=np.int32)
    ok = _lib().bnb_mi355x_stream_geometry(form, BF16, M, N, K, bs, out.ctypes.data)
    return tuple(int(v) for v in out) if ok == 1 else None


def _at(cus, f, *args):
    """f(*args) under bnb_mi355x_set_cu_count(cus) - for the 256-CU plan a cell is compared with -, then back to the enclosing override."""
    _lib().bnb_mi355x_set_cu_count(cus)
    try:
        return f(*args)
    finally:
        _lib().bnb_mi355x_set_cu_count(override.current)


@functools.lru_cache(maxsize=None)
def _inputs(N, K, bs, nested, rows, exps=(-2, 3)):
    """The exact operands of one matrix, quantized and checked once, shared by every cell on it and never written to."""
    ex = X.build(N, K, bs, torch.bfloat16, nested, seed=(N * 31 + K * 7 + bs + nested) % (1 << 31), rows=rows, exps=exps)
    packed = X.check_quantization(ex, S.gpu_ops(), DEV)
    ref = {b: ex.reference(b).to(DEV) for b in (False, True)}
    return dict(ex=ex, packed=packed, stats=ex.stats_args(DEV), x=ex.x.to(DEV), bias=ex.bias.to(DEV), ref=ref)


def _rows_of(N, K, bs, nested):
    return max(max(c["Ms"]) for c in Cases.GEMM_CELLS if (c["N"], c["K"], c["blocksize"], c["nested"]) == (N, K, bs, nested)) + 3


# ------------------------------------------------------------------------------------------ gemm_4bit
@pytest.mark.parametrize("cell", Cases.GEMM_CELLS, ids=lambda c: f"{c['cus']}cus-{c['N']}x{c['K']}-bs{c['blocksize']}{'-nested' if c['nested'] else ''}")
def test_gemm_4bit_under_another_cu_count_is_exact(cell):
    """Every batch size of the cell whose plan differs from the 256-CU plan, through the public op: the plan under the override is
    the committed one, the family that ran is the plan's, the result equals the float64 reference bit for bit."""
    lib = _lib()
    N, K, bs, nested = cell["N"], cell["K"], cell["blocksize"], cell["nested"]
    d = _inputs(N, K, bs, nested, _rows_of(N, K, bs, nested))
    absmax, a8, code, off = d["stats"]
    sentinel = S.Sentinel(K_GENERIC)
    wrong = []
    with override(cell["cus"]):
        for M, want_plan in zip(cell["Ms"], cell["plans"]):
            assert _plan(M, N, K, bs, nested) == tuple(want_plan), (M, "the plan is not the committed one: re-run tests/checks/cu_count_census.py")
            with_bias = M % 2 == 0
            sentinel()
            y = torch.ops.bitsandbytes.gemm_4bit.default(d["x"][:M], d["packed"], [N, K], absmax, bs, "fp4", d["bias"] if with_bias else None, a8, code, off)
            family = lib.bnb_mi355x_last_gemm_kernel()
            assert family == want_plan[0], f"M={M}: the {FAMILY.get(family, family)} kernel ran, the plan names {FAMILY[want_plan[0]]}"
            want = d["ref"][with_bias][:M]
            assert y.shape == want.shape and y.dtype == want.dtype
            if not torch.equal(y, want):
                wrong.append((M, FAMILY[family], X.first_mismatch(y.cpu(), want.cpu())))
    assert not wrong, f"{len(wrong)} of {len(cell['Ms'])} batch sizes wrong; (M, family, (row, column, got, want)): {wrong[:8]}"


def test_exact_geometry_gemv_with_more_rows_per_workgroup():
    """4096 x 4096, M = 1: the exact-geometry instance of the streaming kernel with R = 128 / 64 / 32 (256 CUs: 16)."""
    lib = _lib()
    d = _inputs(4096, 4096, 64, False, 4)
    for cus in OVERRIDES:
        if cus > torch.cuda.get_device_properties(0).multi_processor_count:
            continue
        with override(cus):
            assert lib.bnb_mi355x_gemv_4bit_stream_exact(BF16, 1, 4096, 4096, 64, 0) == 1, cus
            plan = _plan(1, 4096, 4096, 64, False)
            assert plan[0] == K_STREAM and plan[10] == 4096 // cus and plan[1] == cus, (cus, plan)
            for with_bias in (False, True):
                y = torch.ops.bitsandbytes.gemm_4bit.default(d["x"][:1], d["packed"], [4096, 4096], d["stats"][0], 64, "fp4", d["bias"] if with_bias else None)
                assert lib.bnb_mi355x_last_gemm_kernel() == K_STREAM
                assert torch.equal(y, d["ref"][with_bias][:1]), (cus, with_bias, X.first_mismatch(y.cpu(), d["ref"][with_bias][:1].cpu()))


# ------------------------------------------------------------------------------------------ the fused backward
def _grad_plan(M, N, K):
    out = np.zeros(16, dtype=np.int32)
    ok = _lib().bnb_mi355x_gemm_4bit_grad_input_plan(BF16, M, N, K, 64, out.ctypes.data)
    return tuple(int(v) for v in out) if ok == 1 else None


@functools.lru_cache(maxsize=None)
def _grad_inputs(N, K, nested):
    d = _inputs(N, K, 64, nested, 4)
    g, ref = X.grad_inputs(d["ex"], 64, seed=N * 3 + K)
    return d, g.to(DEV), ref.to(DEV)


@pytest.mark.parametrize("cell", Cases.GRAD_CELLS, ids=lambda c: f"{c['cus']}cus-{c['N']}x{c['K']}-M{c['M']}")
def test_fused_backward_under_another_cu_count_is_exact(cell):
    """bitsandbytes_amd::gemm_4bit_grad_input at 1, 2 and 4 row tiles, with one N slice and with several (the op takes the workspace
    size from the query, under the same override), against the float64 g @ W of integer gradients."""
    M, N, K = cell["M"], cell["N"], cell["K"]
    d, g, ref = _grad_inputs(N, K, False)
    absmax, a8, code, off = d["stats"]
    with override(cell["cus"]):
        plan = _grad_plan(M, N, K)
        assert plan == tuple(cell["plan"]), "the plan is not the committed one: re-run tests/checks/cu_count_census.py"
        assert _lib().bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) == (plan[4] * M * K * 4 if plan[4] > 1 else 0)
        y = torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(g[:M], d["packed"], [N, K], absmax, 64, "fp4", a8, code, off)
    assert y.shape == (M, K) and torch.equal(y, ref[:M]), X.first_mismatch(y.cpu(), ref[:M].cpu())


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("cus", OVERRIDES)
def test_fused_backward_1216x384_under_another_cu_count(cus, nested):
    """The routed sweep's 1216 x 384 (19 blocks of 64 n, three 128-column workgroups - no power of two anywhere) at 1, 2 and 4 row
    tiles and two passes of 64 rows."""
    N, K = 1216, 384
    d, g, ref = _grad_inputs(N, K, nested)
    absmax, a8, code, off = d["stats"]
    with override(cus):
        for M in (1, 16, 17, 32, 33, 64):
            y = torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(g[:M], d["packed"], [N, K], absmax, 64, "fp4", a8, code, off)
            assert torch.equal(y, ref[:M]), (M, _grad_plan(M, N, K), X.first_mismatch(y.cpu(), ref[:M].cpu()))


# ------------------------------------------------------------------------------------------ gated, LoRA, grouped
FUSED_SHAPE = {32: (1088, 256), 64: (1088, 256), 128: (4096, 256)}   # (N, K) whose sm and stream plans differ from the 256-CU ones


@pytest.mark.parametrize("cus", OVERRIDES)
def test_gated_launch_under_another_cu_count(cus):
    """bitsandbytes_amd::gemm_4bit_gated through the streaming kernel (M = 1: an even R, pairs) and the streaming MFMA kernel
    (M = 2 ... 16) against torch's silu(gate) * up of the float64 reference rounded once."""
    lib = _lib()
    N, K = FUSED_SHAPE[cus]
    d = _inputs(N, K, 64, False, 20, (-8, -5))
    with override(cus):
        for M in (1, 2, 4, 5, 16):
            if M == 1:
                here, base = _stream_geometry(2, M, N, K, 64), _at(256, _stream_geometry, 2, M, N, K, 64)
                assert here is not None and here != base and here[0] % 2 == 0, (here, base)
            else:
                here, base = _form_plan(1, M, N, K, 64, False), _at(256, _form_plan, 1, M, N, K, 64, False)
                assert here is not None and here != base and here[10] % 2 == 0, (here, base)
            for with_bias in (False, True):
                y = d["ref"][with_bias][:M]
                want = TF.silu(y[:, 0::2]) * y[:, 1::2]
                out = torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(d["x"][:M], d["packed"], [N, K], d["stats"][0], 64, "fp4", d["bias"] if with_bias else None)
                assert lib.bnb_mi355x_last_gemm_kernel() == (K_STREAM if M == 1 else K_SM), M
                assert torch.equal(out, want), (cus, M, with_bias, X.first_mismatch(out.cpu(), want.cpu()))


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("cus", OVERRIDES)
def test_lora_launch_under_another_cu_count(cus, nested):
    """bitsandbytes_amd::gemm_4bit_lora through both families against (x W^T + bias + s t B_l^T) in float64, rounded once
    (tests/lora_cases.py's adapters)."""
    lib = _lib()
    N, K = FUSED_SHAPE[cus]
    case = L.LoRACase(N, K, 64, torch.bfloat16, nested)
    d = _inputs(N, K, 64, nested, L.MAX_ROWS, L.EXPS)
    absmax, a8, code, off = d["stats"]
    y64 = d["x"].double() @ d["ex"].W.to(DEV).double().t()
    with override(cus):
        for r, s in ((8, 0.5), (24, 2.0)):
            t, b = (v.to(DEV) for v in L.build_adapter(case, r))
            term = L.adapter_term64(t, b, s)
            for M in (1, 2, 8, 16):
                if M > 1:
                    here, base = _form_plan(2, M, N, K, 64, nested), _at(256, _form_plan, 2, M, N, K, 64, nested)
                    assert here is not None and here != base, (here, base)
                with_bias = (M + r) % 16 == 0
                want = (y64 + term + (d["bias"].double() if with_bias else 0.0)).to(torch.bfloat16)[:M]
                out = torch.ops.bitsandbytes_amd.gemm_4bit_lora.default(d["x"][:M], d["packed"], [N, K], absmax, 64, "fp4", t[:M].contiguous(), b, s,
                                                                        d["bias"] if with_bias else None, absmax_8bit=a8, absmax_code=code, absmax_offset=off)
                assert lib.bnb_mi355x_last_gemm_kernel() == (K_STREAM if M == 1 else K_SM), M
                assert torch.equal(out, want), (cus, r, M, X.first_mismatch(out.cpu(), want.cpu()))


@pytest.mark.parametrize("cus", OVERRIDES)
def test_grouped_launch_raises_rows_per_workgroup_in_its_limit_loop(cus):
    """bnb_mi355x_gemm_4bit_grouped on members whose own shares, each rounded up, need more workgroups than the plan of their sum:
    the loop of sm_grouped_plan (csrc/gemm4_mfma_sm.hip) raises R - asserted on the plan - and each member equals ITS float64
    reference; one row runs the streaming kernel's grouped launch under the override's R."""
    from bitsandbytes_amd.backends import hip

    lib = _lib()
    heights = {32: (1088, 1216), 64: (2075, 2211), 128: (4200, 4300)}[cus]
    K = 256
    x = X.int_rows(20, K, torch.bfloat16, torch.Generator().manual_seed(cus))
    members = []
    for i, N in enumerate(heights):
        d = _inputs(N, K, 64, False, 4)
        X.assert_exact_sums(d["ex"].W, x, d["ex"].unit, torch.bfloat16, extra=float(X.BIAS_MAX))
        members.append((d, {b: ((x.double() @ d["ex"].W.double().t()) + (d["ex"].bias.double() if b else 0.0)).to(torch.bfloat16).to(DEV) for b in (False, True)}))
    xd = x.to(DEV)
    ns = (ct.c_int * len(heights))(*heights)
    with override(cus):
        for M in (1, 2, 8, 16):
            if M > 1:
                plan, single = _form_plan(4, M, 0, K, 64, False, heights), _plan(M, sum(heights), K, 64, False)
                assert plan is not None and single[0] == K_SM and plan[10] > single[10], (M, plan, single, "the limit loop did not raise R")
            assert lib.bnb_mi355x_gemm_4bit_grouped_route(BF16, len(heights), ns, M, K, 64) == (1 if M == 1 else 2)
            with_bias = [(M + i) % 2 == 0 for i in range(len(heights))]
            mats = [(d["packed"], (d["ex"].N, K), d["stats"][0], d["bias"] if wb else None, None, None, None) for (d, _), wb in zip(members, with_bias)]
            ys = hip.gemm_4bit_grouped(xd[:M], mats, 64, "fp4")
            assert lib.bnb_mi355x_last_gemm_kernel() == (K_STREAM if M == 1 else K_SM), M
            for i, (y, (d, ref), wb) in enumerate(zip(ys, members, with_bias)):
                assert torch.equal(y, ref[wb][:M]), (cus, M, i, X.first_mismatch(y.cpu(), ref[wb][:M].cpu()))


# ------------------------------------------------------------------------------------------ the quantizers' grid caps
def test_quantize_4bit_fp4_pipelined_form_at_32_cus():
    """2 M elements = 512 tiles of 4096: the smallest input that takes the pipelined, grid-strided form (csrc/quantize4.hip: >= 4
    tiles for each of 4 * cus workgroups) on 32 CUs - a grid of 128 workgroups; 256 CUs take it from 16 M. Codes and absmax bit-equal
    to the oracle, and to the one-tile form."""
    import bitsandbytes_amd as bnb
    from oracle import oracle as O

    F = bnb.functional
    n = 512 * 4096
    A = (torch.randn(n, generator=torch.Generator().manual_seed(21)) * 0.3).to(torch.bfloat16)
    A[::4099] = 0
    q_o, am_o = O.quantize_4bit(A, 64, "fp4")
    with override(32):
        q, st = F.quantize_4bit(A.to(DEV), blocksize=64, quant_type="fp4")
    assert torch.equal(q.cpu().flatten(), q_o.flatten()) and torch.equal(st.absmax.cpu(), am_o)
    q1, st1 = F.quantize_4bit(A.to(DEV), blocksize=64, quant_type="fp4")   # (no override: the one-tile form at this size)
    assert torch.equal(q1, q) and torch.equal(st1.absmax, st.absmax)


def test_quantize_blockwise_8bit_at_its_grid_cap_at_32_cus():
    """1 M elements + a ragged tail: the smallest input of the byte-table kernel (csrc/blockwise8.hip: from 2^20 elements), 4097 units
    in 129 workgroups - capped to 2 * cus = 64 persistent ones on 32 CUs, each walking its units twice. Codes and absmax bit-equal to
    the oracle."""
    import bitsandbytes_amd as bnb
    from oracle import oracle as O

    code = bnb.functional.create_dynamic_map()
    n = (1 << 20) + 333
    A = torch.randn(n, generator=torch.Generator().manual_seed(5)) * 0.05
    A[5000:5256] = 0
    q_o, am_o = O.quantize_blockwise(A, code, 256)
    with override(32):
        q, am = torch.ops.bitsandbytes.quantize_blockwise.default(A.to(DEV), code.to(DEV), 256)
    assert torch.equal(q.cpu(), q_o) and torch.equal(am.cpu(), am_o)
