"""GPU: the fused 4-bit matmul kernels under block scales from the whole fp32 range (tests/matmul_scale_range_cases.py; preconditions
on the CPU: tests/test_matmul_scale_range_host.py).

1. The one-hot probe of tests/test_gpu_decode_probe.py under every scale of ``scale_range_cases.scales()`` - subnormal scales, 2^127,
   full mantissas, +inf and NaN - and, nested, every second-level scale of ``nested_absmax2()`` under every offset of ``OFFSETS``. The
   want is the family's own order of operations (the ledger ``ORDER``) restated in CPU fp32.
2. Dense exact sums with the scales at the bottom and at the top of what the type holds, through every K split and finalize launch.
3. One non-finite block scale, activation or bias element per call: its row or column is non-finite, everything else has the clean
   call's bits.

Each family is forced as tests/test_gpu_decode_probe.py forces it and every call asserts the family that ran. No tolerance anywhere:
bit for bit, NaN against NaN, either zero where a zero is wanted.
"""
import os
import time
from contextlib import contextmanager

import pytest
import torch

import decode_probe_cases as P
import matmul_scale_range_cases as C
import scale_range_cases as R
from conftest import gpu_ready

pytestmark = pytest.mark.gpu

DEV = "cuda"
_id = lambda cs: cs.name
INF, NAN = float("inf"), float("nan")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _hip():
    from bitsandbytes_amd.backends import hip

    return hip


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    assert _bnb().lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield


@contextmanager
def _knob(knob):
    lib = _bnb().lib
    lib.bnb_mi355x_set_tuning(0, 0, 0, knob)
    try:
        yield
    finally:
        lib.bnb_mi355x_set_tuning(0, 0, 0, 0)


def _kernel_arg(family):
    return 1 if family in ("stream", "generic") else 2


def _gemm(family, x, packed, shape, stats, blocksize, quant, bias=None, out=None):
    """One forced forward call (the knob is the caller's); asserts the family that ran."""
    absmax, a8, code2, offset = stats
    y = _hip()._gemm_4bit_fused(x, packed, shape, absmax, blocksize, quant, bias, a8, code2, offset, kernel=_kernel_arg(family), out=out)
    ran = _bnb().lib.bnb_mi355x_last_gemm_kernel()
    assert ran == C.FAMILY_ID[family], f"kernel family {ran} ran, the case is about {family}"
    return y


def _report(part, cs, launches, cells, runs, t0):
    """One line per case, then one per run (fill, offset or window) with the census of that run's wants."""
    print(f"matmul-scale-range part={part} family={cs.family} case={cs.name} launches={launches} cells={cells} "
          f"wall_ms={(time.perf_counter() - t0) * 1e3:.0f}")
    for line in runs:
        print(f"    {line}")


# ------------------------------------------------------------------------------------------ part 1: the one-hot probe
def _probe_runs(cs):
    """(fill index, offset) of every run of a case: the fills of a plain case, the offsets of a nested one."""
    return [(0, off) for off in R.OFFSETS] if cs.nested else [(fi, 0.0) for fi in range(cs.fills)]


def _forward(cs):
    t0 = time.perf_counter()
    N, K = cs.N, cs.K
    ks = C.probe_ks(cs)
    x, v = P.one_hot_rows(ks, K, cs.dtype)
    xd = x.to(DEV)
    rows = ks.numel()
    step = cs.rows or rows
    launches = cells = 0
    runs = []
    packed = None
    with _knob(cs.knob):
        for fi, off in _probe_runs(cs):
            pr = C.build(cs, fi, off)
            packed = pr.packed.to(DEV) if packed is None else packed
            want = C.want_forward(pr, ks, v)
            stats = pr.stats_args(DEV)
            got = torch.empty(rows, N, dtype=cs.dtype, device=DEV)
            for m0 in range(0, rows, step):
                m1 = min(rows, m0 + step)
                _gemm(cs.family, xd[m0:m1], packed, (N, K), stats, cs.blocksize, cs.quant, out=got[m0:m1])
                launches += 1
            got = got.cpu()
            cols = C.nonfinite_columns(pr)
            assert int(cols.sum()) >= 4 and not bool(torch.isfinite(got[:, cols].float()).any()), "a column with a non-finite scale holds a finite value"
            mm = C.first_mismatch(pr, got, want, ks)
            assert mm is None, f"fill {fi} offset {off!r} order {C.order_of(cs.family, cs.dtype)}: {mm}"
            cells += want.numel()
            runs.append(f"fill {fi} offset {off!r}: {C.census(want)}")
    _report(1, cs, launches, cells, runs, t0)


@pytest.mark.parametrize("cs", C.CASES["stream"], ids=_id)
def test_stream_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["generic"], ids=_id)
def test_generic_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["sm"], ids=_id)
def test_mfma_sm_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["rt"], ids=_id)
def test_mfma_rt_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["kq"], ids=_id)
def test_mfma_kq_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["pc"], ids=_id)
def test_mfma_pc_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["tall"], ids=_id)
def test_mfma_tall_kernel_under_every_scale(cs):
    _forward(cs)


@pytest.mark.parametrize("cs", C.CASES["experts"], ids=_id)
def test_experts_kernel_under_every_scale(cs):
    t0 = time.perf_counter()
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default
    assert _hip().gemm_4bit_experts_supported(cs.dtype, cs.E, cs.N, cs.K, cs.blocksize)
    ks = C.probe_ks(cs)
    x, ids, v = C.experts_probe(cs, ks)
    xd, idd = x.to(DEV), ids.to(DEV)
    T, S = ids.shape
    masked = ((ids < 0) | (ids >= cs.E)).reshape(-1)
    keep = (~masked).nonzero().flatten()
    probed, expert = ks.repeat_interleave(S)[keep], ids.reshape(-1)[keep]
    launches = cells = 0
    runs = []
    packed = None
    for fi, off in _probe_runs(cs):
        pr = C.build(cs, fi, off)
        packed = pr.packed.to(DEV) if packed is None else packed
        want = C.experts_want(pr, ks, ids, v).reshape(T * S, cs.N)
        absmax, a8, code2, offset = pr.stats_args(DEV)
        y = op(xd, packed, [cs.E, cs.N, cs.K], absmax, idd, cs.blocksize, cs.quant, None, a8, code2, offset)
        assert _bnb().lib.bnb_mi355x_last_gemm_kernel() == C.FAMILY_ID["experts"]
        got = y.cpu().reshape(T * S, cs.N)
        assert not bool(got[masked].any()), "a masked slot is not a row of zeros"
        for e in range(cs.E):
            cols = C.nonfinite_columns(pr, e)
            assert not bool(torch.isfinite(got[(ids.reshape(-1) == e)][:, cols].float()).any())
        mm = C.first_mismatch(pr, got[keep], want[keep], probed, expert=expert)
        assert mm is None, f"fill {fi} offset {off!r}: {mm}"
        launches += 1
        cells += int(keep.numel()) * cs.N
        runs.append(f"fill {fi} offset {off!r}: {C.census(want[keep])}")
    _report(1, cs, launches, cells, runs, t0)


@contextmanager
def _backward_plan(lib, plan, M, N, K):
    """The workspace handling of test_fused_backward_decodes_every_byte: 'single' - the built-in plan of the shape, one N slice, no
    workspace; 'sliced' - one slice per 32-row block asked for, a workspace of three slabs handed over: three slices of unequal length
    through the workspace and the finalize launch. Yields (workspace, bytes)."""
    slab = M * K * 4
    try:
        if plan == "sliced":
            lib.bnb_mi355x_set_tuning(0, N // 32, 0, 0)
            assert lib.bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) == (N // 32) * slab
            yield torch.empty(3 * slab, dtype=torch.uint8, device=DEV), 3 * slab
        else:
            assert lib.bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) == 0, "the built-in plan of this shape is one slice"
            yield None, 0
    finally:
        lib.bnb_mi355x_set_tuning(0, 0, 0, 0)


def _grad_input(lib, dtype, g, packed, stats, M, N, K, blocksize, quant, ws, ws_bytes):
    hip = _hip()
    absmax, a8, code2, offset = stats
    out = torch.empty(M, K, dtype=dtype, device=DEV)
    assert g.data_ptr() % 16 == 0 and packed.data_ptr() % 16 == 0 and g.is_contiguous()
    lib.bnb_mi355x_gemm_4bit_grad_input(hip._DT_CODE[dtype], g.data_ptr(), packed.data_ptr(), absmax.data_ptr(), hip._ptr(a8), hip._ptr(code2),
                                        hip._ptr(offset), out.data_ptr(), M, N, K, blocksize, hip._QT_CODE[quant], hip._ptr(ws), ws_bytes,
                                        hip._stream(g))
    return out


@pytest.mark.parametrize("cs", C.CASES["grad_input"], ids=_id)
def test_fused_backward_under_every_scale(cs):
    lib = _bnb().lib
    t0 = time.perf_counter()
    M, N, K = cs.N, cs.N, cs.K
    assert lib.bnb_mi355x_gemm_4bit_grad_input_supported(_hip()._DT_CODE[cs.dtype], M, N, K, cs.blocksize) == 1
    ns = torch.arange(N)
    g, v = P.one_hot_rows(ns, N, cs.dtype)
    gd = g.to(DEV)
    launches = cells = 0
    runs = []
    packed = None
    with _backward_plan(lib, cs.plan, M, N, K) as (ws, ws_bytes):
        for fi, off in _probe_runs(cs):
            pr = C.build(cs, fi, off)
            packed = pr.packed.to(DEV) if packed is None else packed
            want = C.want_backward(pr, ns, v)
            got = _grad_input(lib, cs.dtype, gd, packed, pr.stats_args(DEV), M, N, K, cs.blocksize, cs.quant, ws, ws_bytes).cpu()
            mm = C.first_mismatch(pr, got, want, ns, backward=True)
            assert mm is None, f"fill {fi} offset {off!r}: {mm}"
            launches += 2 if cs.plan == "sliced" else 1
            cells += want.numel()
            runs.append(f"fill {fi} offset {off!r}: {C.census(want)}")
    _report(1, cs, launches, cells, runs, t0)


# ------------------------------------------------------------------------------------------ parts 2 and 3: dense calls
def _dense_call(dc, di, x=None, stats=None, bias=None, g=None, plan=None):
    """One call of a dense case: the forced forward, the experts op or the fused backward's entry point. Returns the result on the CPU:
    [M, N], [T * S, N] (experts) or [M, K] (backward)."""
    lib = _bnb().lib
    ex = di.ex
    stats = ex.stats_args(DEV) if stats is None else stats
    packed = di.packed.to(DEV)
    if dc.family == "grad_input":
        ws, ws_bytes = plan
        g = (di.g if g is None else g).to(DEV).contiguous()
        return _grad_input(lib, dc.dtype, g, packed, stats, dc.M, dc.N, dc.K, dc.blocksize, "fp4", ws, ws_bytes).cpu()
    x = (ex.x if x is None else x).to(DEV)
    if dc.family == "experts":
        T, S = di.ids.shape
        y = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default(x.view(T, S, dc.K), packed, [dc.E, dc.N, dc.K], stats[0], di.ids.to(DEV), dc.blocksize,
                                                                 "fp4", None if bias is None else bias.to(DEV).view(dc.E, dc.N), *stats[1:])
        assert lib.bnb_mi355x_last_gemm_kernel() == C.FAMILY_ID["experts"]
        return y.cpu().reshape(T * S, dc.N)
    return _gemm(dc.family, x, packed, (dc.N, dc.K), stats, dc.blocksize, "fp4", bias=None if bias is None else bias.to(DEV)).cpu()


@contextmanager
def _dense_plan(dc):
    """The forced launch of a dense case: (workspace, bytes) of the fused backward's plan, or the forward's knob."""
    if dc.family == "grad_input":
        with _backward_plan(_bnb().lib, dc.plan, dc.M, dc.N, dc.K) as plan:
            yield plan
    else:
        with _knob(dc.knob):
            # the knob's K slices are a request: the plan really splits (a workspace, hence a finalize launch) exactly where the case
            # says so - a clamp to one slice would turn a split case into an unsplit one unnoticed
            if dc.family in ("sm", "rt", "kq", "pc", "tall"):
                ws = _bnb().lib.bnb_mi355x_gemm_4bit_workspace_bytes(2, _hip()._DT_CODE[dc.dtype], dc.M, dc.N, dc.K, dc.blocksize)
                assert (ws > 0) == dc.split, f"{dc.name}: workspace of {ws} bytes, split = {dc.split}"
            yield None


@pytest.mark.parametrize("dc", C.ALL_DENSE, ids=lambda dc: f"{dc.family}-{dc.name}")
def test_exact_sums_at_the_ends_of_the_scale_range(dc):
    """exact_inputs at the bottom and top windows of the type: every family's order gives the float64 product rounded once - subnormal
    weights, subnormal fp32 partial sums, partial sums up to 2^127, fp16 results that overflow to +-inf - through every K split,
    workspace and finalize launch."""
    t0 = time.perf_counter()
    cells = 0
    runs = []
    with _dense_plan(dc) as plan:
        for window in C.WINDOWS[dc.dtype]:
            di = C.window_inputs(dc, window)
            want = di.reference()
            got = _dense_call(dc, di, plan=plan)
            want = want.reshape(got.shape)
            mm = R.first_mismatch(got, want)
            assert mm is None, f"window {window} {C.WINDOWS[dc.dtype][window]}: {mm}"
            cells += want.numel()
            runs.append(f"window {window} {C.WINDOWS[dc.dtype][window]}: {C.census(want)}")
    _report(2, dc, len(C.WINDOWS[dc.dtype]) * (2 if dc.split else 1), cells, runs, t0)


def _check_poison(what, clean, got, bad):
    """``bad`` (bool, the result's shape): every output there is non-finite; every other output has the clean call's bits."""
    assert bool(bad.any())
    assert bool((~torch.isfinite(got.float()[bad])).all()), f"{what}: a poisoned output is finite"
    iv = P.INT_VIEW[got.dtype]
    same = got.contiguous().view(iv) == clean.contiguous().view(iv)
    leak = (~same) & ~bad
    assert not bool(leak.any()), f"{what}: {int(leak.sum())} outputs outside the poisoned row / column changed; first at {tuple(leak.nonzero()[0].tolist())}"


def _scale_mask(dc, di, blocks, shape):
    """Outputs that a non-finite scale of ``blocks`` (flat indices) reaches; never all of them (asserted): some output is left to
    show that nothing leaks."""
    bad = _scale_mask_of(dc, di, blocks, shape)
    assert not bool(bad.all()), "the poisoned scale reaches every column: no output is left to compare with the clean call"
    return bad


def _scale_mask_of(dc, di, blocks, shape):
    bad = torch.zeros(shape, dtype=torch.bool)
    bpr = dc.K // dc.blocksize
    if dc.family == "grad_input":
        for b in blocks.tolist():
            bad[:, (b % bpr) * dc.blocksize:(b % bpr + 1) * dc.blocksize] = True
        return bad
    rows = C.rows_of_blocks(dc, blocks)
    if dc.family == "experts":
        flat_ids = di.ids.reshape(-1)
        for r in rows.tolist():
            bad[flat_ids == r // dc.N, r % dc.N] = True
        return bad
    bad[:, rows] = True
    return bad


DENSE_AND_NESTED = list(C.ALL_DENSE) + [dc for dc in C.NESTED_DENSE.values() if dc is not None]


@pytest.mark.parametrize("dc", DENSE_AND_NESTED, ids=lambda dc: f"{dc.family}-{dc.name}")
def test_a_non_finite_operand_poisons_its_row_or_column_only(dc):
    t0 = time.perf_counter()
    di = C.clean_inputs(dc)
    ex = di.ex
    backward = dc.family == "grad_input"
    calls = 0
    with _dense_plan(dc) as plan:
        bias = None if backward else ex.bias
        clean = _dense_call(dc, di, bias=bias, plan=plan)
        want = di.reference(with_bias=not backward).reshape(clean.shape)
        assert R.same_bits(clean, want), R.first_mismatch(clean, want)
        absmax, a8, code2, offset = ex.stats_args("cpu")
        # block scale
        for name, b in C.poison_blocks(dc).items():
            for value in (INF, NAN):
                if dc.nested:
                    a2 = absmax.clone()
                    a2[b // 256] = value
                    stats, blocks = (a2.to(DEV), a8.to(DEV), code2.to(DEV), offset.to(DEV)), torch.arange(b // 256 * 256, min((b // 256 + 1) * 256, a8.numel()))
                else:
                    s = absmax.clone()
                    s[b] = value
                    stats, blocks = (s.to(DEV), None, None, None), torch.tensor([b])
                got = _dense_call(dc, di, stats=stats, bias=bias, plan=plan)
                _check_poison(f"scale {name} = {value}", clean, got, _scale_mask(dc, di, blocks, clean.shape))
                calls += 1
        if dc.nested:   # an entry of the second-level code, selected by one absmax_8bit code: every block that carries the code
            for q, value in ((int(a8[C.poison_blocks(dc)["last-of-row"]]), INF), (int(a8[C.poison_blocks(dc)["ragged-tile"]]), NAN)):
                c2 = code2.clone()
                c2[q] = value
                blocks = (a8 == q).nonzero().flatten()
                got = _dense_call(dc, di, stats=(absmax.to(DEV), a8.to(DEV), c2.to(DEV), offset.to(DEV)), bias=bias, plan=plan)
                _check_poison(f"absmax_code[{q}] = {value}", clean, got, _scale_mask(dc, di, blocks, clean.shape))
                calls += 1
        # activation (the backward: gradient)
        for m, c, value in C.poison_activations(dc):
            src = (di.g if backward else ex.x).clone()
            src[m, c] = value
            got = _dense_call(dc, di, bias=bias, plan=plan, **({"g": src} if backward else {"x": src}))
            bad = torch.zeros(clean.shape, dtype=torch.bool)
            bad[m] = True
            if dc.family == "experts" and not (0 <= int(di.ids.reshape(-1)[m]) < dc.E):
                assert torch.equal(got, clean), "a masked slot read its activations"
            else:
                _check_poison(f"{'g' if backward else 'x'}[{m}, {c}] = {value}", clean, got, bad)
            calls += 1
        # bias
        if not backward:
            n = dc.weight_rows - 2
            b2 = ex.bias.clone()
            b2[n] = NAN
            got = _dense_call(dc, di, bias=b2, plan=plan)
            bad = torch.zeros(clean.shape, dtype=torch.bool)
            if dc.family == "experts":
                bad[di.ids.reshape(-1) == n // dc.N, n % dc.N] = True
            else:
                bad[:, n] = True
            _check_poison(f"bias[{n}] = nan", clean, got, bad)
            calls += 1
    _report(3, dc, calls + 1, (calls + 1) * clean.numel(), [], t0)


@pytest.mark.parametrize("M,family", [(1, "stream"), (13, "sm")])
@pytest.mark.parametrize("form", ["gated", "lora"])
def test_fused_forms_keep_a_non_finite_operand_in_its_row_or_column(form, M, family):
    """The gated and the LoRA epilogue on the streaming kernel (one row) and the streaming MFMA kernel (13 rows), the families the
    plain route of the shape runs: a non-finite block scale, activation or bias element stays in its own output column / row.
    Gated: weight rows 2 i and 2 i + 1 make output column i."""
    t0 = time.perf_counter()
    lib = _bnb().lib
    dc = next(d for d in C.DENSE["stream" if family == "stream" else "sm"] if d.dtype == C.BF)
    dc = C.replace(dc, M=M)
    di = C.clean_inputs(dc)
    ex = di.ex
    N, K = dc.N, dc.K
    packed = di.packed.to(DEV)
    gen = torch.Generator().manual_seed(5)
    r = 8
    lora_t = torch.randint(-2, 3, (M, r), generator=gen).to(dc.dtype).to(DEV)
    lora_b = torch.randint(-2, 3, (N, r), generator=gen).to(dc.dtype).to(DEV)

    def call(x, absmax, bias):
        if form == "gated":
            y = torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(x.to(DEV), packed, [N, K], absmax.to(DEV), dc.blocksize, "fp4", bias.to(DEV))
        else:
            y = torch.ops.bitsandbytes_amd.gemm_4bit_lora.default(x.to(DEV), packed, [N, K], absmax.to(DEV), dc.blocksize, "fp4", lora_t, lora_b, 0.5,
                                                                 bias.to(DEV))
        assert lib.bnb_mi355x_last_gemm_kernel() == C.FAMILY_ID[family]
        return y.cpu()

    clean = call(ex.x, ex.scale, ex.bias)
    assert bool(torch.isfinite(clean.float()).all())
    # the clean call itself: LoRA - float64 of the exact operands rounded once (integers and halves: every fp32 partial sum is
    # exact); gated - silu(gate) * up by torch's kernels on the T-valued reference of the plain product (tests/test_gpu_ffn.py)
    if form == "lora":
        want = (ex.x.double() @ ex.W.double().t() + ex.bias.double() + 0.5 * (lora_t.cpu().double() @ lora_b.cpu().double().t())).to(dc.dtype)
    else:
        y = ex.reference(True).to(DEV)
        want = (torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]).cpu()
    assert R.same_bits(clean, want), f"{form}: {R.first_mismatch(clean, want)}"
    col = (lambda n: n // 2) if form == "gated" else (lambda n: n)
    bpr = K // dc.blocksize
    calls = 1
    for name, b in C.poison_blocks(dc).items():
        for value in (INF, NAN):
            s = ex.scale.clone()
            s[b] = value
            bad = torch.zeros(clean.shape, dtype=torch.bool)
            bad[:, col(b // bpr)] = True
            _check_poison(f"{form} scale {name} = {value}", clean, call(ex.x, s, ex.bias), bad)
            calls += 1
    for m, c, value in C.poison_activations(dc):
        x = ex.x.clone()
        x[m, c] = value
        bad = torch.zeros(clean.shape, dtype=torch.bool)
        bad[m] = True
        _check_poison(f"{form} x[{m}, {c}] = {value}", clean, call(x, ex.scale, ex.bias), bad)
        calls += 1
    b2 = ex.bias.clone()
    b2[N - 2] = NAN
    bad = torch.zeros(clean.shape, dtype=torch.bool)
    bad[:, col(N - 2)] = True
    _check_poison(f"{form} bias = nan", clean, call(ex.x, ex.scale, b2), bad)
    _report(3, dc, calls + 1, (calls + 1) * clean.numel(), [form], t0)
