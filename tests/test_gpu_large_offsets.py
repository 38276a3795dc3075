"""GPU (-m gpu): the 4-bit matmuls on weights past the 2^31 and 2^32 ELEMENT offsets, bit for bit on the whole output.

Every other matmul test runs on at most 5 * 10^8 weight elements; the kernels address weights and block statistics with mixed 32- and
64-bit arithmetic, and their size limits sit in host predicates (tests/test_large_offsets_host.py asserts those). Here the operands
of tests/large_offset_cases.py - packed bytes and statistics written in place, exact by construction, a scale pattern that no
power-of-two shift maps onto itself - go through the PUBLIC calls at the cases around 2^31 and 2^32 elements, and every output element
must equal the float64 reference: a tile index that lost a high bit shows as wrong rows at the far end of the layer.

A weight is built once per case and dropped when the next case is asked for (about 2.3 GiB of bytes, up to 1.3 GiB of statistics and
0.5 GiB of reference chunks at a time). The module skips under 16 GiB of free device memory, as test_quantize_4bit_maximum_size does.
"""
import os
import time

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import large_offset_cases as L
import lora_cases as LC
import routed_sweep as S
from conftest import gpu_ready
from routed_sweep import DEV, FAMILY, K_GENERIC, K_KQ, K_RT, K_SM, K_STREAM

pytestmark = pytest.mark.gpu

_CACHE = {}      # the case that is resident: {"name": ..., (dtype, nested, blocksize): Built}
_LEDGER = []     # (test, case, elements, M, family, seconds, peak GiB)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_native_lib_and_memory():
    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    assert _bnb().lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of free device memory")
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _built(case: L.LargeCase, dtype=torch.bfloat16, nested=False, with_reference=True) -> L.Built:
    """The case on the device: one set of packed bytes per case, shared by its kinds of statistics; another case evicts it."""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        torch.cuda.empty_cache()
        _CACHE["name"] = case.name
    key = (dtype, nested, case.blocksize, with_reference)
    if key not in _CACHE:
        full = _CACHE.get((dtype, nested, case.blocksize, True))
        _CACHE[key] = full or L.build(case, DEV, dtype, nested, packed=_CACHE.get("packed"), with_reference=with_reference)
        _CACHE["packed"] = _CACHE[key].packed
    return _CACHE[key]


def _state(b: L.Built, N=None):
    """The QuantState the public functions take, on the first ``N`` rows."""
    Fn = _bnb().functional
    N = N or b.case.N
    bpr = b.case.K // b.case.blocksize
    shape = torch.Size((N, b.case.K))
    code4 = Fn.get_4bit_type("fp4", device=DEV)
    if b.nested:
        state2 = Fn.QuantState(absmax=b.nest.absmax2, code=b.nest.absmax_code, blocksize=256, dtype=torch.float32)
        return Fn.QuantState(absmax=b.nest.absmax_8bit[:N * bpr], shape=shape, code=code4, blocksize=b.case.blocksize, quant_type="fp4",
                             dtype=b.dtype, offset=b.nest.offset, state2=state2)
    return Fn.QuantState(absmax=b.scale[:N * bpr], shape=shape, code=code4, blocksize=b.case.blocksize, quant_type="fp4", dtype=b.dtype)


class _Timer:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.time()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.seconds = time.time() - self.t0
        self.peak = torch.cuda.max_memory_allocated() / 2 ** 30


def _note(test, case, M, family, t):
    _LEDGER.append((test, case.name, case.elements, M, family, t.seconds, t.peak))
    print(f"[large-offsets] {test} {case.name} M={M}: family {FAMILY.get(family, family)}, {t.seconds:.3f} s, peak {t.peak:.2f} GiB allocated")


_SENTINELS = {}


def _sentinel(family):
    if family not in _SENTINELS:
        _SENTINELS[family] = S.Sentinel(family)
    return _SENTINELS[family]


# ------------------------------------------------------------------------------------------ plain gemm_4bit
def _run_plain(test, case, dtype, nested, Ms):
    """gemm_4bit through the public op at every M: the whole output against the reference, bit for bit; the family that ran is the one
    the route query names. At and past 2^32 elements the call is either bit-exact or raises ValueError - a silently different result
    is the failure this module exists for, and the message names the first wrong weight row (a block index wrapped at 32 bits goes
    wrong from row 2^32 / K on). Below it a refusal is accepted only from the unfused route (dequantize stops at 2^31 - 1 elements)."""
    from bitsandbytes_amd.backends import hip

    lib = _bnb().lib
    b = _built(case, dtype, nested)
    N, K, bs = case.N, case.K, case.blocksize
    absmax, a8, code, off = b.stats_args()
    past32 = case.elements >= 2 ** 32
    wrong, refused, misrouted = [], [], []
    for M in Ms:
        with_bias = M % 3 != 2
        route = 0 if (bs == 32 and nested) else lib.bnb_mi355x_gemm_4bit_route(0, L.DT_CODE[dtype], M, N, K, bs)
        expect = (K_GENERIC if past32 else K_STREAM) if route == 0 else None
        sentinel = _sentinel(K_STREAM if expect == K_GENERIC else K_GENERIC)
        sentinel()
        with _Timer() as t:
            try:
                y = torch.ops.bitsandbytes.gemm_4bit.default(b.x[:M], b.packed.view(-1, 1), [N, K], absmax, bs, "fp4",
                                                             b.bias if with_bias else None, a8, code, off)
            except ValueError as exc:
                y = None
                refused.append((M, str(exc)))
        family = lib.bnb_mi355x_last_gemm_kernel()
        if y is None:
            assert past32 or M > hip.fused_max_m(N, K, bs, nested), f"{case.name} M={M}: the fused route refused: {refused[-1][1]}"
            _note(test, case, M, 0, t)
            continue
        _note(test, case, M, family, t)
        if family == sentinel.family:
            misrouted.append(f"M={M}: no fused kernel was launched")
        elif route == 0 and family != expect:
            misrouted.append(f"M={M}: route 0 names the {FAMILY[expect]} kernel, the {FAMILY.get(family, family)} kernel ran")
        elif route == 1 and family not in S.MFMA_FAMILIES:
            misrouted.append(f"M={M}: route 1 names an MFMA kernel, the {FAMILY.get(family, family)} kernel ran")
        want = b.ref[with_bias][:M]
        assert y.shape == want.shape and y.dtype == want.dtype
        if not torch.equal(y, want):
            n, m, got, ref = L.first_wrong_row(y, want)
            rows_wrong = int((y != want).any(dim=0).sum())
            wrong.append(f"M={M} family={FAMILY.get(family, family)}: first wrong weight row {n} (2^31 / K = {2 ** 31 // K}, 2^32 / K = {2 ** 32 // K}; "
                         f"activation row {m}: got {got!r}, want {ref!r}), {rows_wrong} of {N} rows wrong")
    assert not wrong, f"{case.name} dtype={dtype} nested={nested}: silently wrong results\n  " + "\n  ".join(wrong)
    assert not misrouted, f"{case.name} dtype={dtype} nested={nested}:\n  " + "\n  ".join(misrouted)
    return refused


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_gemm_4bit_is_exact_on_the_whole_output(case):
    """bf16, plain statistics, M in {1, 2, 4, 8, 16, 17, 64}; bias on two calls of three."""
    _run_plain("plain", case, torch.bfloat16, False, L.MS)


@pytest.mark.parametrize("kind", ["fp16", "nested"])
@pytest.mark.parametrize("name", ["below32", "above32"])
def test_gemm_4bit_fp16_and_nested_statistics(name, kind):
    """The f16 instances and the nested statistics (second-level group indices e0 / e1) at M in {1, 4, 16} on either side of 2^32."""
    dtype, nested = (torch.float16, False) if kind == "fp16" else (torch.bfloat16, True)
    _run_plain(kind, L.CASE[name], dtype, nested, (1, 4, 16))


def test_gemm_4bit_blocksize_32_reaches_the_register_transposed_kernel():
    """Past 2^31 elements the built-in route reaches the rt family only through its BS32 instances (the K-quarter kernel stops at 2^31,
    rt_selected at 96 M weights): below32 at blocksize 32, M in {1, 8, 17} - twice as many blocks, the block index just under 2^27."""
    _run_plain("bs32", L.BELOW32_BS32, torch.bfloat16, False, (1, 8, 17))
    assert {r[4] for r in _LEDGER if r[0] == "bs32" and r[3] in (8, 17)} == {K_RT}


# ------------------------------------------------------------------------------------------ fused epilogues on below32
def _matmul64(b: L.Built, rows: int, N: int) -> torch.Tensor:
    """float64 ``x[:rows] @ W[:N].T + bias`` of the constructed operands, unrounded, [rows, N]."""
    K, bs = b.case.K, b.case.blocksize
    xt = b.x[:rows].double().t().contiguous()
    out = torch.empty((rows, N), dtype=torch.float64, device=DEV)
    step = max(1, (1 << 24) // K)
    for r0 in range(0, N, step):
        r1 = min(N, r0 + step)
        out[:, r0:r1] = (L.rows64(b.packed, b.scale, K, bs, r0, r1) @ xt).t() + b.bias[r0:r1].double()
    return out


@pytest.mark.parametrize("M", [1, 4])
def test_gated_epilogue_on_below32(M):
    """matmul_4bit_gated on the first 524286 rows read as (gate, up) pairs: the bits of F.silu(g) * u of the plain call's halves (the
    documented identity; the plain call is the reference, which the test above holds it to). One row: the streaming kernel's gated
    instance; four: the streaming MFMA kernel's."""
    bnb = _bnb()
    case = L.CASE["below32"]
    b = _built(case)
    N = case.N - 1
    state = _state(b, N)
    packed = b.packed[:N * case.K // 2]
    from bitsandbytes_amd.backends import hip

    assert hip.gemm_4bit_gated_supported(torch.bfloat16, M, N, case.K, 64), "the fused gated launch serves this cell"
    _sentinel(K_GENERIC)()
    with _Timer() as t:
        y = bnb.matmul_4bit_gated(b.x[:M], packed, state, bias=b.bias[:N])
    family = bnb.lib.bnb_mi355x_last_gemm_kernel()
    _note("gated", case, M, family, t)
    assert family == (K_STREAM if M == 1 else K_SM)
    plain = b.ref[True][:M, :N]
    want = TF.silu(plain[:, 0::2]) * plain[:, 1::2]
    assert y.shape == (M, N // 2) and y.dtype == torch.bfloat16
    assert torch.equal(y, want), f"first wrong (pair, row, got, want): {L.first_wrong_row(y, want)}"


@pytest.mark.parametrize("M", [1, 4])
def test_lora_epilogues_on_below32(M):
    """matmul_4bit_lora (r = 16) and matmul_4bit_lora_ids (3 adapters, ids {0, 2, -1, 1}: lora_b rebased per adapter, N r and M N past
    2^22) against float64 ``x W^T + bias + s t B_l^T`` within lora_cases.tolerance per element; a row without an adapter is the plain
    row bit for bit."""
    bnb = _bnb()
    case = L.CASE["below32"]
    b = _built(case)
    N, K, r = case.N, case.K, 16
    state = _state(b)
    gen = torch.Generator().manual_seed(77)
    values = torch.tensor(LC.B_VALUES, dtype=torch.float32)
    t_rows = torch.randint(-LC.T_MAX, LC.T_MAX + 1, (4, r), generator=gen).to(torch.bfloat16).to(DEV)
    stack = values[torch.randint(0, len(LC.B_VALUES), (3, N, r), generator=gen)].to(torch.bfloat16).to(DEV)
    scalings = torch.tensor([0.5, 2.0, 1.0], dtype=torch.float32, device=DEV)
    y64 = _matmul64(b, M, N)
    plain = b.ref[True][:M]
    assert torch.equal(y64.to(torch.bfloat16), plain)
    expect_family = K_STREAM if M == 1 else K_SM
    # one adapter
    _sentinel(K_GENERIC)()
    with _Timer() as t:
        y = bnb.matmul_4bit_lora(b.x[:M], b.packed, state, t_rows[:M], stack[1], 2.0, bias=b.bias)
    family = bnb.lib.bnb_mi355x_last_gemm_kernel()
    _note("lora", case, M, family, t)
    assert family == expect_family
    want64 = y64 + LC.adapter_term64(t_rows[:M], stack[1], 2.0)
    err = (y.double() - want64).abs()
    tol = LC.tolerance(want64, plain, t_rows[:M], stack[1], 2.0, torch.bfloat16)
    print(f"[large-offsets] lora M={M}: largest error / tolerance {float((err / tol).max()):.3f}")
    assert y.shape == (M, N) and bool((err <= tol).all()), f"first element outside the tolerance: {L.first_wrong_row(err <= tol, torch.ones_like(err, dtype=torch.bool))}"
    # an adapter id per row
    vals = [0, 2, -1, 1][:M] if M > 1 else [2]
    for idt in (torch.int32, torch.int64):
        ids = torch.tensor(vals, dtype=idt, device=DEV)
        _sentinel(K_GENERIC)()
        with _Timer() as t:
            y = bnb.matmul_4bit_lora_ids(b.x[:M], b.packed, state, t_rows[:M], stack, scalings, ids, bias=b.bias)
        family = bnb.lib.bnb_mi355x_last_gemm_kernel()
        _note("lora_ids", case, M, family, t)
        assert family == expect_family and y.shape == (M, N)
        for m, i in enumerate(vals):
            if i < 0:
                assert torch.equal(y[m], plain[m]), f"row {m} has no adapter: the plain row"
                continue
            s = float(scalings[i])
            want64 = y64[m:m + 1] + LC.adapter_term64(t_rows[m:m + 1], stack[i], s)
            err = (y[m:m + 1].double() - want64).abs()
            tol = LC.tolerance(want64, plain[m:m + 1], t_rows[m:m + 1], stack[i], s, torch.bfloat16)
            assert bool((err <= tol).all()), f"row {m} adapter {i}: first column outside the tolerance {int((err > tol).nonzero()[0, 1])}"


# ------------------------------------------------------------------------------------------ the fused backward
@pytest.mark.parametrize("M", [8, 128])
@pytest.mark.parametrize("name", ["mid", "below32"])
def test_grad_input_across_the_offsets(name, M):
    """gemm_4bit_grad_input contracts over N. The kernel takes whole 64-row groups only (N % 64 == 0: the ledger of the host test), so
    it runs on the first N & ~63 rows of the case - 3 * 2^30 elements for mid, 2^32 - 63 rows for below32. Integer gradients with 64
    nonzero columns per row, drawn from the first, a middle and the last 64-row group and from the groups around rows 2^31 / K and
    2^32 / K - 1 where the weight reaches them; the exact-sum bound of the transposed product is asserted over those rows (the others
    contribute exact zeros), and the result equals float64 ``g @ W`` over them, bit for bit."""
    from bitsandbytes_amd.backends import hip

    case = L.CASE[name]
    b = _built(case, with_reference=False)
    K, bs = case.K, case.blocksize
    N = case.N & ~63
    assert hip.grad_input_fused_ok(torch.bfloat16, M, N, K, bs), "the fused backward serves this cell"
    starts = {0, (N // 2) & ~63, N - 64}
    for row in (2 ** 31 // K, 2 ** 32 // K - 1):
        if row - 32 >= 0 and row + 32 <= N:
            starts.add(row - 32)
        elif row < N + 64:
            starts.add(N - 64)
    cols = torch.cat([torch.arange(s, s + 64) for s in sorted(starts)]).unique()
    gen = torch.Generator().manual_seed(N + M)
    g = torch.zeros((M, N), dtype=torch.bfloat16)
    for m in range(M):
        pick = cols[torch.randperm(cols.numel(), generator=gen)[:64]]
        v = torch.randint(1, X.X_MAX + 1, (64,), generator=gen) * (2 * torch.randint(0, 2, (64,), generator=gen) - 1)
        g[m, pick] = v.to(torch.bfloat16)
    assert torch.unique(g[:, cols], dim=0).shape[0] == M and int((g != 0).sum(dim=1).max()) <= 64
    w64 = L.gather_rows64(b.packed, b.scale, K, bs, cols)
    bound = X.assert_exact_sums(w64.cpu().to(torch.bfloat16), g[:, cols], b.unit, torch.bfloat16, transposed=True)
    want = (g[:, cols].to(DEV).double() @ w64).to(torch.bfloat16)
    gd = g.to(DEV)
    with _Timer() as t:
        y = torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(gd, b.packed[:N * K // 2].view(-1, 1), [N, K], b.scale[:N * K // bs], bs, "fp4",
                                                                    None, None, None)
    _note("grad_input", case, M, -1, t)
    print(f"[large-offsets] grad_input {name} M={M}: {cols.numel()} weight rows in groups at {sorted(starts)}, sum of |products| <= {bound}")
    assert y.shape == (M, K) and y.dtype == torch.bfloat16
    assert torch.equal(y, want), f"first wrong (column k, gradient row, got, want): {L.first_wrong_row(y, want)}"


# ------------------------------------------------------------------------------------------ the expert stack
_EXPERT_IDS = (0, 255, 256, 511, 512, 519, -1)   # the experts on either side of the 2^31 and 2^32 element offsets, the last one, none


@pytest.mark.parametrize("gated", ["none", "chunked"])
@pytest.mark.parametrize("P", [5, 65])
def test_experts_on_a_stack_past_2_32(P, gated):
    """matmul_4bit_experts on 520 experts of 1024 x 8192 (2^32 elements plus 8 experts), flat ids drawn from _EXPERT_IDS, int32 and
    int64: every row equals the float64 reference of its expert's rows bit for bit (zeros for id -1); gated-chunked: F.silu(g) * u of
    the plain result's halves."""
    bnb = _bnb()
    case = L.EXPERTS
    b = _built(case, with_reference=False)
    E, N, K = L.EXPERTS_E, L.EXPERTS_N, L.EXPERTS_K
    assert bnb.lib.bnb_mi355x_gemm_4bit_experts_supported(2, E, N, K, 64) == 1
    Fn = bnb.functional
    state = Fn.QuantState(absmax=b.scale, shape=torch.Size((E, N, K)), code=Fn.get_4bit_type("fp4", device=DEV), blocksize=64, quant_type="fp4",
                          dtype=torch.bfloat16)
    ids = [_EXPERT_IDS[(3 * p + p // 7) % len(_EXPERT_IDS)] for p in range(P)] if P >= len(_EXPERT_IDS) else list(_EXPERT_IDS[-P:])
    assert set(ids) == set(_EXPERT_IDS[-P:])
    x = L.int_rows(P, K, torch.bfloat16, 900 + P, DEV)
    bias = b.bias.view(E, N)
    plain = torch.zeros((P, N), dtype=torch.bfloat16, device=DEV)
    for e in sorted(set(ids) - {-1}):
        rows = [p for p, i in enumerate(ids) if i == e]
        w64 = L.rows64(b.packed, b.scale, K, 64, e * N, (e + 1) * N)
        X.assert_exact_sums(w64.cpu().to(torch.bfloat16), x[rows].cpu(), b.unit, torch.bfloat16, extra=float(X.BIAS_MAX))
        plain[rows] = (x[rows].double() @ w64.t() + bias[e].double()).to(torch.bfloat16)
    want = plain if gated == "none" else TF.silu(plain[:, :N // 2]) * plain[:, N // 2:]
    for idt in (torch.int32, torch.int64):
        idd = torch.tensor(ids, dtype=idt, device=DEV)
        with _Timer() as t:
            y = bnb.matmul_4bit_experts(x, b.packed, state, idd, bias=bias, gated=gated)
        family = bnb.lib.bnb_mi355x_last_gemm_kernel()
        _note(f"experts-{gated}", case, P, family, t)
        assert family == 9 and y.shape == want.shape and y.dtype == torch.bfloat16
        if not torch.equal(y, want):
            bad = sorted({ids[p] for p in (y != want).any(dim=1).nonzero().flatten().tolist()})
            raise AssertionError(f"experts {bad} wrong; first (column, row, got, want): {L.first_wrong_row(y, want)}")


# ------------------------------------------------------------------------------------------ dequantize_4bit_rows
def test_dequantize_rows_of_the_above32_table():
    """dequantize_4bit_rows on the above32 bytes in bf16: row 0, the rows on either side of 2^31 / K and 2^32 / K and the last row; then
    70 000 indices (the launcher's passes of 65 535 rows). int32 and int64 indices; bit-equal to the constructed W rows."""
    case = L.CASE["above32"]
    b = _built(case, with_reference=False)
    N, K, bs = case.N, case.K, case.blocksize
    op = torch.ops.bitsandbytes_amd.dequantize_4bit_rows.default
    edge = [0, 2 ** 31 // K - 1, 2 ** 31 // K, 2 ** 32 // K - 1, 2 ** 32 // K, N - 1]
    gen = torch.Generator().manual_seed(3)
    many = torch.cat([torch.tensor(edge), torch.randint(0, N, (70000 - len(edge),), generator=gen)])
    many = many[torch.randperm(many.numel(), generator=gen)]
    for idt in (torch.int32, torch.int64):
        for rows in (torch.tensor(edge), many):
            idx = rows.to(idt).to(DEV)
            with _Timer() as t:
                y = op(b.packed.view(-1, 1), b.scale, idx, K, bs, "fp4", torch.bfloat16)
            _note(f"rows-{rows.numel()}", case, rows.numel(), -1, t)
            assert y.shape == (rows.numel(), K) and y.dtype == torch.bfloat16
            for c0 in range(0, rows.numel(), 4096):
                w64 = L.gather_rows64(b.packed, b.scale, K, bs, rows[c0:c0 + 4096])
                want = w64.to(torch.bfloat16)
                assert torch.equal(want.double(), w64)
                got = y[c0:c0 + 4096]
                if not torch.equal(got, want):
                    r = int((got != want).any(dim=1).nonzero()[0, 0])
                    raise AssertionError(f"{idt}: output row {c0 + r} = weight row {int(rows[c0 + r])} differs from the constructed W")


# ------------------------------------------------------------------------------------------ the census
def test_every_family_ran_past_2_31_elements():
    """Runs last: across the module the streaming kernel (1), the register-transposed or the K-quarter kernel (3 or 6) and the streaming
    MFMA kernel (7) each served a call on more than 2^31 elements - and, as the route stands, the producer/consumer kernel (4, the
    17- and 64-row calls between 2^31 and 2^32) and the generic kernel (2, everything from 2^32 on)."""
    past = {r[4] for r in _LEDGER if r[2] > 2 ** 31}
    below = {r[4] for r in _LEDGER if r[2] <= 2 ** 31}
    print("\n[large-offsets] families past 2^31 elements:", sorted(str(FAMILY.get(f, f)) for f in past if f > 0),
          "; on below31:", sorted(str(FAMILY.get(f, f)) for f in below if f > 0))
    for test, name, elements, M, family, seconds, peak in _LEDGER:
        print(f"[large-offsets] {test:16s} {name:13s} M={M:<6d} {str(FAMILY.get(family, family)):8s} {seconds:8.3f} s  {peak:6.2f} GiB")
    assert K_STREAM in past and K_SM in past and (K_RT in past or K_KQ in past), sorted(past)
    assert K_KQ in below, "below31 at 17 and 64 rows: the K-quarter kernel's last shape"
    assert S.K_PC in past and K_GENERIC in past
    assert all(r[4] == K_GENERIC for r in _LEDGER if r[2] >= 2 ** 32 and r[0] in ("plain", "fp16", "nested")), "past 2^32: the generic kernel alone"
