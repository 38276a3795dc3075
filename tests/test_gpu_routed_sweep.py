"""GPU (-m gpu): the BUILT-IN route of gemm_4bit and of its two neighbours, at EVERY batch size, bit for bit.

What a user gets is the route: six kernel families behind one call, chosen per call by M, N, K, blocksize, kind of statistics,
pointer alignment and CU count (backends/hip.py: fused_max_m; csrc/c_api.hip: route_to_mfma; csrc/gemm4_mfma.hip: sm_selected,
kq_selected, rt_selected, make_plan), and inside a family M picks the instance. The family tests in test_gpu_parity.py force a
family at hand-picked M under a 1e-2 norm tolerance. Here nothing is forced and nothing is tolerated: the inputs of
tests/exact_inputs.py make the float64 result the only right answer, every M from 1 to fused_max_m + 1 is run, and every output
element must equal it.

Rows above fused_max_m run dequantize + the library GEMM (bf16 / fp16 operands exact, fp32 accumulation): bit-equal as well.
"""
import ctypes as ct

import pytest
import torch

import exact_inputs as X
import routed_sweep as S
from conftest import gpu_ready
from routed_sweep import DEV, FAMILY, K_GENERIC, K_KQ, K_PC, K_RT, K_SM, K_STREAM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    # (as test_gpu_parity.py) A host without any AMD GPU device node: skip. A GPU box whose torch cannot see the device, or whose
    # native library did not load, must FAIL - never pass on a fallback.
    import os

    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    import bitsandbytes_amd as bnb

    assert bnb.lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


_RESULTS = {}


def _result(case: X.SweepCase) -> S.CaseResult:
    """One sweep per case and session (the census test at the end of the file reads them all)."""
    if case.name not in _RESULTS:
        _RESULTS[case.name] = S.run_case(case, X.SWEEP_CASES.index(case))
    return _RESULTS[case.name]


def _report(name, bad, total):
    head = f"{name}: {len(bad)} of {total} calls wrong; the first {min(len(bad), 12)}:\n  "
    return head + "\n  ".join(S.describe(name, r) for r in bad[:12])


# ------------------------------------------------------------------------------------------ 2. the routed sweep
@pytest.mark.parametrize("case", X.SWEEP_CASES, ids=lambda c: c.name)
def test_routed_gemm_4bit_is_exact_at_every_batch_size(case):
    """Every M in 1 ... fused_max_m + 1 (counted), then two batch sizes of the unfused range. Per call: the result equals the float64
    reference bit for bit; M <= fused_max_m launched a fused family and M above it launched none; where
    bnb_mi355x_gemm_4bit_route answers 0 that family is the streaming kernel, where it answers 1 one of rt / pc / kq / sm."""
    res = _result(case)
    fmax = res.fused_max
    ran = [r.M for r in res.records]
    assert ran == X.sweep_ms(fmax) and ran[: fmax + 1] == list(range(1, fmax + 2)), "a batch size of the sweep was not run"
    assert sum(1 for r in res.records if r.fused) == fmax and len(ran) >= fmax + 3
    wrong = [r for r in res.records if r.mismatch is not None]
    assert not wrong, _report(case.name, wrong, len(ran))
    for r in res.records:
        what = S.describe(case.name, r)
        if not r.fused:
            assert r.family == 0, f"{what}: a fused kernel ran above fused_max_m = {fmax}"
        elif r.route == 0:
            assert r.family == K_STREAM, f"{what}: the route query names the streaming kernel"
        else:
            assert r.family in S.MFMA_FAMILIES, f"{what}: the route query names an MFMA kernel"
    print(f"\n{case.name}: {len(ran)} calls in {res.seconds:.1f} s; {S.family_ranges(res.records)}")


def test_routed_sweep_reached_every_family_and_the_anchor_points_hold():
    """A sweep that quietly stopped reaching a family is a failure, not a pass: each of the five routed families served some M, with
    and without bias, and the points the router's own comments name hold (csrc/c_api.hip, csrc/gemm4_mfma.hip: one row = streaming
    kernel; 4096^2 at 2 ... 16 rows = streaming MFMA kernel, at 17 ... 32 = register-transposed kernel; 8192^2 from 17 rows =
    K-quarter kernel; 4096^2 at 64 rows = producer/consumer kernel, from 65 = K-quarter kernel)."""
    results = {c.name: _result(c) for c in X.SWEEP_CASES}
    seen = {(r.family, r.bias) for res in results.values() for r in res.records}
    for fam in S.ROUTED_FAMILIES:
        for b in (False, True):
            assert (fam, b) in seen, f"no call of the sweep ran the {FAMILY[fam]} kernel {'with' if b else 'without'} bias"
    assert (0, False) in seen and (0, True) in seen
    fam = {name: {r.M: r.family for r in res.records} for name, res in results.items()}
    for name, res in results.items():
        assert fam[name][1] == K_STREAM, (name, "one row")
    sq = fam["4096x4096"]
    assert all(sq[m] == K_SM for m in range(2, 17)) and all(sq[m] == K_RT for m in range(17, 33)), "4096^2: sm to 16 rows, rt to 32"
    assert sq[64] == K_PC and all(sq[m] == K_KQ for m in range(65, 641)), "4096^2: pc at 64 rows, kq from 65"
    big = fam["8192x8192"]
    assert all(big[m] == K_SM for m in range(2, 17)) and all(big[m] == K_KQ for m in range(17, 513)), "8192^2: kq from 17 rows"
    assert all(fam["11008x4096-nested"][m] == K_KQ for m in range(17, 513)), "nested blocksize-64 statistics: kq from 17 rows"
    assert all(f == K_PC for m, f in fam["5120x5120-bs128-nested"].items() if 17 <= m <= 512), "nested blocksize 128: pc, not kq"
    assert all(fam["4096x2752"][m] == K_SM for m in range(2, 129)), "K % 256 != 0: sm row passes to 128"
    assert all(fam["96x2752-nested"][m] == K_STREAM for m in range(1, 17)), "below SM_MIN_ROWS: the streaming kernel"
    assert all(fam["4096x4096-bs32"][m] == K_RT for m in range(5, 129)), "blocksize 32: the rt kernel's BS32 instances"
    assert all(fam["4096x4096-fp32"][m] == K_STREAM for m in range(1, 5)), "fp32 activations: the streaming kernel to 4 rows"
    total = sum(len(res.records) for res in results.values())
    print(f"\nrouted sweep: {total} calls over {len(results)} cases, {sum(res.seconds for res in results.values()):.1f} s")


# ------------------------------------------------------------------------------------------ 3a. the fused backward
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("N,K", [(4096, 4096), (1088, 256), (1216, 384)], ids=lambda v: str(v))
def test_fused_backward_is_exact_at_every_batch_size(N, K, nested):
    """bitsandbytes_amd::gemm_4bit_grad_input at every M from 1 to 130 (fused to 128 rows: one, two and four row tiles per workgroup,
    two 64-row passes, N slices and their workspace; 129 and 130 run dequantize + matmul) against the float64 g @ W of integer
    gradients. 1216 x 384: 19 blocks of 64 n, three 128-column workgroups - no power of two anywhere."""
    from bitsandbytes_amd.backends import hip

    rows = 130
    ex = X.build(N, K, 64, torch.bfloat16, nested, seed=N + K + nested, rows=2)
    g, ref = X.grad_inputs(ex, rows + 3, seed=N * 3 + K)
    packed = X.check_quantization(ex, S.gpu_ops(), DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    g, ref = g.to(DEV), ref.to(DEV)
    wrong = []
    for M in range(1, rows + 1):
        assert hip.grad_input_fused_ok(torch.bfloat16, M, N, K, 64) == (M <= hip.FUSED_BACKWARD_MAX_M), M
        y = torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default(g[:M], packed, [N, K], absmax, 64, "fp4", a8, code, off)
        assert y.shape == (M, K) and y.dtype == torch.bfloat16
        if not torch.equal(y, ref[:M]):
            wrong.append((M, X.first_mismatch(y.cpu(), ref[:M].cpu())))
    assert not wrong, f"{N} x {K} nested={nested}: {len(wrong)} of {rows} batch sizes wrong; (M, (row, column, got, want)): {wrong[:12]}"


# ------------------------------------------------------------------------------------------ 3b. the grouped call
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("heights", [(4096, 4096, 4096, 4096), (5504, 2752)], ids=["qkvo", "gate-up"])
def test_grouped_call_is_exact_at_every_batch_size(heights, nested):
    """bnb_mi355x_gemm_4bit_grouped (backends/hip.py: gemm_4bit_grouped) on members that share x, every M from 1 to 66 - one launch
    of the streaming kernel at one row, of the streaming MFMA kernel up to 64 rows (its 32-row instances from 17), member by member
    above - each member against ITS OWN float64 reference (the grouped tests of test_gpu_parity.py compare the group with separate
    calls of the same library). Members differ in weights, scales and bias; bias on alternating members and batch sizes."""
    from bitsandbytes_amd.backends import hip

    K, rows = 4096, 66
    lib = _lib()
    gen = torch.Generator().manual_seed(len(heights) + nested)
    x = X.int_rows(rows + 3, K, torch.bfloat16, gen)
    members = []
    for i, N in enumerate(heights):
        ex = X.build(N, K, 64, torch.bfloat16, nested, seed=1000 + 17 * i + N + nested, rows=2)
        X.assert_exact_sums(ex.W, x, ex.unit, torch.bfloat16, extra=float(X.BIAS_MAX))
        ex.x = x
        packed = X.check_quantization(ex, S.gpu_ops(), DEV)
        members.append((ex, packed, ex.stats_args(DEV), ex.bias.to(DEV), {b: ex.reference(b).to(DEV) for b in (False, True)}))
    xd = x.to(DEV)
    ns = (ct.c_int * len(heights))(*heights)
    sentinel = S.Sentinel(K_GENERIC)
    wrong, routes = [], {}
    for M in range(1, rows + 1):
        with_bias = [(M + i) % 2 == 0 for i in range(len(heights))]
        mats = [(packed, (ex.N, K), st[0], bias if wb else None, st[1], st[2], st[3])
                for (ex, packed, st, bias, _), wb in zip(members, with_bias)]
        route = lib.bnb_mi355x_gemm_4bit_grouped_route(2, len(heights), ns, M, K, 64)
        sentinel()
        ys = hip.gemm_4bit_grouped(xd[:M], mats, 64, "fp4")
        family = lib.bnb_mi355x_last_gemm_kernel()
        routes[M] = (route, family)
        assert family in S.ROUTED_FAMILIES, (M, "the grouped call launched no fused kernel")
        if route == 2:
            assert family == K_SM, (M, FAMILY[family])
        if route == 1:
            assert family == K_STREAM, (M, FAMILY[family])
        for i, (y, (ex, _, _, _, ref), wb) in enumerate(zip(ys, members, with_bias)):
            want = ref[wb][:M]
            assert y.shape == want.shape and y.dtype == want.dtype
            if not torch.equal(y, want):
                wrong.append((M, i, FAMILY[family], route, X.first_mismatch(y.cpu(), want.cpu())))
    assert not wrong, f"{heights} nested={nested}: {len(wrong)} wrong; (M, member, family, grouped route, (row, column, got, want)): {wrong[:12]}"
    assert routes[1][0] == 1 and all(routes[m][0] == 2 for m in range(2, 65)) and all(routes[m][0] == 0 for m in (65, 66)), routes


@pytest.mark.parametrize("heights", [(4096, 4096, 4096, 4096), (5504, 2752)], ids=["qkvo", "gate-up"])
def test_linear4bit_group_forward_is_exact_at_every_batch_size(heights):
    """The same groups as Linear4bit layers through nn.linear4bit_group_forward - from the second call on ONE native call on the
    layers' prepared handles (csrc/torch_dispatch.cpp: linear4bit_group_prepared) -, every M from 1 to 66, each layer against its own
    float64 reference. Plain statistics (the layers quantize their weights themselves: absmax must come out as the intended scales);
    bias on every other layer."""
    import bitsandbytes_amd.nn as bnn

    K, rows = 4096, 66
    gen = torch.Generator().manual_seed(50 + len(heights))
    x = X.int_rows(rows + 3, K, torch.bfloat16, gen)
    layers, refs = [], []
    for i, N in enumerate(heights):
        ex = X.build(N, K, 64, torch.bfloat16, False, seed=2000 + 13 * i + N, rows=2)
        X.assert_exact_sums(ex.W, x, ex.unit, torch.bfloat16, extra=float(X.BIAS_MAX))
        ex.x = x
        layer = bnn.Linear4bit(K, N, bias=i % 2 == 0, compute_dtype=torch.bfloat16, quant_type="fp4", compress_statistics=False)
        layer.weight = bnn.Params4bit(ex.W, requires_grad=False, quant_type="fp4", compress_statistics=False, blocksize=64, module=layer)
        if layer.bias is not None:
            layer.bias.data = ex.bias.clone()
        layer = layer.to(DEV)
        st = layer.weight.quant_state
        assert torch.equal(st.absmax.cpu(), ex.scale), "the layer's quantizer did not return the intended scales"
        back = torch.ops.bitsandbytes.dequantize_4bit.default(layer.weight.data, st.absmax, 64, "fp4", [N, K], torch.bfloat16)
        assert torch.equal(back.cpu().view(torch.uint8), ex.W.view(torch.uint8))
        layers.append(layer)
        refs.append(ex.reference(i % 2 == 0).to(DEV))
    xd = x.to(DEV)
    wrong = []
    with torch.no_grad():
        for _ in range(2):
            bnn.linear4bit_group_forward(layers, xd[:3])
        assert all(layer._prepared is not None for layer in layers), "the layers hold no prepared call: the native group call is not what ran"
        for M in range(1, rows + 1):
            xm = xd[:M] if M % 3 else xd[:M].view(1, M, K)   # (a leading batch dimension on every third call)
            ys = bnn.linear4bit_group_forward(layers, xm)
            family = _lib().bnb_mi355x_last_gemm_kernel()
            for i, (y, ref) in enumerate(zip(ys, refs)):
                y = y.reshape(M, -1)
                assert y.shape == ref[:M].shape and y.dtype == ref.dtype
                if not torch.equal(y, ref[:M]):
                    wrong.append((M, i, FAMILY.get(family, family), X.first_mismatch(y.cpu(), ref[:M].cpu())))
    assert not wrong, f"{heights}: {len(wrong)} wrong; (M, layer, family of the last launch, (row, column, got, want)): {wrong[:12]}"


# ------------------------------------------------------------------------------------------ 4. operand placement
_PLACEMENTS = ("x+2", "weight+1", "weight+8", "absmax+4", "bias+2", "codes+1", "x-transposed", "x-3d")


def _off(t: torch.Tensor, elements: int) -> torch.Tensor:
    """The same values in a view that starts ``elements`` elements behind the start of a fresh allocation."""
    flat = t.contiguous().flatten()
    buf = torch.empty(flat.numel() + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[elements:elements + flat.numel()]
    view.copy_(flat)
    return view.view(t.shape)


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_operand_placement_keeps_the_result_exact(nested):
    """Every *_supported predicate tests pointer alignment and falls back; here the matmul is handed such pointers. 4096 x 4096, M in
    {1, 2, 8, 16, 17, 64, 65, 200}: x 2 bytes off a 16-byte boundary, the packed weight 1 and 8 bytes off, the fp32 statistics 4 bytes
    off, the bias 2 bytes off, the nested codes 1 byte off, a transposed and a 3-D x. The result stays bit-equal to the float64
    reference, and the family that ran is not one whose predicate demands the alignment that was broken: x or the weight off 16
    bytes leaves the scalar kernel alone (csrc/gemv4_stream.hip: stream_ok), the weight 8 bytes off also the producer/consumer kernel
    (csrc/gemm4_mfma.hip: gemm_4bit_mfma_supported), misaligned nested codes keep the K-quarter kernel out (gemm_4bit_kq_serves)."""
    lib = _lib()
    N = K = 4096
    Ms = (1, 2, 8, 16, 17, 64, 65, 200)
    ex = X.build(N, K, 64, torch.bfloat16, nested, seed=77 + nested, rows=max(Ms))
    packed = X.check_quantization(ex, S.gpu_ops(), DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    x, bias = ex.x.to(DEV), ex.bias.to(DEV)
    ref = ex.reference(True).to(DEV)
    sentinels = {K_GENERIC: S.Sentinel(K_GENERIC), K_STREAM: S.Sentinel(K_STREAM)}
    all_fused = set(S.ROUTED_FAMILIES)
    wrong, ran = [], {}
    for place in _PLACEMENTS:
        if place == "codes+1" and not nested:
            continue
        for M in Ms:
            xa, Ba, sa, ba, ca = x[:M], packed, absmax, bias, a8
            allowed, align = all_fused, None
            if place == "x+2":
                xa, allowed, align = _off(xa, 1), {K_GENERIC}, (lambda: xa.data_ptr() % 16 == 2)
            elif place == "weight+1":
                Ba, allowed, align = _off(packed, 1), {K_GENERIC}, (lambda: Ba.data_ptr() % 16 == 1)
            elif place == "weight+8":
                Ba, allowed, align = _off(packed, 8), {K_GENERIC, K_PC}, (lambda: Ba.data_ptr() % 16 == 8)
            elif place == "absmax+4":
                sa, align = _off(absmax, 1), (lambda: sa.data_ptr() % 16 == 4)
            elif place == "bias+2":
                ba, align = _off(bias, 1), (lambda: ba.data_ptr() % 16 == 2)
            elif place == "codes+1":
                ca, allowed, align = _off(a8, 1), all_fused - {K_KQ}, (lambda: ca.data_ptr() % 4 == 1)
            elif place == "x-transposed":
                xa = xa.t().contiguous().t()
                assert M == 1 or not xa.is_contiguous()
            elif place == "x-3d":
                xa = xa.view(2, M // 2, K) if M % 2 == 0 else xa.view(1, M, K)
            assert align is None or align(), (place, "the view is not placed as intended")
            sentinel = sentinels[K_STREAM if K_GENERIC in allowed else K_GENERIC]   # (a family the call may not take)
            sentinel()
            y = torch.ops.bitsandbytes.gemm_4bit.default(xa, Ba, [N, K], sa, 64, "fp4", ba, ca, code, off)
            family = lib.bnb_mi355x_last_gemm_kernel()
            ran[(place, M)] = FAMILY.get(family, family)
            assert family in allowed, f"{place} M={M}: the {FAMILY.get(family, family)} kernel ran (the sentinel was {FAMILY[sentinel.family]}), allowed: {sorted(FAMILY[f] for f in allowed)}"
            y = y.reshape(M, N)
            if not torch.equal(y, ref[:M]):
                wrong.append((place, M, FAMILY.get(family, family), X.first_mismatch(y.cpu(), ref[:M].cpu())))
    assert not wrong, f"nested={nested}: {len(wrong)} wrong; (placement, M, family, (row, column, got, want)): {wrong[:12]}"
    print("\nfamilies by placement:", {p: [ran[(p, m)] for m in Ms] for p in _PLACEMENTS if (p, Ms[0]) in ran})
