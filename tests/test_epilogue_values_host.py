"""CPU (-m "not gpu"): the preconditions of every sweep tests/test_gpu_epilogue_values.py runs (tests/epilogue_value_cases.py) - the
comparison rule, single rounding from float64, coverage of the pattern sweeps, the hand-packed weights through the oracle's
dequantizer, the CPU measurement behind the activation's anchor, representability of the rounding cases, and the teeth of the LoRA case.

The CPU measurement (torch's CPU kernels): ``F.silu`` on T equals the fp32 sequence ``T(g / (1 + exp(-g)))`` at all 65536 patterns of
both types; that sequence differs from float64 rounded ONCE at 17 bf16 patterns (g = -89.0, -89.5 ... -97.0: exp(-g) overflows fp32
and the quotient is -0 - the derived exception) and at one fp16 pattern, g = 2^-24 (1 + exp(-g) rounds to 2, so g / 2 = 2^-25 is a
tie that goes to 0, while the real value lies just above the tie: one unit in the last place). A reference that converts the double
through fp32 - ``.to(torch.float16)`` does - shows one fp16 difference too, but at g = -2.724609375, and that one is its own double
rounding: high-precision arithmetic gives the fp32 sequence's value there.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import epilogue_value_cases as V
import lora_cases as L
from oracle import oracle as O

DT_IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
_dt = lambda d: DT_IDS[d]


# ------------------------------------------------------------------------------------------ comparison and rounding
def test_comparison_rule():
    nan1 = torch.tensor([0x7FC0, 0x7FC1, 0xFFC0 - 65536], dtype=torch.int16).view(torch.bfloat16)
    nan2 = torch.tensor([0x7FC1, 0x7F81, 0x7FC0], dtype=torch.int16).view(torch.bfloat16)
    assert not bool(V.differ(nan1, nan2).any()), "NaN payloads and signs are left out"
    a = torch.tensor([0.0, -0.0, 1.0, float("nan"), float("inf")], dtype=torch.float16)
    b = torch.tensor([-0.0, -0.0, 1.0, 1.0, float("inf")], dtype=torch.float16)
    assert V.differ(a, b).tolist() == [True, False, False, True, False]          # the sign of zero counts; torch.equal(a, a) is False
    assert V.values_differ(a, b).tolist() == [False, False, False, True, False]
    sub = torch.tensor([2.0 ** -24], dtype=torch.float16)
    assert bool(V.values_differ(sub, torch.zeros(1, dtype=torch.float16)).all()), "a flushed subnormal is a difference"
    f = torch.tensor([0.0, float("nan")])
    assert V.differ(f, torch.tensor([-0.0, float("nan")])).tolist() == [True, False]


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_patterns_and_keys(dtype):
    p = V.all_patterns(dtype)
    assert torch.equal(V.pattern_index(p), torch.arange(65536))
    assert V.finite_count(dtype) == (65536 - 256 if dtype == torch.bfloat16 else 65536 - 2048)
    assert torch.equal(torch.sort(V.pattern_index(V.shuffled_patterns(dtype))).values, torch.arange(65536))
    fin = torch.isfinite(p.float())
    key = V.ordered_key(p[fin])
    order = torch.argsort(p[fin].double(), stable=True)
    assert bool((key[order][1:] - key[order][:-1] >= 0).all()) and int(key.max() - key.min()) == 2 * (V.finite_count(dtype) // 2 - 1)
    back = V.from_key(key, dtype)
    assert not bool(V.values_differ(back, p[fin]).any())


def test_round_once_is_a_single_rounding():
    gen = torch.Generator().manual_seed(1)
    v = torch.randn(200000, generator=gen, dtype=torch.float64) * torch.pow(torch.tensor(2.0, dtype=torch.float64),
                                                                            torch.randint(-26, 15, (200000,), generator=gen).double())
    # a value just above an fp16 tie, by less than fp32 resolves: through fp32 it lands ON the tie and goes to even
    trap = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40, 2.0 ** -25 * (1 + 2.0 ** -30), -(1.0 + 2.0 ** -11 + 2.0 ** -40)], dtype=torch.float64)
    v = torch.cat([v, trap])
    with np.errstate(over="ignore"):
        want = torch.from_numpy(v.numpy().astype(np.float16))        # (numpy converts a double to half in one step)
    got = V.round_once(v, torch.float16)
    assert not bool(V.differ(got, want).any())
    assert got[-3:].tolist() == [1.0 + 2.0 ** -10, 2.0 ** -24, -(1.0 + 2.0 ** -10)] and v[-3:].float().to(torch.float16).tolist()[0] == 1.0
    # bf16: the nearest of the three candidates, checked directly
    b = V.round_once(v, torch.bfloat16)
    key = V.ordered_key(b)
    for step in (-1, 1):
        other = V.from_key(key + step, torch.bfloat16)
        assert bool(((b.double() - v).abs() <= (other.double() - v).abs()).all())
    trap_b = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(V.round_once(trap_b, torch.bfloat16)) == 1.0 + 2.0 ** -7 and float(trap_b.float().to(torch.bfloat16)) == 1.0


# ------------------------------------------------------------------------------------------ the activation
@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_cpu_measurement_behind_the_anchor(dtype):
    p = V.all_patterns(dtype)
    formula = V.silu_fp32_formula(p)
    assert not bool(V.differ(TF.silu(p), formula).any()), "torch's CPU kernel is the fp32 sequence at every pattern"
    once = V.silu_once(dtype)
    fin = torch.isfinite(p.float())
    assert bool(torch.isnan(once[~fin]).all()) and not bool(torch.isnan(once[fin]).any())
    off = V.differ(formula, once) & fin
    where = sorted(p[off].double().tolist(), reverse=True)
    print(f"{_dt(dtype)}: the fp32 sequence differs from float64 rounded once at {len(where)} patterns: {where}")
    if dtype == torch.bfloat16:
        assert where == list(V.BF16_MINUS_ZERO_G) and len(where) == 17
        assert bool((V.pattern_index(formula[off]) == 0x8000).all()), "the exception's value is -0"
        assert bool((V.minus_zero_exception(p) == off).all())
    else:
        assert where == [2.0 ** -24] and float(formula[off]) == 0.0 and float(once[off]) == 2.0 ** -24
        assert not bool(V.minus_zero_exception(p).any())
    bad, diff = V.anchor_violations(p, formula, once)
    assert int(bad.sum()) == 0 and int(diff.sum()) == len(where)
    # the check has teeth: a value two units away, and a +0 in place of the exception's -0, miss it
    two_off = V.from_key((V.ordered_key(formula) + 2).clamp(max=0x7B00), dtype)
    bad2, _ = V.anchor_violations(p, torch.where(fin, two_off, formula), once)
    assert int(bad2.sum()) > 60000
    if dtype == torch.bfloat16:
        bad3, _ = V.anchor_violations(p, torch.where(off, torch.zeros_like(formula), formula), once)
        assert int(bad3.sum()) == 17
    # silu(-inf) = -inf / inf = NaN and silu(+inf) = inf, as torch has them
    inf = torch.tensor([float("-inf"), float("inf")], dtype=dtype)
    assert bool(torch.isnan(TF.silu(inf)[0])) and float(TF.silu(inf)[1]) == float("inf")


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_route_1_makes_every_finite_pattern_a_gate_value(dtype):
    pats = V.shuffled_patterns(dtype)
    sites = [(N // 2, K, 1) for (N, K) in V.STREAM_SITES] + [(V.SM_SITE[0] // 2, V.SM_SITE[1], M) for M in V.SM_MS]
    sites.append((V.EXPERTS_SITE["N"] // 2, V.EXPERTS_SITE["K"], V.EXPERTS_SITE["pairs"]))
    for F_, K, rows in sites:
        stride = min(F_, K)
        seen = torch.zeros(65536, dtype=torch.bool)
        seen_u = torch.zeros(65536, dtype=torch.bool)
        _, gate, up = V.gated_columns(F_, K, "interleaved")
        for j in range(V.route1_launches(F_, K, rows)):
            x = V.route1_rows(pats, j * rows, rows, K, stride)
            assert x.shape == (rows, K) and bool(torch.isfinite(x.float()).all())
            seen[V.pattern_index(x[:, gate[0]]).flatten()] = True
            seen_u[V.pattern_index(x[:, up[0]]).flatten()] = True
        fin = torch.isfinite(V.all_patterns(dtype).float())
        assert bool(seen[fin].all()), (F_, K, rows, int(seen[fin].sum()))
        assert int(seen_u[fin].sum()) > 0.6 * int(fin.sum()), "the up values range over the patterns too"


def test_u_list_and_fp32_sweep():
    for dtype in (*V.DTYPES16, torch.float32):
        u = V.u_list(dtype)
        f = u.double()
        fi = torch.finfo(dtype)
        for v in (fi.tiny, fi.max, 1.0, float("inf")):
            assert bool((f == v).any()) and bool((f == -v).any()), (dtype, v)
        assert int(torch.isnan(f).sum()) == 1 and int((f == 0).sum()) == 2 and int(((f != 0) & (f.abs() < fi.tiny)).sum()) == 2
        assert sorted(V.differ(u[:2], u[:2].flip(0)).tolist()) == [True, True], "+0 and -0 are both there"
    v = V.fp32_sweep_values()
    bits = v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert v.numel() == 131072 and bool((bits[:65536] & 0xFFFF == 0).all()) and torch.unique(bits[:65536] >> 16).numel() == 65536
    assert torch.unique(bits[65536:]).numel() > 65000 and int((bits[65536:] & 0xFFFF != 0).sum()) > 65000


# ------------------------------------------------------------------------------------------ hand-packed weights
def _assert_dequantizes(packed, absmax, W, N, K, bs, qt, dtype):
    want = W.to(dtype)
    assert torch.equal(want.float(), W), "a scale is not a value of T"
    got = O.dequantize_4bit(packed, absmax, bs, qt, (N, K), dtype)
    assert got.shape == (N, K) and not bool(V.differ(got, want).any())


def test_one_hot_packing_byte_order():
    cols = torch.tensor([[1], [2]])
    packed, absmax, W = V.pack_one_hot(2, 64, 64, cols, torch.tensor([[3], [-2]]), "fp4")
    assert packed.shape == (64, 1) and packed.dtype == torch.uint8 and absmax.tolist() == [8.0, 0.25]
    assert int(packed[0]) == 0x03 and int(packed[32 + 1]) == 0x30 and int(packed.sum()) == 0x33     # (code[2 j] << 4) | code[2 j + 1]
    packed, _, _ = V.pack_one_hot(2, 64, 64, cols, torch.tensor([[3], [-2]]), "nf4")
    assert int(packed[0]) == 0x7F and int(packed[33]) == 0xF7 and int(packed[5]) == 0x77
    with pytest.raises(AssertionError, match="share a quantization block"):
        V.pack_one_hot(1, 128, 64, torch.tensor([[0, 5]]), torch.tensor([[0, 0]]))


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_gated_matrices_dequantize_to_the_intended_matrix(dtype):
    qt = V.QUANT_OF[dtype]
    for (N, K) in V.STREAM_SITES:
        cols, gate, up = V.gated_columns(N // 2, K, "interleaved")
        assert torch.unique(gate[0]).numel() == min(N // 2, K) and torch.unique(up[0]).numel() == min(N // 2, K)
        packed, absmax, W = V.pack_one_hot(N, K, 64, cols, torch.zeros_like(cols), qt)
        assert int(W.sum()) == N and bool((W.sum(dim=1) == 1).all())
        _assert_dequantizes(packed, absmax, W, N, K, 64, qt, dtype)
    s = V.EXPERTS_SITE
    for layout in ("chunked", "interleaved"):
        cols, gate, up = V.gated_columns(s["N"] // 2, s["K"], layout, s["E"])
        assert not torch.equal(up[0], up[1]) and not torch.equal(gate[0], gate[1]), "the experts' matrices differ"
        packed, absmax, W = V.pack_one_hot(s["E"] * s["N"], s["K"], s["blocksize"], cols, torch.zeros_like(cols), qt)
        _assert_dequantizes(packed, absmax, W, s["E"] * s["N"], s["K"], s["blocksize"], qt, dtype)
        Wv = W.view(s["E"], s["N"], s["K"])
        I = s["N"] // 2
        g_rows = Wv[:, 0::2] if layout == "interleaved" else Wv[:, :I]
        assert torch.equal(g_rows.argmax(dim=2), gate)


# ------------------------------------------------------------------------------------------ the final rounding
def _neighbours(v: float, dtype):
    """The T values directly below and above a float64 that is not one itself."""
    t = V.round_once(torch.tensor([v], dtype=torch.float64), dtype)
    key = V.ordered_key(t)
    around = [float(V.from_key(key + d, dtype).double()) for d in (-1, 0, 1)]
    lo = max(a for a in around if a <= v)
    hi = min(a for a in around if a >= v)
    return lo, hi


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_rounding_cases_are_exact_and_land_where_they_should(dtype):
    grid = V.rounding_grid(dtype)
    cases = {c.name: c for c in V.rounding_cases(dtype)}
    assert len(cases) == len(V.rounding_cases(dtype)) == len(grid.named)
    N, K, bs = V.ROUNDING_SHAPE
    assert grid.pq.shape[0] <= N and grid.ab.shape[0] <= 32
    fi = torch.finfo(dtype)
    scales = 2.0 ** grid.pq.double()
    assert bool((scales >= fi.tiny).all()) and bool((scales <= fi.max).all()), "every block scale is a NORMAL value of T"
    mx = float(fi.max)
    min_sub = 2.0 ** (-133 if dtype == torch.bfloat16 else -24)
    seen = set()
    for name, cs in cases.items():
        i, j = grid.named[name]
        assert bool(grid.exact[i, j]), name
        assert float(grid.total[i, j]) == cs.total
        terms = (cs.a * 2.0 ** cs.p, cs.b * 2.0 ** cs.q, cs.c)
        for sub in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):                # every partial sum is an fp32 value, in float64
            v = sum(terms[k] for k in sub)
            assert float(torch.tensor(v, dtype=torch.float64).float().double()) == v, (name, sub)
        if cs.c == 0:
            assert bool(grid.exact_nobias[i, j]) and not bool(V.differ(grid.want[i, j], grid.want_nobias[i, j])), name
        else:
            assert not bool(grid.exact_nobias[i, j])
        want = float(grid.want[i, j].double())
        tot = abs(cs.total)
        base = name.replace("-neg", "").replace("-bias", "")
        assert (want < 0 or (want == 0 and V.pattern_index(grid.want[i, j]) == 0x8000)) == name.endswith("-neg"), name
        want = abs(want)
        if base.startswith("tie-") and not base.endswith("ulp32"):
            lo, hi = _neighbours(tot, dtype)
            assert tot - lo == hi - tot and lo < tot < hi, name
            lo_even = int(V.pattern_index(torch.tensor([lo], dtype=torch.float64).to(dtype))) % 2 == 0
            assert lo_even == (base == "tie-even") and want == (lo if lo_even else hi), name
            seen.add("tie-even-lower" if lo_even else "tie-odd-lower")
        elif base.startswith("tie-"):
            lo, hi = _neighbours(tot, dtype)
            mid = (lo + hi) / 2
            ulp32 = 2.0 ** -13
            assert abs(tot - mid) == ulp32 and want == (hi if tot > mid else lo), name
            seen.add("tie+ulp32" if tot > mid else "tie-ulp32")
        elif base.startswith("max"):
            threshold = mx + (mx - float(V.from_key(V.ordered_key(torch.tensor([mx], dtype=torch.float64).to(dtype)) - 1, dtype).double())) / 2
            assert (dtype != torch.float16) or threshold == 65520.0
            assert want == (float("inf") if tot >= threshold else mx), name
            seen.add("overflow" if tot >= threshold else "below-overflow")
        else:
            assert tot < float(fi.tiny) and (dtype == torch.float16 or tot < 2.0 ** -126), name
            if base in ("zero-tie", "zero-tie-"):
                assert want == 0.0 and tot <= min_sub / 2, name
                seen.add("tie-to-zero" if tot == min_sub / 2 else "below-zero-tie")
            elif base == "sub-exact":
                assert want == tot
                seen.add("subnormal-exact")
            elif base == "normal-boundary-tie":
                assert want == float(fi.tiny) and float(fi.tiny) - tot == min_sub / 2, name
                seen.add("subnormal-normal-boundary")
            else:
                assert want > 0 and want % min_sub == 0 and abs(want - tot) <= min_sub / 2, name
                seen.add("subnormal-tie" if abs(want - tot) == min_sub / 2 else "above-zero-tie")
    assert seen == {"tie-even-lower", "tie-odd-lower", "tie+ulp32", "tie-ulp32", "overflow", "below-overflow", "tie-to-zero", "below-zero-tie",
                    "subnormal-exact", "subnormal-normal-boundary", "subnormal-tie", "above-zero-tie"}, seen
    assert sum(n.endswith("-neg") for n in cases) * 2 == len(cases) and sum("-bias" in n for n in cases) >= 8
    # the grid's reference is one rounding of an exact sum: the single-rounding conversion agrees wherever the cell qualifies
    once = V.round_once(grid.total.clamp(-mx, mx), dtype)
    inside = grid.exact & (grid.total.abs() <= mx)
    assert not bool((V.differ(once, grid.want) & inside).any())
    print(f"{_dt(dtype)}: {len(cases)} named cases, {int(grid.exact.sum())} exact cells with bias, {int(grid.exact_nobias.sum())} without")


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_rounding_weights_through_the_oracle(dtype):
    grid = V.rounding_grid(dtype)
    N, K, bs = V.ROUNDING_SHAPE
    for qt in ("fp4", "nf4"):
        packed, absmax, W, row_of = V.rounding_weights(grid, N, K, bs, qt)
        _assert_dequantizes(packed, absmax, W, N, K, bs, qt, dtype)
        assert bool((W[:, 0] == 2.0 ** grid.pq[row_of, 0].double()).all()) and bool((W[:, K - bs] == 2.0 ** grid.pq[row_of, 1].double()).all())
        assert int((W != 0).sum()) == 2 * N
    chunks = V.rounding_activations(grid, K, bs, 16)
    idx = torch.cat([i for _, i in chunks])
    assert torch.equal(idx[idx >= 0], torch.arange(grid.ab.shape[0])) and all(x.shape == (16, K) for x, _ in chunks)
    # the oracle's fused matmul on a chunk gives the grid's reference where the cell qualifies (its fp32 sums are exact there)
    x, rows = chunks[0]
    y = O.gemm_4bit(x, packed, (N, K), absmax, bs, "nf4", grid.c[row_of])[0]
    ok = grid.exact[rows][:, row_of]
    assert not bool((V.differ(y, grid.want[rows][:, row_of]) & ok).any())


# ------------------------------------------------------------------------------------------ LoRA, row scale
@functools.lru_cache(maxsize=None)
def _lora_terms(dtype, r):
    N, K, bs = V.LORA_SHAPE
    case = L.LoRACase(N, K, bs, dtype, False)
    ex = L.build_case(case)
    t, b = L.build_adapter(case, r)
    acc, lv = V.lora_terms(ex, t, b)
    return acc + ex.bias.double(), lv


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_lora_case_has_teeth(dtype):
    """A single-rounding fused multiply-add in place of ``rounded(vb) + rounded(s * lv)`` gives another T value somewhere: the case
    can see the fold it is there for. (The scalings of tests/lora_cases.py, 0.5 and 2, cannot: their product does not round.)"""
    assert (V.LORA_SHAPE[:2] + (V.LORA_SHAPE[2],)) in L.STREAM_SHAPES and V.LORA_SHAPE in L.SM_SHAPES and V.LORA_SHAPE in L.NESTED_SHAPES
    counts = {}
    for r in V.LORA_RANKS:
        vb, lv = _lora_terms(dtype, r)
        assert float(lv.abs().max()) > 0 and float((lv.abs() * 1.7 + vb.abs()).max()) < 60000
        for s in V.LORA_SCALINGS:
            ref = V.lora_reference(vb, lv, s, dtype)
            fused = V.lora_fused_emulation(vb, lv, s, dtype)
            counts[r, round(s, 4)] = int(V.differ(ref, fused).sum())
            pr_rounds = int(((torch.tensor(s, dtype=torch.float32) * lv.float()).double() != float(torch.tensor(s, dtype=torch.float32)) * lv).sum())
            assert pr_rounds > 0.5 * int((lv != 0).sum()), "the product s * lv rounds at most elements"
        for s in L.SCALINGS:
            assert not bool(V.differ(V.lora_reference(vb, lv, s, dtype), V.lora_fused_emulation(vb, lv, s, dtype)).any())
    print(f"{_dt(dtype)}: elements of {tuple(vb.shape)} at which a fused multiply-add gives another value, by (rank, scaling): {counts}")
    assert max(counts.values()) > 0, counts


def test_scale_samples_cover_the_edges():
    for dtype in (*V.DTYPES16, torch.float32):
        n = V.EXPERTS_SITE["E"] * V.EXPERTS_SITE["N"]
        v = V.scale_samples(dtype, n)
        f = v.double()
        fi = torch.finfo(dtype)
        assert v.numel() == n and v.dtype == dtype and bool(torch.isfinite(f).all())
        sub = (f != 0) & (f.abs() < fi.tiny)
        assert int(sub.sum()) >= 254 and bool((f == fi.max).any()) and bool((f == -fi.max).any()) and bool((f == fi.tiny).any())
        if dtype != torch.float32:
            assert torch.unique(V.pattern_index(v[sub])).numel() == 2 * (2 ** V.MANT_BITS[dtype] - 1), "every subnormal of a 16-bit type"
        for wdt in {torch.float32, dtype}:
            w = V.scale_weights(wdt, 64, 0)
            wf = w.double()
            assert w.dtype == wdt and int(torch.isnan(wf[:9]).sum()) == 1 and int(torch.isinf(wf[:9]).sum()) == 2 and int((wf[:9] == 0).sum()) == 2
            assert int(((wf[:9] != 0) & (wf[:9].abs() < torch.finfo(wdt).tiny)).sum()) == 2
            assert not torch.equal(V.scale_weights(wdt, 64, 1)[9:].float().nan_to_num(), w[9:].float().nan_to_num())
            ref = V.scale_reference(v.view(V.EXPERTS_SITE["E"], -1), w)
            assert ref.shape == (64, V.EXPERTS_SITE["N"]) and ref.dtype == dtype
            assert bool(torch.isnan(ref[6]).all()) and bool(torch.isnan(ref[4][f.view(2, -1)[0] == 0]).all())        # NaN scale; inf * 0
