"""GPU: the fused epilogues over VALUES (tests/epilogue_value_cases.py; preconditions on the CPU: tests/test_epilogue_values_host.py).

A. the gated activation ``T(T(silu(g)) * u)`` at its three single-GPU sites - the streaming kernel's kGated epilogue (M = 1, the
   exact-geometry instance and a general one), the streaming MFMA kernel's GATED instances (2, 4, 8, 16 rows) and the experts kernel's
   kEpiGated (chunked and interleaved; bf16, fp16 and fp32) - with every finite 16-bit pattern as ``g`` through the accumulator
   (route 1) and all 65536 patterns, +-inf, every NaN and -0 included, through the bias against a list of edge values of ``u`` (route
   2). Asserted: the gated output equals torch's ``F.silu(g) * u`` on the plain call's output; the plain output holds the intended
   patterns as values (a flushed subnormal would show here); for finite ``g`` and ``u = 1`` the result is within one unit in the last
   place of float64 ``g / (1 + exp(-g))`` rounded once, except bf16 g in [-97, -89], which give exactly -0.
B. the final rounding ``T(acc + bias)`` of every kernel family on ties, around the overflow threshold and among the subnormals of T:
   the float64 sum rounded once, bit for bit.
C. the two fp32 epilogues that multiply: the LoRA sum at scalings that are not powers of two, and the experts kernel's row scale,
   against the documented sequence in CPU float32, bit for bit.
Every sweep asserts the kernel family that ran and its own coverage. Comparison: equal NaN masks, equal bits elsewhere.
"""
import ctypes as ct
import functools
import time

import pytest
import torch
import torch.nn.functional as TF

import epilogue_value_cases as V
import lora_cases as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT_IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
_dt = lambda d: DT_IDS[d]


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _hip():
    from bitsandbytes_amd.backends import hip

    return hip


def _experts_op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_experts.default


def _grad_input_op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_grad_input.default


def _family():
    return _bnb().lib.bnb_mi355x_last_gemm_kernel()


def _on_device(packed, absmax, W, N, K, bs, qt, dtype):
    """The hand-packed matrix on the device, checked once through the library's dequantizer: the intended matrix, bit for bit."""
    _bnb()                                                       # (the import registers the operators)
    packed, absmax = packed.to(DEV), absmax.to(DEV)
    back = torch.ops.bitsandbytes.dequantize_4bit.default(packed, absmax, bs, qt, [N, K], dtype)
    assert not bool(V.differ(back, W.to(dtype).to(DEV)).any()), "the hand-packed matrix does not dequantize to the intended one"
    return packed, absmax


# ------------------------------------------------------------------------------------------ A: the sites
class GatedSite:
    """One place where the activation is computed: ``plain(x, bias) -> (g, u)`` and ``gated(x, bias) -> h`` on the same operands,
    the intended ``(g, u)`` of route 1 and the layout of a bias; each call asserts the family that ran."""

    def __init__(self, name, dtype, F_, K, rows, E=1, layout="interleaved", bs=64):
        self.name, self.dtype, self.F, self.K, self.rows, self.E, self.layout, self.bs = name, dtype, F_, K, rows, E, layout, bs
        self.qt = V.QUANT_OF[dtype]
        cols, gate, up = V.gated_columns(F_, K, layout, E)
        packed, absmax, W = V.pack_one_hot(E * 2 * F_, K, bs, cols, torch.zeros_like(cols), self.qt)
        self.packed, self.absmax = _on_device(packed, absmax, W, E * 2 * F_, K, bs, self.qt, dtype)
        self.gate, self.up = gate.to(DEV), up.to(DEV)
        self.expert = (torch.arange(rows) % E).to(DEV)           # pairs spread over the experts (one "expert" elsewhere)

    def intended(self, x):
        return x.gather(1, self.gate[self.expert]), x.gather(1, self.up[self.expert])

    def bias(self, bg, bu):
        """[E, F] gate and up biases -> the op's bias argument."""
        b = V.bias_in_layout(bg, bu, self.layout)
        return b if self.E > 1 else b.reshape(-1)


class DenseSite(GatedSite):
    def __init__(self, name, dtype, N, K, M, family):
        super().__init__(name, dtype, N // 2, K, M)
        self.N, self.family = N, family
        lib = _bnb().lib
        assert lib.bnb_mi355x_gemm_4bit_gated_supported(V.DT_CODE[dtype], M, N, K, self.bs) == 1, (name, M)

    def plain(self, x, bias):
        y = torch.ops.bitsandbytes.gemm_4bit.default(x, self.packed, [self.N, self.K], self.absmax, self.bs, self.qt, bias)
        assert _family() == self.family, (self.name, _family())
        return y[:, 0::2], y[:, 1::2]

    def gated(self, x, bias):
        h = torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(x, self.packed, [self.N, self.K], self.absmax, self.bs, self.qt, bias)
        assert _family() == self.family, (self.name, _family())
        return h


class ExpertsSite(GatedSite):
    def __init__(self, dtype, layout, rows):
        s = V.EXPERTS_SITE
        super().__init__(f"experts-{layout}", dtype, s["N"] // 2, s["K"], rows, E=s["E"], layout=layout, bs=s["blocksize"])
        self.N, self.family = s["N"], V.K_EXPERTS
        self.ids = self.expert.view(rows, 1)
        assert _hip().gemm_4bit_experts_ffn_supported(dtype, self.E, self.N, self.K, self.bs, layout)
        assert _hip().gemm_4bit_experts_supported(dtype, self.E, self.N, self.K, self.bs)

    def plain(self, x, bias):
        y = _experts_op()(x, self.packed, [self.E, self.N, self.K], self.absmax, self.ids, self.bs, self.qt, bias)
        assert _family() == self.family
        y = y.view(self.rows, self.N)
        return (y[:, 0::2], y[:, 1::2]) if self.layout == "interleaved" else (y[:, :self.F], y[:, self.F:])

    def gated(self, x, bias):
        h = torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default(x, self.packed, [self.E, self.N, self.K], self.absmax, self.ids, self.bs, self.qt,
                                                                     bias, None, None, None, None, self.layout)
        assert _family() == self.family
        return h.view(self.rows, self.F)


def _first(mask, *tensors):
    """The first element of a mismatch mask with the values of the given tensors there."""
    pos = torch.nonzero(mask)[0].tolist()
    return tuple(pos), [t[tuple(pos)].item() if t.dtype != torch.bfloat16 else float(t[tuple(pos)]) for t in tensors]


def _note(fails, mask, what, *tensors):
    """Record a finding - how many elements, and the first with its values - and go on: one run shows every kind of difference."""
    if bool(mask.any()):
        fails.append(f"{what}: {int(mask.sum())} elements, first {_first(mask, *tensors)}")


def _sweep_route_1(site, pats_cpu):
    """Every finite pattern as a gate value through the accumulator. Returns the number of patterns seen as g."""
    n = pats_cpu.numel()
    finite = torch.isfinite(pats_cpu.float()).to(DEV)
    seen = torch.zeros(n, dtype=torch.bool, device=DEV)
    stride = min(site.F, site.K)
    fails = []
    for j in range(V.route1_launches(site.F, site.K, site.rows, n)):
        x, idx = V.route1_rows(pats_cpu, j * site.rows, site.rows, site.K, stride, with_index=True)
        x, idx = x.to(DEV), idx.to(DEV)
        gi, ui = site.intended(x)
        g, u = site.plain(x, None)
        h = site.gated(x, None)
        want = TF.silu(g) * u
        _note(fails, V.differ(h, want), f"{site.name} route 1 launch {j}: gated != silu(g) * u of the plain output (g, u, got, want)", g, u, h, want)
        for nm, got, meant in (("g", g, gi), ("u", u, ui)):
            _note(fails, V.values_differ(got, meant), f"{site.name} route 1 launch {j}, family {site.family}: the plain output's {nm} is not the "
                  "activation it copies (got, intended)", got, meant)
        seen[idx.gather(1, site.gate[site.expert]).flatten()] = True
    assert bool(seen[finite].all()), f"{site.name}: {int(seen[finite].sum())} of {int(finite.sum())} finite patterns were a gate value"
    assert not fails, f"{len(fails)} findings; first: {fails[:6]}"
    return int(seen[finite].sum())


def _sweep_route_2(site, pats_cpu, anchor):
    """All patterns (+-inf, NaN, -0 too) as the gate's bias against every listed ``u``, x = 0. Returns (patterns seen as g, sorted gate
    values at which T(silu(g)) differs from float64 rounded once - 16-bit types only)."""
    n = pats_cpu.numel()
    pats = pats_cpu.to(DEV)
    ul = V.u_list(site.dtype).to(DEV)
    Lu = ul.numel()
    table = V.silu_once(site.dtype).to(DEV) if anchor else None
    x = torch.zeros(site.rows, site.K, dtype=site.dtype, device=DEV)
    met = torch.zeros(n, Lu, dtype=torch.bool, device=DEV)
    off_anchor = torch.zeros(65536, dtype=torch.bool, device=DEV)
    per = site.E * site.F
    fails = []
    for rot in range(Lu):
        for j in range(-(-n // per)):
            idx = (j * per + torch.arange(per, device=DEV)) % n
            ui = (idx + rot) % Lu
            bg, bu = pats[idx].view(site.E, site.F), ul[ui].view(site.E, site.F)
            bias = site.bias(bg, bu)
            g, u = site.plain(x, bias)
            h = site.gated(x, bias)
            want = TF.silu(g) * u
            _note(fails, V.differ(h, want), f"{site.name} route 2 (rotation {rot}, launch {j}): gated != silu(g) * u of the plain output (g, u, got, want)",
                  g, u, h, want)
            gi, uu = bg[site.expert], bu[site.expert]
            for nm, got, meant in (("g", g, gi), ("u", u, uu)):
                _note(fails, V.values_differ(got, meant), f"{site.name} route 2, family {site.family}: T(0 + bias) is not the bias ({nm}: got, bias)", got, meant)
            met[idx, ui] = True
            if anchor:
                one = uu == 1.0
                miss, diff = V.anchor_violations(g, h, table)
                _note(fails, miss & one, f"{site.name}: the anchor is missed (g, got)", g, h)
                off_anchor[V.pattern_index(g)[diff & one]] = True
                neg_inf = torch.isinf(g) & (g < 0) & one
                _note(fails, neg_inf & ~torch.isnan(h), f"{site.name}: silu(-inf) * 1 is NaN, as in torch (g, got)", g, h)
    assert bool(met.all()), f"{site.name}: {int(met.sum())} of {n * Lu} (g, u) pairs were met"
    assert not fails, f"{len(fails)} findings; first: {fails[:6]}"
    where = sorted(V.all_patterns(site.dtype)[off_anchor.cpu()].double().tolist(), reverse=True) if anchor else []
    return int(met.any(dim=1).sum()), where


def _report(site, t0, seen1, seen2, where):
    line = (f"[epilogue-values] {site.name} {_dt(site.dtype)} rows={site.rows} family={site.family}: route 1 {seen1} finite patterns as g, "
            f"route 2 {seen2} patterns x {V.u_list(site.dtype).numel()} u")
    if site.dtype != torch.float32:
        line += f"; differs from float64 rounded once at {len(where)} gate values {where}"
    print(line + f"; {time.time() - t0:.1f} s")


def _run_site(site):
    t0 = time.time()
    f32 = site.dtype == torch.float32
    pats1 = V.fp32_sweep_values() if f32 else V.shuffled_patterns(site.dtype)
    pats2 = V.fp32_sweep_values() if f32 else V.all_patterns(site.dtype)
    seen1 = _sweep_route_1(site, pats1)
    seen2, where = _sweep_route_2(site, pats2, anchor=not f32)
    assert seen2 == pats2.numel() and seen1 == int(torch.isfinite(pats1.float()).sum())
    if not f32:
        assert seen2 == 65536 and seen1 == V.finite_count(site.dtype)
        # the derived exception is the only place where more than the last place may differ, and there the value is pinned
        if site.dtype == torch.bfloat16:
            assert set(V.BF16_MINUS_ZERO_G) <= set(where), "the fp32 sequence gives -0 on [-97, -89]: expf(-g) overflows"
    _report(site, t0, seen1, seen2, where)


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
@pytest.mark.parametrize("shape", V.STREAM_SITES, ids=lambda s: "x".join(map(str, s)))
def test_gated_values_streaming_kernel(shape, dtype):
    N, K = shape
    _run_site(DenseSite(f"stream-{N}x{K}", dtype, N, K, 1, V.K_STREAM))


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
@pytest.mark.parametrize("M", V.SM_MS)
def test_gated_values_streaming_mfma_kernel(M, dtype):
    N, K = V.SM_SITE
    _run_site(DenseSite(f"sm-{N}x{K}", dtype, N, K, M, V.K_SM))


@pytest.mark.parametrize("dtype", (*V.DTYPES16, torch.float32), ids=_dt)
@pytest.mark.parametrize("layout", ["chunked", "interleaved"])
def test_gated_values_experts_kernel(layout, dtype):
    """fp32: the 65536 values whose low 16 bits are zero and 65536 random bit patterns, against torch's fp32 ``F.silu(g) * u`` on the
    GPU only."""
    _run_site(ExpertsSite(dtype, layout, V.EXPERTS_SITE["pairs"]))


# ------------------------------------------------------------------------------------------ B: the final rounding
REQUIRED_FAMILIES = ("stream", "sm", "rt", "pc", "kq", "experts", "grouped-stream", "grouped-sm", "grad-input")


@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_final_rounding_in_every_family(dtype):
    from test_gpu_parity import _forced

    bnb, hip = _bnb(), _hip()
    lib = bnb.lib
    t0 = time.time()
    grid = V.rounding_grid(dtype)
    N, K, bs = V.ROUNDING_SHAPE
    qt = V.QUANT_OF[dtype]
    packed, absmax, W, row_of = V.rounding_weights(grid, N, K, bs, qt)
    packed, absmax = _on_device(packed, absmax, W, N, K, bs, qt, dtype)
    row_of = row_of.to(DEV)
    c = grid.c.to(DEV)[row_of]
    want = {True: grid.want.to(DEV), False: grid.want_nobias.to(DEV)}
    exact = {True: grid.exact.to(DEV), False: grid.exact_nobias.to(DEV)}
    named_cells = {True: set(grid.named.values()), False: {v for k, v in grid.named.items() if bool(grid.exact_nobias[v])}}
    dt = V.DT_CODE[dtype]

    def fused(kernel):
        return lambda x, bias: hip._gemm_4bit_fused(x, packed, (N, K), absmax, bs, qt, bias, None, None, None, kernel=kernel)

    def forced(knob, family):
        def call(x, bias):
            with _forced(knob, family):
                return hip._gemm_4bit_fused(x, packed, (N, K), absmax, bs, qt, bias, None, None, None, kernel=2)
        return call

    def experts(x, bias):
        E = 2
        ids = (torch.arange(x.shape[0], device=DEV) % E).view(-1, 1)
        assert hip.gemm_4bit_experts_supported(dtype, E, N, K, bs)
        y = _experts_op()(x, torch.cat([packed, packed]), [E, N, K], torch.cat([absmax, absmax]), ids, bs, qt,
                          None if bias is None else torch.stack([bias, bias]))
        return y.view(x.shape[0], N)

    def grouped(route):
        def call(x, bias):
            ns = (ct.c_int * 2)(N, N)
            assert lib.bnb_mi355x_gemm_4bit_grouped_route(dt, 2, ns, x.shape[0], K, bs) == route, (route, x.shape[0])
            # bias per member: the first member carries it, the second runs bare (and is checked as the call without bias)
            ys = hip.gemm_4bit_grouped(x, [(packed, (N, K), absmax, bias, None, None, None), (packed, (N, K), absmax, None, None, None, None)], bs, qt)
            call.second = ys[1]
            return ys[0]
        return call

    # (name, rows per launch, call, family asserted after the launch; _forced asserts its own)
    families = [("stream", 1, fused(1), V.K_STREAM), ("sm", 16, forced(5000, V.K_SM), V.K_SM), ("rt", 16, forced(2000, V.K_RT), V.K_RT),
                ("pc", 16, forced(1101, V.K_PC), V.K_PC), ("kq", 16, forced(4000, V.K_KQ), V.K_KQ), ("experts", 16, experts, V.K_EXPERTS),
                ("grouped-stream", 1, grouped(1), V.K_STREAM), ("grouped-sm", 16, grouped(2), V.K_SM)]
    ran, failures = {}, []      # ran: family name -> (kernel family the library reports after the launches, exact cells compared)
    A, R = grid.exact.shape
    for name, rows, call, family in families:
        cells, launched = 0, set()
        compared = {wb: torch.zeros(A, R, dtype=torch.bool, device=DEV) for wb in (False, True)}
        for x, idx in V.rounding_activations(grid, K, bs, rows):
            x, idx = x.to(DEV), idx.to(DEV)
            valid = (idx >= 0)[:, None]
            a_of = idx.clamp(min=0)
            for with_bias in (False, True):
                y = call(x, c if with_bias else None)
                launched.add(_family())
                results = [(with_bias, y)]
                if name.startswith("grouped") and with_bias:
                    results.append((False, call.second))
                for wb, out in results:
                    ok = exact[wb][a_of][:, row_of] & valid
                    bad = V.differ(out, want[wb][a_of][:, row_of]) & ok
                    cells += int(ok.sum())
                    compared[wb][a_of[:, None].expand_as(ok)[ok], row_of[None, :].expand_as(ok)[ok]] = True
                    if bool(bad.any()):
                        m, n = torch.nonzero(bad)[0].tolist()
                        a, r = int(a_of[m]), int(row_of[n])
                        label = [k for k, v in grid.named.items() if v == (a, r)] or ["unnamed cell"]
                        failures.append(f"{name} bias={int(wb)}: {int(bad.sum())} cells; first {label[0]}: {float(grid.total[a, r])!r} (c = {float(grid.c[r])!r}) "
                                        f"gave {float(out[m, n])!r}, want {float(want[wb][a, r])!r}")
        for wb in (False, True):
            missing = [cell for cell in named_cells[wb] if not bool(compared[wb][cell])]
            assert not missing, f"{name} bias={int(wb)}: named cases that were not compared: {missing}"
        if launched == {family}:   # (a family that fell back to another kernel is not reached)
            ran[name] = (family, cells)
        else:
            failures.append(f"{name}: kernel families {sorted(launched)} ran, the case is about {family}")
    # gemm_4bit_grad_input: no bias, the two terms in weight rows 0 and N - 1 of one column
    pk, am, Wt, rows_t = V.rounding_weights_transposed(grid, N, bs, qt)
    Kt = Wt.shape[1]
    pk, am = _on_device(pk, am, Wt, N, Kt, bs, qt, dtype)
    gout = torch.zeros(A, N, dtype=dtype)
    gout[:, 0], gout[:, N - 1] = grid.ab[:, 0], grid.ab[:, 1]
    fused_backward = hip.grad_input_fused_ok(dtype, A, N, Kt, bs)
    gin = _grad_input_op()(gout.to(DEV), pk, [N, Kt], am, bs, qt)
    got = gin[:, torch.arange(rows_t.numel(), device=DEV) * bs]
    ok = exact[False][:, rows_t.to(DEV)]
    bad = V.differ(got, want[False][:, rows_t.to(DEV)]) & ok
    if bool(bad.any()):
        m, n = torch.nonzero(bad)[0].tolist()
        failures.append(f"grad-input: {int(bad.sum())} cells; first: {float(grid.total[m, rows_t[n]])!r} gave {float(got[m, n])!r}, want {float(want[False][m, rows_t[n]])!r}")
    for cell in named_cells[False]:
        assert bool(ok[cell[0], rows_t.tolist().index(cell[1])]), f"grad-input: named case {cell} was not compared"
    if fused_backward:   # (the operator composes dequantize + matmul where the fused kernel does not serve: not the kernel under test)
        ran["grad-input"] = ("fused", int(ok.sum()))
    print(f"[epilogue-values] final rounding {_dt(dtype)}: families reached (kernel family, exact cells compared): {ran}; {len(grid.named)} named "
          f"cases each; {time.time() - t0:.1f} s")
    assert not failures, failures
    assert not [f for f in REQUIRED_FAMILIES if f not in ran], ran


# ------------------------------------------------------------------------------------------ C: LoRA, row scale
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("dtype", V.DTYPES16, ids=_dt)
def test_lora_sum_at_scalings_that_round(dtype, nested):
    from test_gpu_lora import _prepared

    lib = _bnb().lib
    t0 = time.time()
    N, K, bs = V.LORA_SHAPE
    case = L.LoRACase(N, K, bs, dtype, nested)
    d = _prepared(case)
    acc = d["y64"].cpu()
    op = torch.ops.bitsandbytes_amd.gemm_4bit_lora.default
    failures, calls = [], 0
    # elements at which ONE fused multiply-add in place of the product and the sum would give another value, per kernel: the streaming
    # kernel runs every one of the 17 activation rows as its own M = 1 launch, the streaming MFMA kernel rows 0 ... M - 1
    fold_visible = {V.K_STREAM: 0, V.K_SM: 0}
    rows_all = d["x"].shape[0]
    for r in V.LORA_RANKS:
        t_cpu, b_cpu = L.build_adapter(case, r)
        t, b = t_cpu.to(DEV), b_cpu.to(DEV)
        lv = t_cpu.double() @ b_cpu.double().t()
        for s in V.LORA_SCALINGS:
            for with_bias in (False, True):
                vb = acc + d["ex"].bias.double() if with_bias else acc
                ref = V.lora_reference(vb, lv, s, dtype)
                visible = V.differ(ref, V.lora_fused_emulation(vb, lv, s, dtype))
                fold_visible[V.K_STREAM] += int(visible.sum())
                fold_visible[V.K_SM] += int(visible[:max(V.LORA_MS)].sum())
                launches = [(m0, 1) for m0 in range(rows_all)] + [(0, M) for M in V.LORA_MS if M > 1]
                for m0, M in launches:
                    assert lib.bnb_mi355x_gemm_4bit_lora_supported(V.DT_CODE[dtype], M, N, K, bs, int(nested), r) == 1
                    y = op(d["x"][m0:m0 + M], d["packed"], [N, K], d["absmax"], bs, "fp4", t[m0:m0 + M].contiguous(), b, s,
                           d["bias"] if with_bias else None, **d["stats"])
                    assert _family() == (V.K_STREAM if M == 1 else V.K_SM), (M, _family())
                    calls += 1
                    bad = V.differ(y.cpu(), ref[m0:m0 + M])
                    if bool(bad.any()):
                        m, n = torch.nonzero(bad)[0].tolist()
                        m += m0
                        failures.append(f"r={r} s={s!r} bias={int(with_bias)} rows {m0}..{m0 + M - 1}: {int(bad.sum())} elements; first [{m}, {n}]: vb {float(vb[m, n])!r} "
                                        f"lora {float(lv[m, n])!r} gave {float(y[m - m0, n])!r}, want {float(ref[m, n])!r}")
    print(f"[epilogue-values] lora {case.name}: {calls} calls, {len(failures)} not bit-equal; a fused multiply-add would show at "
          f"{fold_visible[V.K_STREAM]} elements of the streaming kernel's launches and {fold_visible[V.K_SM]} of the streaming MFMA kernel's; "
          f"{time.time() - t0:.1f} s")
    assert fold_visible[V.K_STREAM] > 0 and fold_visible[V.K_SM] > 0, "the case cannot see the fold it is there for"
    assert not failures, failures[:5]


@pytest.mark.parametrize("dtype", (*V.DTYPES16, torch.float32), ids=_dt)
def test_row_scale_values(dtype):
    """``T((acc + b) * w)`` with ``acc = 0``: the bias holds a sample of T (every 16-bit subnormal, the largest finite value), the
    scales are random fp32 bit patterns, +-0, +-subnormal, +-inf and NaN, in fp32 and in T."""
    t0 = time.time()
    s = V.EXPERTS_SITE
    E, N, K, bs, P = s["E"], s["N"], s["K"], s["blocksize"], s["pairs"]
    site = ExpertsSite(dtype, "chunked", P)
    vb_cpu = V.scale_samples(dtype, E * N).view(E, N)
    vb = vb_cpu.to(DEV)
    x = torch.zeros(P, K, dtype=dtype, device=DEV)
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default
    assert _hip().gemm_4bit_experts_ffn_supported(dtype, E, N, K, bs, "none")
    failures, calls = [], 0
    for wdt in dict.fromkeys((torch.float32, dtype)):
        for seed in range(4):
            w = V.scale_weights(wdt, P, seed)
            y = op(x, site.packed, [E, N, K], site.absmax, site.ids, bs, site.qt, vb, None, None, None, w.to(DEV).view(P, 1), "none")
            assert _family() == V.K_EXPERTS
            calls += 1
            ref = V.scale_reference(vb_cpu, w)
            bad = V.differ(y.view(P, N).cpu(), ref)
            if bool(bad.any()):
                p, n = torch.nonzero(bad)[0].tolist()
                failures.append(f"w in {_dt(wdt)} seed {seed}: {int(bad.sum())} elements; first: b {float(vb_cpu[p % E, n])!r} w {float(w[p])!r} "
                                f"gave {float(y.view(P, N)[p, n])!r}, want {float(ref[p, n])!r}")
    print(f"[epilogue-values] row scale {_dt(dtype)}: {calls} calls of {P} x {N} products, {len(failures)} not bit-equal; {time.time() - t0:.1f} s")
    assert not failures, failures[:5]
