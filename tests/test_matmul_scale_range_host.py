"""CPU preconditions of tests/test_gpu_matmul_scale_range.py (builders: tests/matmul_scale_range_cases.py): what the GPU tests take
for granted about their inputs and wants is asserted here, without a GPU."""
import pytest
import torch

import decode_probe_cases as P
import exact_inputs as X
import matmul_scale_range_cases as C
import scale_range_cases as R

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
_id = lambda cs: f"{cs.family}-{cs.name}"


def _grid(quant):
    """(code [16, 1, 1], every scale [1, 1532, 1], V_CYCLE [1, 1, 8]): the 196 096 cells of the issue's census."""
    return (P.code_table(quant)[:, None, None], R.scales()[None, :, None], torch.tensor(P.V_CYCLE, dtype=torch.float32)[None, None, :])


def _differ(a, b) -> int:
    return int(R._mismatches(a, b).sum())


# ------------------------------------------------------------------------------------------ the restated orders
@pytest.mark.parametrize("quant", ["nf4", "fp4"])
@pytest.mark.parametrize("dtype", [BF, HF, F32], ids=["bf16", "fp16", "fp32"])
def test_restated_orders_equal_one_rounding_where_that_is_the_truth(quant, dtype):
    """Power-of-two scale, normal result (and normal intermediate values): every step but the last is exact, so each order is the
    float64 product of ITS operand - T(code) for order A, the fp32 code otherwise - rounded once."""
    c, s, v = _grid(quant)
    pow2 = (torch.frexp(s)[0] == 0.5) & torch.isfinite(s)
    fi = torch.finfo(dtype)
    checked = 0
    for order in C.ORDERS:
        if order == "B32" and dtype != F32:
            continue
        operand = c.to(dtype).float() if order == "A" else c
        exact = operand.double() * s.double() * v.double()
        once = exact.float().to(dtype)
        # normal everywhere a rounding could happen: the result in T, and code * scale / code * v * scale in fp32
        normal = pow2 & (exact.abs() >= max(fi.tiny, 2.0 ** -126) * 4) & (exact.abs() <= fi.max / 4) & ((operand.double() * s.double()).abs() >= 2.0 ** -120)
        if order != "A" and dtype != F32:
            # an unrounded code under a power-of-two scale: T(fl32(c s) v) and T(fl32(c v) s) round c s v once - fp32 holds it exactly
            assert torch.equal(exact.float().double()[normal.expand_as(exact)], exact[normal.expand_as(exact)])
        got = C.restate(order, c, s, v, dtype)
        m = normal.expand_as(exact)
        assert torch.equal(got[m].view(P.INT_VIEW[dtype]), once[m].view(P.INT_VIEW[dtype])), order
        checked += int(m.sum())
    assert checked > 5000


@pytest.mark.parametrize("quant,dtype,floor", [("nf4", BF, 22790), ("fp4", BF, 824), ("nf4", HF, 6820), ("fp4", HF, 3452)])
def test_post_scaled_and_pre_scaled_orders_disagree(quant, dtype, floor):
    """Orders A and B16 differ on at least the stated number of the 196 096 (code, scale, v) cells: a family filed under the wrong
    order of the ledger fails its probe. The fp32 table of A32 moves further cells."""
    c, s, v = _grid(quant)
    a, a32, b = (C.restate(o, c, s, v, dtype) for o in ("A", "A32", "B16"))
    assert a.numel() == 196096
    assert _differ(a, b) >= floor
    assert _differ(a, a32) >= 150 and _differ(a32, b) >= 600


@pytest.mark.parametrize("quant,floor", [("nf4", 550), ("fp4", 612)])
def test_fp32_orders_disagree(quant, floor):
    c, s, v = _grid(quant)
    assert _differ(C.restate("A32", c, s, v, F32), C.restate("B32", c, s, v, F32)) >= floor


def test_the_issue_s_two_examples():
    """fp16, scale 2^18, code 0.25, x = 0.5: 32768 post-scaled, inf pre-scaled. fp32, scale 2^-148, code 0.25, x = 4: 2^-148
    post-scaled, 0 pre-scaled."""
    t = lambda x: torch.tensor([x], dtype=torch.float32)
    assert float(C.restate("A", t(0.25), t(2.0 ** 18), t(0.5), HF)) == 32768.0
    assert float(C.restate("B16", t(0.25), t(2.0 ** 18), t(0.5), HF)) == float("inf")
    assert float(C.restate("A32", t(0.25), t(2.0 ** -148), t(4.0), F32)) == 2.0 ** -148
    assert float(C.restate("B32", t(0.25), t(2.0 ** -148), t(4.0), F32)) == 0.0


def test_ledger_names_every_family():
    fams = set(P.COPIES) | {"generic"}
    assert set(C.ORDER) == fams == set(C.CASES) == set(C.DENSE) == set(C.NESTED_DENSE)
    for fam, per in C.ORDER.items():
        assert set(per.values()) <= set(C.ORDERS)
        assert {cs.dtype for cs in C.CASES[fam]} == set(per), fam
    for fam in fams:
        # parts 1, 2 and 3 have a case of every family; blocksize 4096 or a written reason
        assert C.CASES[fam] and C.DENSE[fam]
        assert any(cs.blocksize == 4096 for cs in C.CASES[fam]) or len(C.NO_BS4096[fam]) > 20
        assert any(cs.nested for cs in C.CASES[fam]) and any(not cs.nested for cs in C.CASES[fam])
        for quant in ("nf4", "fp4"):
            assert any(cs.quant == quant for cs in C.CASES[fam])
    for fam in ("rt", "kq", "pc", "grad_input"):   # the families that split their contraction over workgroups
        for dt in (BF, HF):
            assert any(dc.split and dc.dtype == dt for dc in C.DENSE[fam]), fam
    assert any(cs.blocksize == 32 for cs in C.CASES["rt"])
    assert {cs.rows for cs in C.CASES["sm"]} >= {2, 5, 16} and {cs.rows for cs in C.CASES["stream"]} == {0, 1}
    assert {cs.plan for cs in C.CASES["grad_input"]} == {"single", "sliced"}
    assert all(cs.E == 3 for cs in C.CASES["experts"])
    assert all(cs.N == 1040 for fam in ("stream", "generic", "sm", "rt", "kq", "pc", "tall") for cs in C.CASES[fam])


# ------------------------------------------------------------------------------------------ part 1: coverage
def _scale_ids(values: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """Index into ``table`` (distinct fp32 values, by bit pattern) of every element of ``values``; -1 where it is not in the table."""
    tb = table.contiguous().view(torch.int32).long()
    order = torch.argsort(tb)
    vb = values.contiguous().view(torch.int32).long()
    pos = torch.searchsorted(tb[order], vb).clamp(max=tb.numel() - 1)
    return torch.where(tb[order][pos] == vb, order[pos], torch.full_like(pos, -1))


def _run_wants(cs, pr, ks):
    """(want, overlaid, own) of one run of a case, each [weight rows, len(ks)] - aligned with ``pr.scale_full[:, ks]``: what the GPU
    test compares with, the cells that want_forward / want_backward overlaid with NaN (they compare nothing of their own term), and
    the cell's own term in the family's order before the overlay."""
    order = C.order_of(cs.family, cs.dtype)
    if cs.family == "grad_input":
        _, v = P.one_hot_rows(ks, cs.N, cs.dtype)       # (ks: the probed weight rows, all of them)
        want, over = C.want_backward(pr, ks, v, overlay=True)
        own = C.restate(order, pr.code_full, pr.scale_full, v.float()[:, None], cs.dtype)
        return want, over, own
    _, v = P.one_hot_rows(ks, cs.K, cs.dtype)
    per = [C.want_forward(pr, ks, v, expert=e, overlay=True) for e in range(cs.E)]
    want, over = (torch.cat([p[i] for p in per], dim=1).t() for i in (0, 1))
    own = C.restate(order, pr.code_full[:, ks], pr.scale_full[:, ks], v.float()[None, :], cs.dtype)
    return want, over, own


def _assert_floor(cs, what, want, over, own):
    """Every run of every case: of the cells whose own term is finite and not zero in the family's order - what the number formats
    leave to compare - at most half are overlaid with NaN. (The share of such terms is the formats' own: fp16 holds 2^-24 ... 2^15
    of the 255 exponents, so most fp16 wants are zeros and infinities whatever the kernel does.)"""
    testable = torch.isfinite(own.float()) & (own.float() != 0)
    kept = testable & ~over
    assert bool((torch.isnan(want) == (over | torch.isnan(own)))[~over].all())
    assert int(kept.sum()) * 2 >= int(testable.sum()), f"{what}: {int(kept.sum())} of {int(testable.sum())} finite non-zero terms are compared"
    return int(kept.sum()), int(testable.sum())


@pytest.mark.parametrize("cs", [cs for cs in C.ALL_CASES if not cs.nested], ids=_id)
def test_plain_case_meets_every_scale_with_every_code_in_both_nibbles(cs):
    """Coverage counts a (scale, nibble, code) cell only where the want is the cell's own term, not the NaN overlay of another
    term. Order B16 rounds code * scale to T: a scale T does not hold makes inf weights, which no probe of their row (forward) or
    column (backward) survives; those scales are counted by position, every other scale by un-overlaid wants."""
    fin = R.finite_scales()
    assert fin.numel() == 1530
    seen = torch.zeros(fin.numel(), 2, 16, dtype=torch.bool)
    compared = torch.zeros_like(seen)
    backward = cs.family == "grad_input"
    ks = torch.arange(cs.N if backward else cs.K) if backward else C.probe_ks(cs)
    kcols = torch.arange(cs.K) if backward else ks
    assert torch.unique(kcols % 64).numel() == min(64, cs.K), "a k position inside a 64-group is never probed"
    held = torch.isfinite(fin.to(cs.dtype).float()) if C.order_of(cs.family, cs.dtype) == "B16" else torch.ones(fin.numel(), dtype=torch.bool)
    assert int(held.sum()) >= 850
    kept_cells = 0
    for fi in range(cs.fills):
        pr = C.build(cs, fi)
        sf = pr.scale_full[:, kcols]
        probed_blocks = torch.unique(((torch.arange(cs.weight_rows)[:, None] * cs.K + kcols[None, :]) // cs.blocksize))
        assert probed_blocks.numel() == pr.scale.numel(), "a block is never probed"
        want, over, own = _run_wants(cs, pr, ks)
        kept_cells += _assert_floor(cs, f"fill {fi}", want, over, own)[0]
        finite = torch.isfinite(sf)
        ids = _scale_ids(sf, fin)
        assert bool((ids[finite] >= 0).all())
        nib, code = (kcols % 2).expand(sf.shape[0], -1), pr.nibbles[:, kcols].long()
        seen[ids[finite], nib[finite], code[finite]] = True
        m = finite & ~over
        compared[ids[m], nib[m], code[m]] = True
        # the non-finite scales: +inf and NaN, in dedicated rows, never the only content of the case
        bad_rows = C.nonfinite_columns(pr) if cs.E == 1 else (~torch.isfinite(pr.scale_full)).any(dim=1)
        assert 4 <= int(bad_rows.sum()) <= 4 * max(1, -(cs.blocksize // -cs.K)) + 4 < cs.weight_rows // 4
        assert bool(torch.isinf(pr.scale).any()) and bool(torch.isnan(pr.scale).any())
        if backward:   # every non-finite weight of the case lies in the poisoned block columns; the other columns compare everything
            cols = C.poison_columns(cs).repeat_interleave(cs.blocksize)
            assert not bool(over[:, ~cols].any()), "a NaN overlay outside the poisoned block columns"
            assert int((~cols).sum()) * 2 >= cs.K
        if cs.K % cs.blocksize == 0 and cs.K // cs.blocksize > 1:
            s2 = pr.scale.view(cs.weight_rows, -1)
            e = torch.frexp(s2)[1]
            ok = torch.isfinite(s2[:, 1:]) & torch.isfinite(s2[:, :-1])
            assert bool((s2[:, 1:] != s2[:, :-1])[ok].all()), "neighbouring blocks of a row share a scale"
            # (the few scales bf16 does not hold are one exponent: the class behind the others)
            assert float(((e[:, 1:] - e[:, :-1]).abs()[ok] >= 16).float().mean()) > 0.95, "neighbouring blocks of a row are close in exponent"
    assert bool(seen.all()), f"{int((~seen).sum())} (scale, nibble, code) cells are never probed"
    assert bool(compared[held].all()), f"{int((~compared[held]).sum())} (scale, nibble, code) cells are probed under a NaN overlay only"
    assert kept_cells > 0


@pytest.mark.parametrize("cs", [cs for cs in C.ALL_CASES if cs.nested], ids=_id)
def test_nested_case_meets_every_second_level_scale(cs):
    am2 = R.nested_absmax2()
    assert am2.numel() == 383
    backward = cs.family == "grad_input"
    b16 = C.order_of(cs.family, cs.dtype) == "B16"
    pr = C.build(cs, 0, 0.03)
    groups = pr.absmax.numel()
    # the second-level scales whose weights T holds under order B16 (every one under the other orders)
    held = torch.isfinite((2 * am2).to(cs.dtype).float()) if b16 else torch.ones(383, dtype=torch.bool)
    held = held if int((~held).sum()) >= 16 else torch.ones(383, dtype=torch.bool)
    assert int(held.sum()) >= 190
    if backward:   # no non-finite second-level scale (a group spans every block column), none T does not hold
        assert groups >= 386 and torch.equal(pr.absmax[:383][held], am2[held]) and bool(torch.isfinite(pr.absmax).all())
        assert bool(torch.isfinite((2 * pr.absmax).to(cs.dtype).float()).all()) or cs.dtype == BF
    else:
        assert groups >= 386 and torch.equal(pr.absmax[:383], am2)
        assert int(torch.isinf(pr.absmax).sum()) == 1 and int(torch.isnan(pr.absmax).sum()) == 1
    q8 = pr.absmax_8bit.long()
    full = q8[:(q8.numel() // 256) * 256].view(-1, 256)
    assert bool((torch.sort(full, dim=1)[0] == torch.arange(256)).all()), "a group does not hold every 8-bit code"
    assert bool((q8[1:] != q8[:-1]).all())
    assert torch.unique(pr.absmax_code).numel() == 256
    # the scale is the two-rounding reconstruction, in separate fp32 operations
    prod = pr.absmax_code[q8] * pr.absmax.repeat_interleave(256)[:q8.numel()]
    assert R.same_bits(pr.scale, prod + torch.tensor(0.03))
    fused = (pr.absmax_code[q8].double() * pr.absmax.repeat_interleave(256)[:q8.numel()].double() + 0.03).float()
    assert _differ(pr.scale, fused) > (500 if backward and cs.dtype == HF else 1000), "one fused multiply-add would pass: the two roundings are not tested"
    ks = torch.arange(cs.N) if backward else C.probe_ks(cs)
    kcols = torch.arange(cs.K) if backward else ks
    assert torch.unique(kcols % 64).numel() == 64
    flat = (torch.arange(cs.weight_rows)[:, None] * cs.K + kcols[None, :]) // cs.blocksize
    assert torch.unique(flat).numel() == pr.scale.numel(), "a block is never probed"
    nib, code = (kcols % 2).expand(flat.shape[0], -1), pr.nibbles[:, kcols].long()
    seen = torch.zeros(groups, 2, 16, dtype=torch.bool)
    seen[flat // 256, nib, code] = True
    # (the last group may hold a few blocks only: one of those to spare)
    assert bool(seen[:groups - 1].all()), "a second-level scale does not meet every code in both nibbles"
    assert len(R.OFFSETS) == 5
    # per offset: the floor, and the coverage over wants that are the cell's own term
    counted = torch.zeros(groups, dtype=torch.bool)
    counted[:383] = held
    for off in R.OFFSETS:
        pr = C.build(cs, 0, off)
        want, over, own = _run_wants(cs, pr, ks)
        kept, testable = _assert_floor(cs, f"offset {off!r}", want, over, own)
        if b16 and not bool(torch.isfinite((pr.scale[torch.isfinite(pr.scale)].abs().min() * 0.25).to(cs.dtype).float())):
            assert testable == 0    # (fp16 under the offset 2^100: every weight is inf, nothing can be compared)
            continue
        if backward:
            assert float(over.float().mean()) < 0.25, f"offset {off!r}: {float(over.float().mean()):.3f} of the wants are the NaN overlay"
        compared = torch.zeros_like(seen)
        m = ~over
        compared[(flat // 256)[m], nib[m], code[m]] = True
        assert bool(compared[counted].all()), f"offset {off!r}: {int((~compared[counted]).sum())} (group, nibble, code) cells are probed under a NaN overlay only"


def test_bytes_hold_every_code_in_every_block():
    for cs in (C.CASES["stream"][0], C.CASES["rt"][4], C.CASES["experts"][0], C.CASES["generic"][0]):
        b = C.build_bytes(cs)
        run = b.reshape(-1, 16) if (cs.K // 2) % 16 == 0 else b[:, :(cs.K // 2) // 16 * 16].reshape(-1, 16)
        assert bool((torch.sort(run >> 4, dim=1)[0] == torch.arange(16)).all()) and bool((torch.sort(run & 15, dim=1)[0] == torch.arange(16)).all())


@pytest.mark.parametrize("cs", [C.CASES["stream"][0], C.CASES["tall"][2], C.CASES["tall"][-1], C.CASES["stream"][5], C.CASES["generic"][0],
                                C.CASES["sm"][3], C.CASES["rt"][4], C.CASES["kq"][-1]], ids=_id)
def test_forward_want_is_the_dense_product_in_the_family_s_order(cs):
    """want_forward's shortcut (one term, NaN overlay) against the whole contraction written out: every term x[m, k] * w[n, k] in the
    family's order, summed in float64 (a sum of zeros and one term, or a NaN)."""
    pr = C.build(cs, 0, 0.03)
    # (a stride over the probes, and every probe of the first and of the last 64-group: the dedicated non-finite blocks themselves)
    ks = torch.unique(torch.cat([C.probe_ks(cs)[::7][:24], C.probe_ks(cs)[:4], C.probe_ks(cs)[-4:]]))
    x, v = P.one_hot_rows(ks, cs.K, cs.dtype)
    want = C.want_forward(pr, ks, v)
    order = C.order_of(cs.family, cs.dtype)
    c, s = pr.code_full[None], pr.scale_full[None]          # [1, N, K]
    xf = x.float()[:, None, :]                               # [P, 1, K]
    if order in ("A", "A32"):
        cc = c.to(cs.dtype).float() if order == "A" else c
        # a granule's partial sum (one term or zero) times its block's scale
        g = C.granule(cs.family, cs.blocksize)
        assert cs.K % g == 0
        terms = (cc * xf).view(xf.shape[0], c.shape[1], -1, g).sum(dim=3) * s.view(1, s.shape[1], -1, g)[..., 0]
    elif order == "B16":
        terms = (c * s).to(cs.dtype).float() * xf
    else:
        terms = (c * s) * xf
    dense = terms.double().sum(dim=2).float().to(cs.dtype)
    assert R.same_bits(want, dense), R.first_mismatch(want, dense)
    cols = C.nonfinite_columns(pr)
    assert not bool(torch.isfinite(want[:, cols].float()).any()) and int(cols.sum()) >= 4
    assert int(torch.isfinite(want.float()).sum()) > want.numel() // 3, "too few finite probes survive"


@pytest.mark.parametrize("cs", [C.CASES["grad_input"][0], C.CASES["grad_input"][3], C.CASES["grad_input"][7]], ids=_id)
def test_backward_want_is_the_dense_product(cs):
    pr = C.build(cs)
    ns = torch.arange(cs.N)
    g, v = P.one_hot_rows(ns, cs.N, cs.dtype)
    want = C.want_backward(pr, ns, v)
    w = (pr.code_full * pr.scale_full).to(cs.dtype).float()
    dense = (g.float()[:, :, None] * w[None, :, :]).double().sum(dim=1).float().to(cs.dtype)
    assert R.same_bits(want, dense), R.first_mismatch(want, dense)
    assert int(torch.isfinite(want.float()).sum()) > want.numel() // 2


# ------------------------------------------------------------------------------------------ part 2: windows
@pytest.mark.parametrize("dc", C.ALL_DENSE, ids=_id)
def test_windows_are_exact_in_every_order(dc):
    assert set(C.WINDOWS[dc.dtype]) == ({"bottom", "top", "top-inf"} if dc.dtype == HF else {"bottom", "top"})
    tiny = {F32: 2.0 ** -149, BF: 2.0 ** -133, HF: 2.0 ** -24}[dc.dtype]
    for window, (lo, hi) in C.WINDOWS[dc.dtype].items():
        di = C.window_inputs(dc, window)          # asserts the exact-sum bound and worst < 2^128
        ex = di.ex
        assert ex.unit == 2.0 ** (lo - 2) and (window != "bottom" or ex.unit == tiny)
        e = torch.frexp(ex.scale)
        assert bool((e[0] == 0.5).all()) and int(e[1].min()) - 1 == lo and int(e[1].max()) - 1 == hi
        assert not bool(ex.bias.any())
        assert C.orders_agree(ex), (dc.name, window)
        assert di.worst < 2.0 ** 24 * ex.unit and di.worst < 2.0 ** 128
        assert dc.K <= 1024 or dc.family == "rt", "only the two-slice form of the rt kernel needs longer rows"
        # the packed nibbles decode to W bit for bit
        fp4 = P.code_table("fp4")
        q = di.packed.reshape(-1).long()
        nib = torch.stack([q >> 4, q & 15], dim=1).reshape(ex.W.shape)
        w = (fp4[nib] * ex.scale.view(ex.N, -1).repeat_interleave(ex.blocksize, dim=1)).to(dc.dtype)
        assert torch.equal(w.view(P.INT_VIEW[dc.dtype]), ex.W.view(P.INT_VIEW[dc.dtype]))
        ref = di.reference().float()
        if window == "top-inf":
            assert 0.02 < float(torch.isinf(ref).float().mean()) < 0.99, "the fp16 (10, 15) window wants infinities and finite values"
        elif not (dc.dtype == HF and window == "top"):   # (fp16 (4, 9): the longest rows overflow a few sums - correctly)
            assert bool(torch.isfinite(ref).all())
        if window == "bottom":
            sub = (ref != 0) & (ref.abs() < torch.finfo(dc.dtype).tiny)
            assert int(sub.sum()) > 0, "no subnormal result"


def test_assert_exact_sums_keeps_its_fp16_condition_by_default():
    dc = next(d for d in C.DENSE["sm"] if d.dtype == HF)
    di = C.window_inputs(dc, "top-inf")
    with pytest.raises(AssertionError, match="fp16 range"):
        X.assert_exact_sums(di.ex.W, di.ex.x, di.ex.unit, HF)
    X.assert_exact_sums(di.ex.W, di.ex.x, di.ex.unit, HF, allow_fp16_overflow=True)


# ------------------------------------------------------------------------------------------ part 3: poison positions
@pytest.mark.parametrize("dc", [d for d in C.ALL_DENSE] + [d for d in C.NESTED_DENSE.values() if d is not None], ids=_id)
def test_poison_positions(dc):
    di = C.clean_inputs(dc)
    assert bool(torch.isfinite(di.reference(True).float()).all())
    bpr = dc.K // dc.blocksize
    blocks = C.poison_blocks(dc)
    assert len(set(blocks.values())) == 6 and max(blocks.values()) == dc.weight_rows * bpr - 1
    assert blocks["first-of-row"] % bpr == 0 and blocks["last-of-row"] % bpr == bpr - 1
    cut = dc.k_boundary // dc.blocksize
    assert blocks["before-k-cut"] % bpr == cut - 1 and blocks["after-k-cut"] % bpr == cut
    assert blocks["ragged-tile"] // bpr == dc.weight_rows - 2
    assert dc.N % 32 != 0 or dc.family == "grad_input"   # (the fused backward takes whole 64-row blocks of the weight only)
    acts = C.poison_activations(dc)
    width = dc.N if dc.family == "grad_input" else dc.K
    assert {m for m, _, _ in acts} >= {0, dc.M - 1} and all(0 <= m < dc.M and 0 <= c < width for m, c, _ in acts)
    assert {c for _, c, _ in acts} >= {3, width - 1} and len(acts) >= 6
    vals = [v for _, _, v in acts]
    assert float("inf") in vals and float("-inf") in vals and any(v != v for v in vals)
    if dc.nested:
        assert di.ex.absmax2.numel() >= 2 and di.ex.absmax_8bit is not None
