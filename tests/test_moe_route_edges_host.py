"""CPU (-m "not gpu"): the preconditions of every input of tests/moe_route_edge_cases.py, and the fp32 torch composition
(``_moe_topk_composition``, what ``bitsandbytes_amd.moe_topk`` runs on CPU tensors) against the float64 reference on each of them - so
what tests/test_gpu_moe_route_edges.py expects of the kernel is proven without a GPU: every ranking is unambiguous or its ambiguity
is counted and capped, and an fp32 implementation reproduces every reference id."""
import pytest
import torch

import moe_route_cases as C
import moe_route_edge_cases as EC

EDGES = EC.structured_edges()


def _composition(edge, renormalize=None):
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    with torch.no_grad():
        return _moe_topk_composition(edge.logits, edge.S, edge.scoring, edge.renormalize if renormalize is None else renormalize, edge.scale,
                                     edge.bias)


def test_the_builders_cover_what_they_name():
    names = [e.name for e in EDGES]
    assert len(set(names)) == len(names)
    assert {e.E for e in EC.position_edges()} == {64, 128, 256, 512, 1024} and all(e.logits.shape == (e.E, e.E) and e.S == 3 for e in EC.position_edges())
    assert {(e.E, e.S) for e in EC.one_lane_edges()} == set(EC.ONE_LANE) and all(e.logits.shape[0] == 64 for e in EC.one_lane_edges())
    assert {e.E for e in EC.tie_edges()} == set(C.ES) and {e.E for e in EC.tie_edges() if e.bias is not None} == {E for E in C.ES if E >= 66}
    assert {C.lane_slots(e.E) for e in EC.tie_edges()} == {1, 2, 4, 8, 16}
    for group in (EC.position_edges(), EC.one_lane_edges(), EC.tie_edges(), EC.nonfinite_edges()):
        assert {e.scoring for e in group} == set(C.SCORINGS)
    assert {e.renormalize for e in EC.one_lane_edges()} == {True, False}
    assert max(e.logits.numel() * e.logits.element_size() for e in EDGES) == 4 << 20
    assert EC.MASK_LIVE == (11, 8, 6, 1, 0) and EC.long_batch_edge().logits.shape == (4099, 8)
    assert EC.long_batch_base().name == "E8-S2-T37-float32-softmax-renorm-nobias"


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: e.name)
def test_ranking_is_unambiguous_and_the_composition_reproduces_it(edge):
    """float64 is the one right answer for the ids: by the ranked grid's own rule where the logits are ordinary, by classes
    otherwise. Then the fp32 composition on the CPU: ids exactly, weights within :func:`_bound` by the edge module's error metric,
    NaN / 0 exactly where the reference has them."""
    if edge.ordinary:
        gap = C.assert_unambiguous(edge.logits, edge.scoring, edge.bias)
    else:
        gap = EC.assert_classes_unambiguous(edge)
    assert gap > C.KEY_GAP
    assert edge.ids.shape == edge.weights.shape == (edge.logits.shape[0], edge.S)
    assert all(len(set(r)) == edge.S for r in edge.ids[:64].tolist()) and bool(((edge.ids >= 0) & (edge.ids < edge.E)).all())
    ids, w = _composition(edge)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids, edge.ids)
    assert EC.weight_err(w, edge.weights) <= _bound(edge.E, edge.scoring)


def _bound(E, scoring):
    """What any fp32 evaluation keeps, in units of 2^-24: WEIGHT_FLOOR's 16 for argument rounding, expf, the division (and a
    renormalizing sum of at most 17 terms); under softmax E - 1 more, the worst case of an fp32 sum of E positive terms in whatever
    order the library adds them. The tight rule - the kernel against this composition on the same GPU - is the GPU file's."""
    return C.WEIGHT_FLOOR + (E - 1) * 2.0 ** -24 if scoring == "softmax" else C.WEIGHT_FLOOR


def test_the_stated_gaps():
    """The smallest float64 key gaps of the constructions, as the issue that asked for them states them: positions at least 2.3e-3
    (sigmoid) and 0.034 (softmax); one lane at least 2.3e-3 (sigmoid) and 2.65e-3 (softmax, at E = 1024)."""
    gaps = {sc: min(C.assert_unambiguous(e.logits, sc, None) for e in EC.position_edges() if e.scoring == sc) for sc in C.SCORINGS}
    assert 2.3e-3 <= gaps["sigmoid"] < 2.4e-3 and 0.034 <= gaps["softmax"] < 0.035, gaps
    gaps = {sc: min(C.assert_unambiguous(e.logits, sc, None) for e in EC.one_lane_edges() if e.scoring == sc) for sc in C.SCORINGS}
    assert 2.3e-3 <= gaps["sigmoid"] < 2.4e-3 and 2.65e-3 <= gaps["softmax"] < 2.7e-3, gaps
    assert 2.65e-3 <= C.assert_unambiguous(EC.one_lane_edge(1024, 16, "softmax", False).logits, "softmax", None) < 2.7e-3


def test_whole_row_ties_and_masks_say_what_they_should():
    for e in EC.tie_edges():
        if e.scoring == "softmax":   # float64 agrees with the bits the kernel must give to within fp32 rounding
            want = torch.tensor([EC.tie_softmax_bits(e.E)], dtype=torch.int32).view(torch.float32).double()
            assert bool(((e.weights - want).abs() <= want * 2.0 ** -24).all())
    for E in EC.MASK_ES:
        for sc in C.SCORINGS:
            for live in EC.MASK_LIVE:
                e = EC.mask_edge(E, sc, live)
                finite = torch.isfinite(e.logits)
                assert finite.sum(-1).tolist() == [live] * 4
                for t in range(4):
                    row, k = e.ids[t].tolist(), min(live, e.S)
                    assert all(bool(finite[t, j]) for j in row[:k]) and row[k:] == [j for j in range(E) if not finite[t, j]][:e.S - k]
                if live == 0:
                    assert bool(torch.isnan(e.weights).all()) if sc == "softmax" else bool((e.weights == 0).all())
                else:
                    assert bool((e.weights[:, min(live, e.S):] == 0).all()) and bool((e.weights[:, :min(live, e.S)] > 0).all())
        assert bool(torch.isnan(EC.mask_edge(E, "sigmoid", 0, True).weights).all())
        e = EC.nan_logit_edge(E, "sigmoid")
        for t in range(3):
            row = e.ids[t].tolist()
            assert not bool(torch.isnan(e.logits[t, row[:12]]).any()) and row[12:] == torch.isnan(e.logits[t]).nonzero().flatten()[:4].tolist()
        assert bool(torch.isnan(e.weights[:, 12:]).all()) and bool(torch.isfinite(e.weights[:, :12]).all())
        e = EC.nan_logit_edge(E, "softmax")
        assert e.ids.tolist() == [list(range(16))] * 3 and bool(torch.isnan(e.weights).all())
        e = EC.inf_logit_edge(E, "sigmoid")
        assert all(e.ids[r, 0] == c and e.weights[r, 0] == 1.0 for r, c in EC.INF_AT) and bool(torch.isfinite(e.weights).all())
        e = EC.inf_logit_edge(E, "softmax")
        assert all(e.ids[r].tolist() == list(range(8)) and bool(torch.isnan(e.weights[r]).all()) for r, _ in EC.INF_AT)
        assert bool(torch.isfinite(e.weights[[0, 2]]).all())


@pytest.mark.parametrize("dtype", EC.SWEEP_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_sigmoid_sweep_on_the_composition(dtype):
    e = EC.sigmoid_sweep(dtype)
    assert e.logits.shape == (65536, 1) and torch.equal(e.logits.view(torch.int16).flatten().int() & 0xFFFF, torch.arange(65536, dtype=torch.int32))
    ids, w = _composition(e)
    assert bool((ids == 0).all()) and bool((e.ids == 0).all())
    assert EC.weight_err(w, e.weights) <= C.WEIGHT_FLOOR
    _, wn = _composition(e, renormalize=True)
    EC.check_sigmoid_renormalized(w, wn)
    # the float64 reference states the same rule: 1 or NaN
    ref = EC.sigmoid_sweep(dtype, True).weights
    assert bool(((ref == 1.0) | torch.isnan(ref)).all()) and torch.equal(torch.isnan(ref), ~(e.weights > 0))


# Finite patterns whose softmax order is not asserted: 0 > l >= -2e-3 (|p0 - p1| = tanh(|l| / 2) <= KEY_GAP). A property of the number
# format: every fp16 / bf16 pattern from the smallest denormal up to 2e-3, one sign.
#   float16: 6168 of 63488 finite patterns (9.7 %);  bfloat16: 15107 of 65280 (23.1 %)
# By |p0 - p1| <= KEY_GAP alone - both signs - the counts are 12336 (19.4 %) and 30214 (46.3 %): bf16 spends 40 % of its exponents
# below 2^-25, where expf(l) rounds to 1 in fp32. No fp32 router can follow float64 there, so no cap below that share can hold for
# bf16; the positive half is asserted by the argument in moe_route_edge_cases.softmax_sweep instead.
SWEEP_FINITE = {torch.float16: 63488, torch.bfloat16: 65280}
SWEEP_CLOSE = {torch.float16: 12336, torch.bfloat16: 30214}
SWEEP_OPEN = {torch.float16: 6168, torch.bfloat16: 15107}


@pytest.mark.parametrize("dtype", EC.SWEEP_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_softmax_sweep_unasserted_orders_are_counted(dtype):
    s = EC.softmax_sweep(dtype)
    l = s.logits[:, 0].double()
    assert int(s.finite.sum()) == SWEEP_FINITE[dtype]
    assert int(s.close.sum()) == SWEEP_CLOSE[dtype]
    unasserted = s.finite & ~s.ranked
    assert int(unasserted.sum()) == SWEEP_OPEN[dtype]
    assert bool(((l[unasserted] < 0) & (l[unasserted] >= -2.0e-3 * 1.001)).all())
    if dtype == torch.float16:
        assert SWEEP_OPEN[dtype] < 0.15 * SWEEP_FINITE[dtype]
    # what is asserted where: +-0 and every non-finite pattern are ranked; the expectations for them
    ids = s.ids.tolist()
    zero, neg_inf = [v for v in range(65536) if l[v] == 0], [v for v in range(65536) if l[v] == -EC.INF]
    assert len(zero) == 2 and len(neg_inf) == 1 and bool(s.ranked[~s.finite].all()) and bool(s.ranked[zero].all())
    assert all(ids[v] == [0, 1] for v in zero) and ids[neg_inf[0]] == [1, 0] and s.p[neg_inf[0]].tolist() == [0.0, 1.0]
    bad = ~s.finite & (l != -EC.INF)
    assert bool((s.ids[bad] == torch.tensor([0, 1], dtype=torch.int32)).all()) and bool(torch.isnan(s.p[bad]).all())


@pytest.mark.parametrize("dtype", EC.SWEEP_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_softmax_sweep_on_the_composition(dtype):
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    s = EC.softmax_sweep(dtype)
    with torch.no_grad():
        ids, w = _moe_topk_composition(s.logits, 2, "softmax", False, 1.0, None)
    assert EC.check_softmax_sweep(s, ids, w) <= C.WEIGHT_FLOOR


def test_placement_on_the_composition():
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    logits = EC.placement_logits()
    assert logits.shape == (64, 1024) and logits.dtype == torch.float16
    with torch.no_grad():
        ids, w = _moe_topk_composition(logits, 1, "sigmoid", False, 1.0, None)
    assert EC.check_placement(ids, w) <= C.WEIGHT_FLOOR
    # the rows of the non-finite patterns: +inf leads its row with exactly 1; -inf leads the row it shares with NaN only, with 0
    assert ids[31].item() == 0 and w[31].item() == 1.0 and ids[63].item() == 0 and w[63].item() == 0.0
