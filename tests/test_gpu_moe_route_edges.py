"""GPU: the MoE router's scoring + top-k launch (bitsandbytes_amd::moe_topk, csrc/moe_route.hip) on the structured inputs of
tests/moe_route_edge_cases.py - a winner at every (lane, slot), one lane that supplies every winner, whole-row ties, masks and
non-finite keys, every 16-bit logit value, a long batch - and ``bitsandbytes_amd.moe_topk`` on views, a 16-bit bias and a shape past
the launch. The preconditions of every input, and the fp32 composition on the CPU against the same expectations, are
tests/test_moe_route_edges_host.py's.

* ids: ``torch.equal`` with the float64 ranking (ties to the lower index; finite keys, then -inf keys, then NaN keys by index). Only
  the 16-bit sweep over softmax rows [l, 0] states a condition, in moe_route_edge_cases.softmax_sweep.
* weights: ``err = |w - w64| / max(|w64|, 2^-100)``, NaN exactly where float64 has NaN and 0 exactly where it has 0; the kernel's
  maximum over a test's inputs at most WEIGHT_FACTOR x the maximum of torch's fp32 composition on the same inputs on this GPU,
  floor WEIGHT_FLOOR (moe_route_cases). Each test prints both maxima; profiles/moe_route.txt records them.
The op has no fall-back: it raises where it has no kernel."""
import functools

import pytest
import torch

import moe_route_cases as C
import moe_route_edge_cases as EC

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.moe_topk.default


def _composition(logits, S, scoring, renormalize, scale, bias):
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    return _moe_topk_composition(logits, S, scoring, renormalize, scale, bias)


def _run(fn, logits, S, scoring, renormalize, scale, bias):
    ids, w = fn(logits.to(DEV), S, scoring, renormalize, scale, None if bias is None else bias.to(DEV))
    return ids.cpu(), w.cpu()


@functools.lru_cache(maxsize=None)
def _result(edge_name):
    """One edge, once: (kernel ids, kernel weights, composition ids, composition weights), on the CPU."""
    e = EDGE[edge_name]
    return _run(_op(), e.logits, e.S, e.scoring, e.renormalize, e.scale, e.bias) + _run(_composition, e.logits, e.S, e.scoring, e.renormalize, e.scale, e.bias)


def _within(what, err_kernel, err_torch):
    bound = max(C.WEIGHT_FACTOR * err_torch, C.WEIGHT_FLOOR)
    print(f"moe_topk weights, {what}: max err against float64: kernel {err_kernel:.3e}, torch fp32 composition {err_torch:.3e}, bound {bound:.3e}")
    assert err_kernel <= bound


def _check_ids(edge):
    ids, w, cids, _ = _result(edge.name)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == edge.ids.shape
    assert torch.equal(ids, edge.ids), f"first differing row: {int((ids != edge.ids).any(-1).nonzero()[0])}"
    assert torch.equal(cids, edge.ids), "the torch composition on the GPU does not give the float64 ranking"


def _check_weights(what, edges):
    """The rule of the file head over a group of edges."""
    err_kernel = max(EC.weight_err(_result(e.name)[1], e.weights) for e in edges)
    err_torch = max(EC.weight_err(_result(e.name)[3], e.weights, strict=False) for e in edges)
    _within(f"{what} ({len(edges)} inputs)", err_kernel, err_torch)


POSITIONS, ONE_LANE, TIES, NONFINITE = EC.position_edges(), EC.one_lane_edges(), EC.tie_edges(), EC.nonfinite_edges()
EDGE = {e.name: e for e in POSITIONS + ONE_LANE + TIES + NONFINITE + [EC.long_batch_edge()]}
_name = lambda e: e.name


# ------------------------------------------------------------------------------------------ 2a, 2b: where a winner sits
@pytest.mark.parametrize("edge", POSITIONS, ids=_name)
def test_a_winner_at_every_lane_and_slot(edge):
    _check_ids(edge)


def test_position_weights():
    _check_weights("a winner at every (lane, slot)", POSITIONS)


@pytest.mark.parametrize("edge", ONE_LANE, ids=_name)
def test_one_lane_supplies_every_winner(edge):
    _check_ids(edge)


def test_one_lane_weights():
    _check_weights("one lane supplies every winner", ONE_LANE)


# ------------------------------------------------------------------------------------------ 2c: ties
@pytest.mark.parametrize("edge", TIES, ids=_name)
def test_whole_row_ties_go_by_index(edge):
    _check_ids(edge)
    if edge.scoring == "softmax":
        # expf(0) = 1, E ones sum exactly, IEEE division: the bits of 1.0f / E, whatever the level of the row and with or without a bias
        w = _result(edge.name)[1]
        assert bool((w.view(torch.int32) == EC.tie_softmax_bits(edge.E)).all()), (w.view(torch.int32).unique().tolist(), EC.tie_softmax_bits(edge.E))
    else:
        w = _result(edge.name)[1]
        assert all(len(row.unique()) == 1 for row in w.view(torch.int32))


def test_tie_weights():
    _check_weights("whole-row ties", TIES)


# ------------------------------------------------------------------------------------------ 2d: masks and non-finite keys
@pytest.mark.parametrize("edge", NONFINITE, ids=_name)
def test_masks_and_non_finite_keys(edge):
    _check_ids(edge)
    w = _result(edge.name)[1]
    EC.weight_err(w, edge.weights)   # NaN where float64 has NaN, 0 where it has 0 (a masked expert), finite elsewhere
    if edge.name.startswith("inflogit") and edge.scoring == "sigmoid":
        assert all(w[r, 0].item() == 1.0 for r, _ in EC.INF_AT)
    if edge.name.startswith("huge"):
        assert w.tolist() == [[0.5, 0.5, 0.0, 0.0]]


def test_non_finite_weights():
    _check_weights("masks and non-finite keys", NONFINITE)


# ------------------------------------------------------------------------------------------ 2e: every 16-bit logit value
@pytest.mark.parametrize("dtype", EC.SWEEP_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_every_16_bit_logit_through_sigmoid(dtype):
    e = EC.sigmoid_sweep(dtype)
    ids, w = _run(_op(), e.logits, 1, "sigmoid", False, 1.0, None)
    _, cw = _run(_composition, e.logits, 1, "sigmoid", False, 1.0, None)
    assert bool((ids == 0).all())
    _within(f"65536 {dtype} patterns, sigmoid", EC.weight_err(w, e.weights), EC.weight_err(cw, e.weights, strict=False))
    ids, wn = _run(_op(), e.logits, 1, "sigmoid", True, 1.0, None)
    assert bool((ids == 0).all())
    EC.check_sigmoid_renormalized(w, wn)


@pytest.mark.parametrize("dtype", EC.SWEEP_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_every_16_bit_logit_through_softmax(dtype):
    s = EC.softmax_sweep(dtype)
    ids, w = _run(_op(), s.logits, 2, "softmax", False, 1.0, None)
    cids, cw = _run(_composition, s.logits, 2, "softmax", False, 1.0, None)
    err = EC.check_softmax_sweep(s, ids, w)
    _within(f"65536 {dtype} patterns, softmax over [l, 0]", err, EC.weight_err(cw, s.p.gather(-1, cids.long()), strict=False))


def test_every_fp16_logit_at_every_place():
    logits = EC.placement_logits()
    ids, w = _run(_op(), logits, 1, "sigmoid", False, 1.0, None)
    cids, cw = _run(_composition, logits, 1, "sigmoid", False, 1.0, None)
    err = EC.check_placement(ids, w)
    _within("65536 fp16 patterns as 64 x 1024, sigmoid, top-1", err, EC.check_placement(cids, cw))


# ------------------------------------------------------------------------------------------ 2f: a long batch
def test_a_long_batch_repeats_its_37_rows():
    e = EC.long_batch_edge()
    _check_ids(e)
    ids, w = _result(e.name)[:2]
    base = C.build(EC.long_batch_base())
    bids, bw = _run(_op(), base.logits, e.S, e.scoring, e.renormalize, e.scale, base.bias)
    rows = torch.arange(EC.LONG_T) % 37
    assert torch.equal(ids, bids[rows]) and torch.equal(w.view(torch.int32), bw.view(torch.int32)[rows])


# ------------------------------------------------------------------------------------------ 2g: the Python entry
def test_python_entry_takes_views_and_leading_dimensions():
    moe_topk = _bnb().moe_topk
    E, S = 160, 8
    gen = torch.Generator().manual_seed(160)
    wide = torch.randn(6, E + 11, generator=gen).bfloat16().to(DEV)
    parent = wide.clone()
    view = wide[:, 3:3 + E]
    assert not view.is_contiguous()
    sb = ((torch.arange(E) % 5 - 2) / 4).float().to(DEV)
    want = _op()(view.contiguous().view(-1, E), S, "sigmoid", True, 2.5, sb)
    with C.CountedEntry() as entry:
        got = moe_topk(view, S, "sigmoid", True, 2.5, sb)
        batch = moe_topk(view.reshape(2, 3, E), S, "sigmoid", True, 2.5, sb)
        strided_batch = moe_topk(wide.view(2, 3, E + 11)[..., 3:3 + E], S, "sigmoid", True, 2.5, sb)
    assert entry.calls == 3
    assert torch.equal(wide, parent)
    assert got[0].shape == got[1].shape == (6, S) and torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    for ids, w in (batch, strided_batch):
        assert ids.shape == w.shape == (2, 3, S) and ids.is_contiguous() and w.is_contiguous()
        assert torch.equal(ids.view(6, S), want[0]) and torch.equal(w.view(6, S).view(torch.int32), want[1].view(torch.int32))
    assert len({tuple(r) for r in got[0].tolist()}) > 1 and got[0].dtype == torch.int32   # (the rows differ: a row read at the parent's stride would show)


def test_python_entry_casts_a_16_bit_bias():
    """A bf16 select_bias is cast to fp32 (exactly) and the same launch runs: the bits of the call with the fp32 copy."""
    moe_topk = _bnb().moe_topk
    case = next(c for c in C.CASES if c.E == 256 and c.bias)
    b = C.build(case)
    logits, bias16 = b.logits.to(DEV), b.bias.to(DEV).bfloat16()
    assert torch.equal(bias16.float().cpu(), b.bias)
    want = moe_topk(logits, case.S, case.scoring, case.renormalize, case.scale, bias16.float())
    with C.CountedEntry() as entry:
        got = moe_topk(logits, case.S, case.scoring, case.renormalize, case.scale, bias16)
    assert entry.calls == 1 and bias16.dtype == torch.bfloat16
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(got[0].cpu(), b.ids)


def test_python_entry_composes_past_the_launch():
    """E = 1025, top_k = 17: no kernel, so the public function composes on the GPU - the float64 ranking - and the C entry is not
    called; the op itself raises."""
    e = EC.beyond_range_edge()
    logits, bias = e.logits.to(DEV), e.bias.to(DEV)
    with C.CountedEntry() as entry:
        ids, w = _bnb().moe_topk(logits, e.S, e.scoring, e.renormalize, e.scale, bias)
    assert entry.calls == 0
    assert ids.is_cuda and ids.dtype == torch.int32 and w.dtype == torch.float32 and torch.equal(ids.cpu(), e.ids)
    assert EC.weight_err(w, e.weights) <= C.WEIGHT_FLOOR
    with pytest.raises(ValueError, match="no kernel"):
        _op()(logits, e.S, e.scoring, e.renormalize, e.scale, bias)
