"""Structured inputs for the MoE router's scoring + top-k launch (``bitsandbytes_amd::moe_topk``, csrc/moe_route.hip), shared by
tests/test_moe_route_edges_host.py (CPU: the preconditions, and the fp32 torch composition against float64) and
tests/test_gpu_moe_route_edges.py (GPU: the kernel). tests/moe_route_cases.py draws ordinary rows at random; what a random row does
not reach is built here on purpose. Every builder returns :class:`Edge` objects: the logits, the optional selection bias and the
float64 :func:`moe_route_cases.reference` result.

  positions  a winner at every (lane, slot): row t has 4.0 at t, 3.875 at the next slot of the same lane and 3.75 on the next lane
  one_lane   one lane supplies all S = NI winners, in an order permuted per row (the winner leaves, the lane offers its next best)
  ties       rows that are one tie (ids 0 ... S-1; softmax weights with the bits of 1.0f / E), and a tie that only the bias breaks
  masks      -inf logits on all but m experts; NaN logits; +inf logits; -inf / +inf / NaN selection biases; logits of +-3e38
  sweeps     every 16-bit pattern as a logit: values, not ranking (E = 1 and E = 2), and once over all (lane, slot) places
  long batch 4099 rows: more workgroups than the chip holds at once, and a last workgroup with three idle wavefronts

Unambiguity. `positions` and `one_lane` use multiples of 1/8 in [-4, 4] and pass :func:`moe_route_cases.assert_unambiguous`. The
others hold non-finite keys: :func:`assert_classes_unambiguous` states what makes their float64 ranking the one right answer for an
fp32 implementation too - two neighbouring keys of the ranking are the same key for a reason that holds in either precision, or are
of different classes (finite / -inf / +inf / NaN), or differ by more than KEY_GAP.

Weights. ``err = |w - w64| / max(|w64|, 2^-100)`` (:func:`weight_err`): near 2^-126 an fp32 result legitimately has no relative
precision, and the floor keeps denormal and flushed results from dominating. Non-finite reference values are compared by class, and
a reference weight of exactly 0 (a masked expert; float64 underflows far below fp32) must be exactly 0."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

import moe_route_cases as C

ERR_FLOOR = 2.0 ** -100
INF, NAN = float("inf"), float("nan")


class Edge(NamedTuple):
    name: str
    logits: torch.Tensor            # [T, E]
    bias: Optional[torch.Tensor]    # [E] float32 or None
    S: int
    scoring: str
    renormalize: bool
    scale: float
    ids: torch.Tensor               # the float64 ranking, int32 [T, S]
    weights: torch.Tensor           # float64 [T, S]
    ordinary: bool                  # multiples of 1/8 in [-4, 4], finite bias: moe_route_cases.assert_unambiguous applies

    @property
    def E(self) -> int:
        return int(self.logits.shape[-1])


def _edge(name, logits, bias, S, scoring, renormalize=False, scale=1.0, ordinary=False) -> Edge:
    ids, w = C.reference(logits, S, scoring, renormalize, scale, bias)
    return Edge(name, logits, bias, S, scoring, renormalize, scale, ids, w, ordinary)


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


# ------------------------------------------------------------------------------------------ the error metric
def weight_err(w: torch.Tensor, w64: torch.Tensor, strict: bool = True) -> float:
    """max |w - w64| / max(|w64|, 2^-100) over the finite reference values. strict: NaN exactly where the reference has NaN, the same
    infinity, exactly 0 where the reference is exactly 0. Not strict (a figure only): positions where both are finite."""
    w = w.double().cpu()
    assert w.shape == w64.shape
    fin = torch.isfinite(w64)
    if strict:
        assert torch.equal(torch.isnan(w), torch.isnan(w64)), "NaN weights are not where the reference has them"
        assert torch.equal(w[torch.isinf(w64)], w64[torch.isinf(w64)]) and bool(torch.isfinite(w[fin]).all())
        assert bool((w[w64 == 0] == 0).all()), "a weight whose reference is exactly 0 is not 0"
    else:
        fin = fin & torch.isfinite(w)
    if not bool(fin.any()):
        return 0.0
    return float(((w[fin] - w64[fin]).abs() / w64[fin].abs().clamp_min(ERR_FLOOR)).max())


def assert_classes_unambiguous(edge: Edge) -> float:
    """Walks every row's whole float64 ranking. Two neighbours are fine when they are both NaN; when they are equal and come from
    identical (logit, bias) pairs, or are equal infinities, or are softmax scores that are exactly 0 because both logits lie more
    than 800 below the row's maximum (0 in float64 and, from 104 on, in fp32); when one of them is not finite (classes do not
    depend on the precision); or when they differ by more than KEY_GAP. Returns the smallest gap between two finite keys."""
    l = edge.logits.double()
    E = edge.E
    b = torch.zeros(E, dtype=torch.float64) if edge.bias is None else edge.bias.double()
    key = C.scores64(l, edge.scoring) + b
    order, _ = C.reference(edge.logits, E, edge.scoring, False, 1.0, edge.bias)
    smallest = INF
    for t in range(l.shape[0]):
        o = order[t].long()
        assert sorted(o.tolist()) == list(range(E))
        k, lo, bo = key[t][o], l[t][o], b[o]
        a, z = slice(0, E - 1), slice(1, E)
        both_nan = torch.isnan(k[a]) & torch.isnan(k[z])
        same_pair = ((lo[a] == lo[z]) | (torch.isnan(lo[a]) & torch.isnan(lo[z]))) & ((bo[a] == bo[z]) | (torch.isnan(bo[a]) & torch.isnan(bo[z])))
        equal = k[a] == k[z]
        deep = (lo[a] < l[t].max() - 800) & (lo[z] < l[t].max() - 800) if edge.scoring == "softmax" and edge.bias is None else torch.zeros_like(equal)
        fine_equal = equal & (same_pair | torch.isinf(k[a]) | deep)
        one_not_finite = ~equal & ~both_nan & (~torch.isfinite(k[a]) | ~torch.isfinite(k[z]))
        gap = k[a] - k[z]
        apart = torch.isfinite(gap) & (gap > C.KEY_GAP)
        assert bool((both_nan | fine_equal | one_not_finite | apart).all()), f"{edge.name}: row {t} has two keys that fp32 could order differently"
        if bool(apart.any()):
            smallest = min(smallest, float(gap[apart].min()))
    return smallest


# ------------------------------------------------------------------------------------------ 2a: every (lane, slot) position
POSITION_ES = (64, 128, 256, 512, 1024)


@functools.lru_cache(maxsize=None)
def position_edge(E: int, scoring: str, dtype: torch.dtype) -> Edge:
    """T = E rows; row t: background -4, 4.0 at t, 3.875 at (t + 64) % E - the same lane, the next slot; E = 64 has one slot, there
    (t + 2) % E - and 3.75 at (t + 1) % E. S = 3: the ids are those three positions in that order."""
    t = torch.arange(E)
    l = torch.full((E, E), -4.0, dtype=torch.float64)
    second = (t + 64) % E if E > 64 else (t + 2) % E
    l[t, t], l[t, second], l[t, (t + 1) % E] = 4.0, 3.875, 3.75
    edge = _edge(f"pos-E{E}-{scoring}-{_dt(dtype)}", l.to(dtype), None, 3, scoring, ordinary=True)
    assert torch.equal(edge.ids.long(), torch.stack([t, second, (t + 1) % E], dim=-1))
    return edge


def position_edges():
    return [position_edge(E, sc, dt) for E in POSITION_ES for sc in C.SCORINGS for dt in (torch.float32, torch.bfloat16)]


# ------------------------------------------------------------------------------------------ 2b: one lane supplies every winner
ONE_LANE = ((128, 2), (256, 4), (512, 8), (1024, 16))


@functools.lru_cache(maxsize=None)
def one_lane_edge(E: int, NI: int, scoring: str, renormalize: bool) -> Edge:
    """T = 64 rows; row `lane`: background -4 and the levels 4 - k / 8, k < NI, on the experts lane + 64 i, in an order permuted per
    row. S = NI: all winners of a row sit in one lane, which hands them out one after the other."""
    assert C.lane_slots(E) == NI and E == 64 * NI
    rng = np.random.RandomState(100 * NI + 1)
    l = torch.full((64, E), -4.0, dtype=torch.float64)
    want = torch.empty((64, NI), dtype=torch.int64)
    for lane in range(64):
        slots = rng.permutation(NI)             # slots[k]: the slot that holds level k
        for k in range(NI):
            l[lane, lane + 64 * int(slots[k])] = 4.0 - k / 8.0
        want[lane] = lane + 64 * torch.from_numpy(slots)
    edge = _edge(f"lane-E{E}-{scoring}-{'renorm' if renormalize else 'raw'}", l.to(torch.float16), None, NI, scoring, renormalize, ordinary=True)
    assert torch.equal(edge.ids.long(), want)
    return edge


def one_lane_edges():
    return [one_lane_edge(E, NI, sc, rn) for E, NI in ONE_LANE for sc in C.SCORINGS for rn in (True, False)]


# ------------------------------------------------------------------------------------------ 2c: whole-row ties
TIE_LEVELS = (-4.0, 0.0, 4.0)
BIAS_TIE = (63, 64, 65)


@functools.lru_cache(maxsize=None)
def tie_edge(E: int, scoring: str, with_bias: bool) -> Edge:
    """Three rows, every logit of a row equal (-4, 0, 4), S = min(E, 16), raw weights: ids 0 ... S-1. with_bias: select_bias is +1 on
    the experts 63, 64 and 65 (the last lane's first slot, the first two lanes' second one): they lead, then 0, 1, ...; the weights
    are the unbiased scores."""
    S = min(E, 16)
    dtype = C.DTYPES[C.ES.index(E) % 3]
    l = torch.tensor(TIE_LEVELS, dtype=torch.float64).view(3, 1).expand(3, E).contiguous()
    bias = None
    want = list(range(S))
    if with_bias:
        assert E > max(BIAS_TIE)
        bias = torch.zeros(E, dtype=torch.float32)
        bias[list(BIAS_TIE)] = 1.0
        want = (list(BIAS_TIE) + list(range(S)))[:S]
    edge = _edge(f"tie-E{E}-{scoring}-{'bias' if with_bias else 'nobias'}-{_dt(dtype)}", l.to(dtype), bias, S, scoring)
    assert edge.ids.tolist() == [want] * 3
    return edge


def tie_edges():
    return [tie_edge(E, sc, wb) for E in sorted(C.ES) for sc in C.SCORINGS for wb in (False, True) if not wb or E > max(BIAS_TIE)]


def tie_softmax_bits(E: int) -> int:
    """The bits of float32(1) / float32(E): expf(0) = 1, a sum of E ones is exact, IEEE division."""
    return int((np.float32(1.0) / np.float32(E)).view(np.int32))


# ------------------------------------------------------------------------------------------ 2d: masks and non-finite keys
MASK_ES = (72, 256)
MASK_S = 8
MASK_LIVE = (MASK_S + 3, MASK_S, MASK_S - 2, 1, 0)


def _levels_at(E: int, T: int, count: int, seed: int, fill: float) -> torch.Tensor:
    """[T, E] float64: `fill` everywhere but at `count` random places per row, which hold 4, 3.875, ... in a random order."""
    rng = np.random.RandomState(seed)
    l = torch.full((T, E), fill, dtype=torch.float64)
    for t in range(T):
        at = rng.permutation(E)[:count]
        l[t, torch.from_numpy(at)] = 4.0 - torch.arange(count, dtype=torch.float64) / 8.0
    return l


@functools.lru_cache(maxsize=None)
def mask_edge(E: int, scoring: str, live: int, renormalize: bool = False) -> Edge:
    """-inf logits on all but `live` experts: the live ones first, by score, then masked ones by index with weight exactly 0. No live
    expert: softmax is NaN (-inf - -inf), sigmoid is a row of zeros - and NaN from 0 / 0 once renormalized."""
    dtype = torch.float16 if E == 72 else torch.bfloat16
    l = _levels_at(E, 4, live, 7000 + 10 * E + live, -INF)
    return _edge(f"mask-E{E}-live{live}-{scoring}-{'renorm' if renormalize else 'raw'}", l.to(dtype), None, MASK_S, scoring, renormalize)


@functools.lru_cache(maxsize=None)
def nan_logit_edge(E: int, scoring: str) -> Edge:
    """NaN logits on all but 12 experts, S = 16. Sigmoid: the 12 finite ones, then the four NaN experts of lowest index with NaN
    weights. Softmax: one NaN makes the row NaN: 0 ... 15."""
    dtype = torch.float32 if E == 72 else torch.float16
    return _edge(f"nanlogit-E{E}-{scoring}", _levels_at(E, 3, 12, 7100 + E, NAN).to(dtype), None, 16, scoring)


INF_AT = ((1, 70), (3, 0))   # (row, expert): the second slot of lane 6; the first expert of the last row


@functools.lru_cache(maxsize=None)
def inf_logit_edge(E: int, scoring: str) -> Edge:
    """Ordinary rows; rows 1 and 3 hold one +inf logit. Sigmoid: its score is exactly 1 and it leads. Softmax: the row is NaN."""
    l = C.build_logits(E, 4, 7200 + E)
    for row, col in INF_AT:
        l[row, col] = INF
    return _edge(f"inflogit-E{E}-{scoring}", l.to(torch.bfloat16), None, MASK_S, scoring)


class BiasRows(NamedTuple):
    logits: torch.Tensor   # [4, E] float64
    best: tuple            # the three experts that hold 4, 3.875, 3.75 (rotated per row; best[0] leads row 0)
    good: tuple            # nine experts below them: 3.625 ... 2.625, rotated per row
    background: tuple      # two experts of the background, ascending


@functools.lru_cache(maxsize=None)
def bias_rows(E: int) -> BiasRows:
    rng = np.random.RandomState(7300 + E)
    at = [int(i) for i in rng.permutation(E)[:14]]
    best, good, background = tuple(at[:3]), tuple(at[3:12]), tuple(sorted(at[12:]))
    l = torch.empty((4, E), dtype=torch.float64)
    for r in range(4):
        l[r, :] = -4.0 + r / 8.0
        for k in range(3):
            l[r, best[(k + r) % 3]] = 4.0 - k / 8.0
        for k in range(9):
            l[r, good[(k + r) % 9]] = 3.625 - k / 8.0
    return BiasRows(l, best, good, background)


BIAS_KINDS = ("neginf-best3", "posinf-background2", "nan-best", "neginf-all-but5")


@functools.lru_cache(maxsize=None)
def bias_edge(E: int, scoring: str, kind: str) -> Edge:
    """Non-finite selection biases; the weights stay the finite unbiased scores.
      neginf-best3        -inf on the three best experts: they fall behind every finite key (the ids are the next eight)
      posinf-background2  +inf on two background experts: they lead, the lower index first
      nan-best            NaN on row 0's best expert: ranked last
      neginf-all-but5     -inf on all but five experts, the usual way to mask by bias: the five, then -inf keys by ascending index"""
    rows = bias_rows(E)
    bias = torch.zeros(E, dtype=torch.float32)
    if kind == "neginf-best3":
        bias[list(rows.best)] = -INF
    elif kind == "posinf-background2":
        bias[list(rows.background)] = INF
    elif kind == "nan-best":
        bias[rows.best[0]] = NAN
    else:
        bias[:] = -INF
        bias[list(rows.good[:5])] = 0.0
    edge = _edge(f"bias-E{E}-{kind}-{scoring}", rows.logits.to(torch.float32 if E == 72 else torch.bfloat16), bias, MASK_S, scoring)
    got = edge.ids.tolist()
    if kind == "neginf-best3":
        assert all(set(r) <= set(rows.good) for r in got)
    elif kind == "posinf-background2":
        assert all(tuple(r[:2]) == rows.background for r in got)
    elif kind == "nan-best":
        assert all(rows.best[0] not in r for r in got)
    else:
        masked = [j for j in range(E) if j not in rows.good[:5]][:3]
        assert all(set(r[:5]) == set(rows.good[:5]) and r[5:] == masked for r in got)
    assert bool(torch.isfinite(edge.weights).all())
    return edge


@functools.lru_cache(maxsize=None)
def nan_bias_last_edge(scoring: str) -> Edge:
    """E = S = 16, sixteen different levels, NaN bias on the best expert of row 0: the whole ranking is returned, and it ends with it."""
    l = _levels_at(16, 3, 16, 7400, 0.0)
    best = int(l[0].argmax())
    bias = torch.zeros(16, dtype=torch.float32)
    bias[best] = NAN
    edge = _edge(f"bias-E16-nan-last-{scoring}", l.to(torch.float16), bias, 16, scoring)
    assert all(r[-1] == best for r in edge.ids.tolist())
    return edge


@functools.lru_cache(maxsize=None)
def huge_logit_edge() -> Edge:
    """fp32 [3e38, -3e38, 3e38, 0, -3e38 ...]: l - max overflows to -inf, expf gives 0: ids 0, 2, 1, 3 with the weights 0.5, 0.5, 0, 0."""
    l = torch.full((1, 72), -3e38, dtype=torch.float32)
    l[0, :4] = torch.tensor([3e38, -3e38, 3e38, 0.0])
    edge = _edge("huge-E72-softmax", l, None, 4, "softmax")
    assert edge.ids.tolist() == [[0, 2, 1, 3]] and edge.weights.tolist() == [[0.5, 0.5, 0.0, 0.0]]
    return edge


def nonfinite_edges():
    out = []
    for E in MASK_ES:
        for sc in C.SCORINGS:
            out += [mask_edge(E, sc, m) for m in MASK_LIVE]
            out += [nan_logit_edge(E, sc), inf_logit_edge(E, sc)]
            out += [bias_edge(E, sc, kind) for kind in BIAS_KINDS]
        out.append(mask_edge(E, "sigmoid", 0, True))
    out += [nan_bias_last_edge(sc) for sc in C.SCORINGS]
    out.append(huge_logit_edge())
    return out


# ------------------------------------------------------------------------------------------ 2e: every 16-bit logit value
SWEEP_DTYPES = (torch.float16, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def patterns(dtype: torch.dtype) -> torch.Tensor:
    """[65536]: element v has the bit pattern v."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dtype)


@functools.lru_cache(maxsize=None)
def sigmoid_sweep(dtype: torch.dtype, renormalize: bool = False) -> Edge:
    """T = 65536, E = 1, S = 1: id 0 and w = sigmoid64(l)."""
    return _edge(f"sweep-sigmoid-{_dt(dtype)}-{'renorm' if renormalize else 'raw'}", patterns(dtype).view(-1, 1).clone(), None, 1, "sigmoid", renormalize)


def check_sigmoid_renormalized(p: torch.Tensor, w: torch.Tensor) -> None:
    """p: the raw weights of an implementation, w: its renormalized ones on the same input. p / p: exactly 1 wherever 0 < p is finite
    (a denormal p included: IEEE division), NaN where p is 0 or NaN."""
    p, w = p.cpu(), w.cpu()
    one = (p > 0) & torch.isfinite(p)
    assert bool((w[one] == 1.0).all()), f"{int((w[one] != 1.0).sum())} rows with p > 0 do not renormalize to exactly 1"
    assert bool(torch.isnan(w[~one]).all())


class SoftmaxSweep(NamedTuple):
    logits: torch.Tensor    # [65536, 2]: row v is [pattern v, 0]
    p: torch.Tensor         # float64 softmax
    ids: torch.Tensor       # the float64 ranking (NaN rows: 0, 1)
    finite: torch.Tensor    # [65536] bool: the pattern is finite
    ranked: torch.Tensor    # [65536] bool: the order is asserted
    close: torch.Tensor     # [65536] bool: finite, not +-0, |p0 - p1| <= KEY_GAP in float64


@functools.lru_cache(maxsize=None)
def softmax_sweep(dtype: torch.dtype) -> SoftmaxSweep:
    """T = 65536, E = 2, S = 2, rows [l, 0]. The order of a row is asserted where float64 decides it by more than KEY_GAP, where l
    is +-0 (a tie: 0, 1), where l is not finite (-inf: 1, 0; NaN and +inf: a NaN row, 0, 1) - and for every l > 0: there
    e_0 = expf(l - l) = 1 >= e_1 = expf(-l) in any fp32 evaluation, and a tie goes to the lower index, so (0, 1) is the answer of
    fp32 and of float64 alike. What stays open is 0 > l >= -2e-3: float64 says (1, 0), fp32 says so only where expf(l) < 1."""
    l = patterns(dtype)
    logits = torch.stack([l, torch.zeros_like(l)], dim=-1)
    p = C.scores64(logits, "softmax")
    ids, _ = C.reference(logits, 2, "softmax", False, 1.0, None)
    finite = torch.isfinite(l)
    l64 = l.double()
    close = finite & (l64 != 0) & ((p[:, 0] - p[:, 1]).abs() <= C.KEY_GAP)
    ranked = ~close | (l64 > 0)
    return SoftmaxSweep(logits, p, ids, finite, ranked, close)


def check_softmax_sweep(sweep: SoftmaxSweep, ids: torch.Tensor, w: torch.Tensor) -> float:
    """The ids of a row are a permutation of {0, 1}; the weight reported for id j is softmax64(row)[j], whatever the order (returns
    the error, :func:`weight_err`); the order where it is asserted; and on every finite row the order agrees with the reported
    weights themselves: not increasing, and equal weights in ascending index."""
    ids, w = ids.cpu(), w.cpu()
    assert torch.equal(ids.sort(dim=-1).values, torch.tensor([0, 1], dtype=torch.int32).expand(65536, 2))
    err = weight_err(w, sweep.p.gather(-1, ids.long()))
    bad = (ids != sweep.ids).any(-1) & sweep.ranked
    assert not bool(bad.any()), f"{int(bad.sum())} rows in another order, the first at pattern {int(bad.nonzero()[0])}"
    f = sweep.finite
    assert bool((w[f, 0] >= w[f, 1]).all()) and bool((ids[f & (w[:, 0] == w[:, 1]), 0] == 0).all())
    return err


@functools.lru_cache(maxsize=None)
def placement_logits() -> torch.Tensor:
    """[64, 1024] fp16: the 65536 patterns once more, 1024 to a row: every value class at every (lane, slot) place."""
    return patterns(torch.float16).view(64, 1024).clone()


def check_placement(ids: torch.Tensor, w: torch.Tensor) -> float:
    """S = 1, sigmoid, raw: the winner's weight is the maximum of the float64 scores of its row (NaN scores apart), and the id is one
    whose float64 score is within KEY_GAP of that maximum. Returns the weight error."""
    p = C.scores64(placement_logits(), "sigmoid")
    best = torch.where(torch.isnan(p), torch.full_like(p, -INF), p).max(dim=-1, keepdim=True).values
    assert bool(torch.isfinite(best).all())
    got = p.gather(-1, ids.cpu().long())
    assert bool((got >= best - C.KEY_GAP).all()), "a winner that float64 puts more than KEY_GAP behind the best"
    return weight_err(w, best)


# ------------------------------------------------------------------------------------------ 2f: a long batch
LONG_T = 4099


def long_batch_base() -> C.RouteCase:
    base = [c for c in C.CASES if c.E == 8 and c.S == 2 and c.T == 37]
    assert len(base) == 1
    return base[0]


@functools.lru_cache(maxsize=None)
def long_batch_edge() -> Edge:
    """4099 rows of E = 8, S = 2: the 37 rows of a case of the ranked grid, repeated cyclically. 1025 workgroups - more than the chip
    holds at once - and the last one has a single live wavefront."""
    case = long_batch_base()
    b = C.build(case)
    rows = torch.arange(LONG_T) % case.T
    edge = _edge("long-T4099-E8", b.logits[rows].contiguous(), b.bias, case.S, case.scoring, case.renormalize, case.scale, ordinary=True)
    assert torch.equal(edge.ids, b.ids[rows]) and torch.equal(edge.weights, b.weights[rows])
    return edge


# ------------------------------------------------------------------------------------------ 2g: beyond the kernel's range
@functools.lru_cache(maxsize=None)
def beyond_range_edge() -> Edge:
    """E = 1025, top_k = 17: an ordinary input of the ranked grid's construction, one expert and one slot past the launch."""
    l = C.build_logits(1025, 5, 1025017)
    return _edge("beyond-E1025-S17", l.to(torch.bfloat16), C.build_bias(1025, 17, 1025017), 17, "sigmoid", True, 2.5, ordinary=True)


def structured_edges():
    """Everything that is compared as it stands: ids exactly, weights by :func:`weight_err`."""
    return position_edges() + one_lane_edges() + tie_edges() + nonfinite_edges() + [long_batch_edge(), beyond_range_edge()]
