"""Cases, inputs and the float64 reference shared by tests/test_moe_route_grouped_host.py (CPU) and tests/test_gpu_moe_route_grouped.py
(GPU): group-limited MoE routing (``bitsandbytes_amd::moe_topk_grouped``, csrc/moe_route.hip; ``moe_topk_grouped`` /
``moe_route_grouped``).

The rules (one definition for kernel, composition and :func:`reference`): G = E / n_group, group g = experts [g G, (g + 1) G);
  1. p = softmax / sigmoid of the logits, key c = p (+ select_bias);
  2. a group's score: its first key in the order "larger key, then lower index, NaN keys last by index" (``"max"``), or first + second
     key (``"top2sum"``);
  3. the topk_group groups first in the same order on (score, group index) stay;
  4. top_k rounds of the selection over the experts of those groups only;
  5. weights = p[ids], divided by their sum in slot order if renormalize (no epsilon), times scale.

Grid: geometry (E, n_group, topk_group, S) x T x logits dtype x scoring x group_score x renormalize x select_bias, thinned PAIRWISE
as in tests/moe_route_cases.py; G = 1 goes with ``"max"`` only.

Rankings are unambiguous BY CONSTRUCTION (asserted in float64 for every row by :func:`assert_unambiguous`; no row is dropped or
redrawn). Logits are multiples of 1/8 in [-4, 4]. Per case, the groups have fixed roles at random places:
  * STARS "lone star" groups: ONE expert at 4.0, the largest key of the row. Under ``"max"`` such a group goes first; under
    ``"top2sum"`` its score p(4) + p(background) is below that of every high group - and the ungrouped top-k takes its star.
  * up to max(8, topk_group + 2) "high" groups: a first expert on one of the levels 3.75, 3.625, 3.5 and a second one 0 or 1/8 below it
    (G = 1: the first only) - six score classes for more groups than that: planted group ties. In row 0 every high group is
    (3.75, 3.75), so that the cut at topk_group falls inside a tie (the number of stars is chosen so that it does, see :func:`layout`).
  * every other expert sits on the row's one background level in [-4, -2].
Two different score classes differ in one operand by one level at least: sigmoid'(3.75) / 8 = 2.8e-3; softmax: the sums of e^l are
85.0, 80.0, 75.0, 70.6, 66.2, 62.3 and 54.7 for a star, over Z < 1600: more than 2e-3 apart. Keys are the levels themselves:
KEY_GAP of tests/moe_route_cases.py holds as it does there.
select_bias (multiples of 1/4, here -1, 0, +1) never lets two different operand pairs sum to the same score: -1 demotes single
experts (the first expert of one high group, and E / 16 background experts), and +1 promotes min(2, G, S - 1) background experts of
ONE otherwise plain group - part of a group, fewer than S, so the promoted group does not take every slot. Groups whose (logit, bias)
operands differ then differ by about 1 or by a level step. GROUP_GAP = 1e-4: a group score is below 4 in magnitude, a few fp32 ulps
there are about 2e-6, which leaves a factor of 50; it is not KEY_GAP because a softmax row of many experts brings two score classes
within 1e-3 of each other.

What the construction promises per case (:func:`build` asserts it): with topk_group < n_group, one row at least whose cut at
topk_group falls between two groups of identical operands (the lower group index wins), and one row at least whose ids differ from
the UNGROUPED ranking of tests/moe_route_cases.py on the same inputs - a kernel that ignored the groups would not pass. The one
exception is mathematical: under ``"max"`` with top_k <= topk_group the two rankings coincide for every input (the top_k experts lie
in at most top_k groups, each of which is then among the first top_k groups, ties included: groups are contiguous, so the lower
index wins at both levels alike); :func:`build` asserts that equality there instead."""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple, Optional

import numpy as np
import torch

import moe_route_cases as C

GEOMETRIES = ((8, 4, 2, 2), (60, 6, 2, 4), (64, 8, 3, 6), (64, 64, 16, 16), (72, 2, 1, 8), (128, 64, 16, 16), (160, 8, 3, 6),
              (256, 8, 4, 8), (384, 1, 1, 8), (512, 32, 8, 16), (1024, 16, 4, 16))   # (E, n_group, topk_group, S)
TS = (1, 3, 37)
DTYPES = C.DTYPES
SCORINGS = C.SCORINGS
GROUP_SCORES = ("max", "top2sum")
GROUP_GAP = 1e-4
HIGH_LEVELS = (3.75, 3.625, 3.5)
MAX_EXPERTS, MAX_TOP_K, MAX_GROUPS = 1024, 16, 64


class GroupedCase(NamedTuple):
    geometry: tuple
    T: int
    dtype: torch.dtype
    scoring: str
    group_score: str
    renormalize: bool
    bias: bool

    @property
    def E(self) -> int:
        return self.geometry[0]

    @property
    def n_group(self) -> int:
        return self.geometry[1]

    @property
    def topk_group(self) -> int:
        return self.geometry[2]

    @property
    def S(self) -> int:
        return self.geometry[3]

    @property
    def G(self) -> int:
        return self.E // self.n_group

    @property
    def scale(self) -> float:
        return 2.5 if (self.scoring == "sigmoid" and self.renormalize) else 1.0   # (DeepSeek-V3's routed_scaling_factor)

    @property
    def seed(self) -> int:
        return 1000 * self.E + 10 * self.n_group + self.T

    @property
    def name(self) -> str:
        return (f"E{self.E}-g{self.n_group}-k{self.topk_group}-S{self.S}-T{self.T}-{str(self.dtype).replace('torch.', '')}-{self.scoring}-"
                f"{self.group_score}-{'renorm' if self.renormalize else 'raw'}-{'bias' if self.bias else 'nobias'}")


AXES = (GEOMETRIES, TS, DTYPES, SCORINGS, GROUP_SCORES, (True, False), (False, True))


def valid(combo) -> bool:
    E, n_group = combo[0][0], combo[0][1]
    return combo[4] == "max" or E // n_group >= 2


def all_pairs():
    out = set()
    for combo in itertools.product(*AXES):
        if valid(combo):
            for a, b in itertools.combinations(range(len(AXES)), 2):
                out.add((a, combo[a], b, combo[b]))
    return out


def pairwise():
    """A greedy pairwise cover in a fixed order (a pure function of AXES): every value pair of every two axes that a valid combination
    can hold occurs in one case at least."""
    axis_pairs = tuple(itertools.combinations(range(len(AXES)), 2))
    pairs_of = {c: frozenset((a, c[a], b, c[b]) for a, b in axis_pairs) for c in itertools.product(*AXES) if valid(c)}
    todo = set().union(*pairs_of.values())
    chosen = []
    while todo:
        best = max(pairs_of, key=lambda c: len(pairs_of[c] & todo))   # (the first of equals: dicts keep insertion order)
        chosen.append(best)
        todo -= pairs_of[best]
    return tuple(GroupedCase(*c) for c in chosen)


CASES = pairwise()


# ------------------------------------------------------------------------------------------ inputs
class Layout(NamedTuple):
    stars: tuple        # (group, place in the group)
    highs: tuple        # (group, (place of the first expert, place of the second one or None))
    promoted: tuple     # the experts with select_bias +1
    demoted: tuple      # the experts with select_bias -1


def layout(case: GroupedCase) -> Layout:
    """The roles of the groups of a case (n_group >= 2). A +1 bias puts one plain group in front of every other, so the groups with
    roles compete for k = topk_group - 1 places then. Row 0 has every high group in one score class, and the cut must fall inside a
    tie in both group_score modes: under "max" the stars lead (cut inside the stars for k < stars, inside the high groups for
    k > stars: never k == stars), under "top2sum" the high groups lead (cut inside them, or, where they are fewer than k, inside the
    stars)."""
    E, n_group, topk_group, S = case.geometry
    G = case.G
    rng = np.random.RandomState(case.seed + 1)
    promote = case.bias and n_group >= 6 and topk_group >= 2
    k = topk_group - (1 if promote else 0)
    n_stars = min(3 if k == 2 else 2, n_group - (1 if promote else 0))
    n_highs = max(0, min(n_group - n_stars - (1 if promote else 0), max(8, topk_group + 2)))
    roles = rng.permutation(n_group)
    stars = tuple((int(g), int(rng.randint(G))) for g in roles[:n_stars])
    highs = []
    for g in roles[n_stars:n_stars + n_highs]:
        places = rng.permutation(G)[:2]
        highs.append((int(g), (int(places[0]), int(places[1]) if G >= 2 else None)))
    promoted, demoted = [], []
    if case.bias:
        taken = {g * G + pl for g, pl in stars} | {g * G + pl for g, pls in highs for pl in pls if pl is not None}
        if promote:
            g = int(roles[n_stars + n_highs])
            promoted = [g * G + int(pl) for pl in rng.permutation(G)[:min(2, G, S - 1)]]
        if n_highs >= 2:
            demoted.append(highs[-1][0] * G + highs[-1][1][0])
        plain = [j for j in rng.permutation(E) if j not in taken and j not in promoted]
        demoted += [int(j) for j in plain[:max(1, E // 16)]]
    return Layout(stars, tuple(highs), tuple(promoted), tuple(demoted))


def build_logits(case: GroupedCase) -> torch.Tensor:
    """[T, E] float64, multiples of 1/8 in [-4, 4]: the construction of the file head (n_group == 1: that of tests/moe_route_cases.py)."""
    if case.n_group == 1:
        return C.build_logits(case.E, case.T, case.seed)
    lay, G = layout(case), case.G
    rng = np.random.RandomState(case.seed)
    out = np.empty((case.T, case.E), dtype=np.float64)
    for t in range(case.T):
        out[t, :] = -4.0 + rng.randint(0, 17) / 8.0
        for g, place in lay.stars:
            out[t, g * G + place] = 4.0
        for g, (first, second) in lay.highs:
            level = HIGH_LEVELS[0] if t == 0 else HIGH_LEVELS[rng.randint(len(HIGH_LEVELS))]
            step = 0.0 if t == 0 else rng.randint(2) / 8.0
            out[t, g * G + first] = level
            if second is not None:
                out[t, g * G + second] = level - step
    return torch.from_numpy(out)


def build_bias(case: GroupedCase) -> torch.Tensor:
    """[E] float32: +1 on the promoted experts, -1 on the demoted ones (n_group == 1: the bias of tests/moe_route_cases.py)."""
    if case.n_group == 1:
        return C.build_bias(case.E, case.S, case.seed)
    lay = layout(case)
    out = np.zeros(case.E, dtype=np.float32)
    out[list(lay.promoted)] = 1.0
    out[list(lay.demoted)] = -1.0
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------ the float64 reference
def _order(keys: np.ndarray) -> np.ndarray:
    """The indices of `keys` in the order of the selection: larger key first, lower index on ties, NaN keys last by index."""
    nan = np.isnan(keys)
    return np.lexsort((np.arange(keys.size), -np.where(nan, -np.inf, keys), nan))


def group_scores(key_row: np.ndarray, n_group: int, group_score: str) -> np.ndarray:
    with np.errstate(invalid="ignore"):   # (inf + -inf is NaN, as in the kernel)
        by_group = key_row.reshape(n_group, -1)
        out = np.empty(n_group, dtype=np.float64)
        for g in range(n_group):
            first = _order(by_group[g])[:2]
            out[g] = by_group[g][first[0]] + by_group[g][first[1]] if group_score == "top2sum" else by_group[g][first[0]]
    return out


def reference(logits: torch.Tensor, S: int, n_group: int, topk_group: int, group_score: str, scoring: str, renormalize: bool, scale: float,
              bias: Optional[torch.Tensor]):
    """float64: (ids int32 [T, S], weights float64 [T, S], kept bool [T, n_group]) by the five rules of the file head."""
    p = C.scores64(logits, scoring)
    key = (p if bias is None else p + bias.double()).numpy()
    G = key.shape[-1] // n_group
    ids, kept = [], []
    for row in key:
        stay = np.zeros(n_group, dtype=bool)
        stay[_order(group_scores(row, n_group, group_score))[:topk_group]] = True
        ranked = _order(row)
        ids.append(ranked[stay[ranked // G]][:S])
        kept.append(stay)
    ids = torch.from_numpy(np.stack(ids))
    w = p.gather(-1, ids)
    if renormalize:
        total = w[:, 0].clone()
        for s in range(1, S):
            total = total + w[:, s]
        w = w / total.unsqueeze(-1)
    return ids.to(torch.int32), w * scale, torch.from_numpy(np.stack(kept))


def assert_unambiguous(logits: torch.Tensor, n_group: int, topk_group: int, group_score: str, scoring: str, bias: Optional[torch.Tensor]):
    """Every row, in float64: two KEYS come from identical (logit, bias) pairs or differ by more than KEY_GAP (every key of the row,
    kept groups or not); two GROUP SCORES come from identical (logit, bias) operands or differ by more than GROUP_GAP. Returns
    (smallest gap between two different group scores, the rows whose cut at topk_group falls between two groups of identical operands)."""
    C.assert_unambiguous(logits, scoring, bias)
    l = logits.double().numpy()
    b = np.zeros(l.shape[-1]) if bias is None else bias.double().numpy()
    key = C.scores64(logits, scoring).numpy() + b
    take = 2 if group_score == "top2sum" else 1
    smallest, tied_cuts = float("inf"), []
    for t in range(l.shape[0]):
        score = group_scores(key[t], n_group, group_score)
        assert bool(np.isfinite(score).all()) and float(np.abs(score).max()) < 4.0
        operands = []
        for g in range(n_group):
            sl = slice(g * (l.shape[-1] // n_group), (g + 1) * (l.shape[-1] // n_group))
            first = _order(key[t][sl])[:take]
            operands.append(tuple(sorted((float(l[t][sl][i]), float(b[sl][i])) for i in first)))
        ranked = _order(score)
        for a, c in zip(ranked[:-1], ranked[1:]):
            gap = score[a] - score[c]
            if operands[a] == operands[c]:
                assert gap == 0
            else:
                assert gap > GROUP_GAP, f"row {t}: groups {a} and {c} of different operands are within {GROUP_GAP}: {gap}"
                smallest = min(smallest, float(gap))
        if topk_group < n_group and operands[ranked[topk_group - 1]] == operands[ranked[topk_group]]:
            tied_cuts.append(t)
    return smallest, tied_cuts


def coincides_with_ungrouped(case: GroupedCase) -> bool:
    """Whether the grouped and the ungrouped ranking are the same for EVERY input (file head): no group is dropped, or "max" with
    top_k <= topk_group."""
    return case.topk_group == case.n_group or (case.group_score == "max" and case.S <= case.topk_group)


class Built(NamedTuple):
    logits: torch.Tensor            # [T, E] in the case's dtype (exact)
    bias: Optional[torch.Tensor]    # [E] float32 or None
    ids: torch.Tensor               # the float64 ranking
    weights: torch.Tensor           # float64
    kept: torch.Tensor              # [T, n_group] bool: the groups that stay
    gap: float                      # the smallest gap between two different group scores
    differs: tuple                  # the rows whose ids are not the ungrouped ranking's


@functools.lru_cache(maxsize=None)
def build(case: GroupedCase) -> Built:
    l64 = build_logits(case)
    bias = build_bias(case) if case.bias else None
    logits = l64.to(case.dtype)
    assert torch.equal(logits.double(), l64)
    gap, tied_cuts = assert_unambiguous(logits, case.n_group, case.topk_group, case.group_score, case.scoring, bias)
    ids, w, kept = reference(logits, case.S, case.n_group, case.topk_group, case.group_score, case.scoring, case.renormalize, case.scale, bias)
    plain_ids, _ = C.reference(logits, case.S, case.scoring, case.renormalize, case.scale, bias)
    differs = tuple(int(t) for t in (ids != plain_ids).any(-1).nonzero().flatten())
    if case.topk_group < case.n_group:
        assert tied_cuts, f"{case.name}: no row cuts the groups inside a tie"
    if coincides_with_ungrouped(case):
        assert not differs
    else:
        assert differs, f"{case.name}: every row has the ids of the ungrouped ranking"
    return Built(logits, bias, ids, w, kept, gap, differs)


class CountedEntry:
    """Counts the calls of bnb_mi355x_moe_topk_grouped (and of bnb_mi355x_moe_topk: ``plain``) that the Python layer makes."""

    def __enter__(self):
        from bitsandbytes_amd.backends import hip

        self.hip, self.real, self.calls, self.plain = hip, hip.lib, 0, 0
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(outer.real, name)
                if name not in ("bnb_mi355x_moe_topk_grouped", "bnb_mi355x_moe_topk"):
                    return fn

                def counted(*args):
                    if name == "bnb_mi355x_moe_topk":
                        outer.plain += 1
                    else:
                        outer.calls += 1
                    return fn(*args)

                return counted

        hip.lib = Proxy()
        return self

    def __exit__(self, *exc):
        self.hip.lib = self.real
        return False
