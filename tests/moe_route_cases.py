"""Cases, inputs and the float64 reference shared by tests/test_moe_route_host.py (CPU) and tests/test_gpu_moe_route.py (GPU): the
router's scoring + top-k launch (``bitsandbytes_amd::moe_topk``, csrc/moe_route.hip) and the public ``moe_topk`` / ``moe_route``.

Grid: E x S x T x logits dtype x scoring x renormalize x select_bias, S <= E, thinned PAIRWISE (:func:`pairwise`): every value pair of
every two axes that can occur together occurs in at least one case. The cover of the first grid (FIRST_ES) leads unchanged; a cover of
the pairs that involve a later expert count (LATER_ES) follows it.

Rankings are unambiguous BY CONSTRUCTION, so that float64 is the one right answer for the ids and a float32 implementation has to
reproduce it exactly:
  * logits are multiples of 1/8 in [-4, 4] (exact in bf16, fp16 and fp32). A row has up to HI_COUNT "high" experts at random places,
    on the HI_LEVELS top levels 4, 3.875, ... (more experts than levels: planted ties), and one background level in [-4, -2] for all
    the others (one large tie). Softmax: Z <= 20 e^4 + 1004 e^-2 < 1230, the lowest high score is >= e^3.125 / 1230 = 0.0185, and two
    neighbouring levels differ by the factor e^(1/8): by more than 2e-3. Sigmoid: levels 1/8 apart differ by >= sigmoid'(4) / 8 = 2.2e-3.
  * select_bias values are multiples of 1/4 - here -1, 0 and +1: a score lies in (0, 1) and the scores of a row span less than
    0.999, so keys of different bias classes are more than 1e-3 apart, and the bias reorders the selection (a background expert with
    +1 goes before every high expert with 0) while the weights stay the unbiased scores.
:func:`assert_unambiguous` checks the outcome in float64 for every row: two keys come from identical (logit, bias) pairs or differ by
more than 1e-3. No row is dropped or redrawn.

Which inputs pin which rule. This grid pins the ids and the weights of ordinary rows in every template instance (E of FIRST_ES and
LATER_ES: NI = 1, 2, 4, 8, 16 at both edges of an instance, :func:`lane_slots`), with ties among the ~20 high experts at random
places. What a random row does not reach is built on purpose in tests/moe_route_edge_cases.py: a winner at every (lane, slot)
position; one lane that supplies every winner; rows that are one tie; -inf, +inf and NaN logits and selection biases, where the
order is "finite keys, then -inf keys, then NaN keys, each by index"; every 16-bit logit value through to_f32, expf and the
division; a batch longer than the chip holds at once; and the Python entry on views. The tolerance for weights is the same
everywhere: WEIGHT_FACTOR times the torch composition's error on the same GPU, floor WEIGHT_FLOOR."""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple, Optional

import numpy as np
import torch

FIRST_ES = (1, 8, 60, 64, 72, 128, 1024)            # the grid of the first 29 cases: NI = 1, 2, 16
LATER_ES = (65, 129, 160, 256, 257, 384, 512, 513)  # appended: NI = 2, 4, 8, 16 at their edges; DeepSeek-V2 / -V3 and Kimi-K2's E
ES = FIRST_ES + LATER_ES
SS = (1, 2, 8, 16)
TS = (1, 3, 16, 37)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
SCORINGS = ("softmax", "sigmoid")
MAX_EXPERTS, MAX_TOP_K = 1024, 16
HI_COUNT, HI_LEVELS = 20, 8
KEY_GAP = 1e-3
WEIGHT_FLOOR = 2.0 ** -20   # |l - max| <= 8: argument rounding, expf, the sum and the division: about 16 fp32 ulps
WEIGHT_FACTOR = 4.0         # two correct expf + division implementations legitimately differ by a few ulps


class RouteCase(NamedTuple):
    E: int
    S: int
    T: int
    dtype: torch.dtype
    scoring: str
    renormalize: bool
    bias: bool

    @property
    def scale(self) -> float:
        return 2.5 if (self.scoring == "sigmoid" and self.renormalize) else 1.0   # (DeepSeek-V3's routed_scaling_factor)

    @property
    def seed(self) -> int:
        return 1000 * self.E + 10 * self.S + self.T

    @property
    def name(self) -> str:
        return (f"E{self.E}-S{self.S}-T{self.T}-{str(self.dtype).replace('torch.', '')}-{self.scoring}-"
                f"{'renorm' if self.renormalize else 'raw'}-{'bias' if self.bias else 'nobias'}")


AXES = (ES, SS, TS, DTYPES, SCORINGS, (True, False), (False, True))
FIRST_AXES = (FIRST_ES,) + AXES[1:]


def lane_slots(E: int) -> int:
    """NI of csrc/moe_route.hip: the experts a lane holds, ceil(E / 64) rounded up to a power of two."""
    per_lane = (E + 63) // 64
    return next(n for n in (1, 2, 4, 8, 16) if per_lane <= n)


def valid(combo) -> bool:
    return combo[1] <= combo[0]


def all_pairs():
    """Every (axis a, value, axis b, value) that a valid combination can hold."""
    out = set()
    for combo in itertools.product(*AXES):
        if valid(combo):
            for a, b in itertools.combinations(range(len(AXES)), 2):
                out.add((a, combo[a], b, combo[b]))
    return out


def _greedy(axes, wanted):
    """Greedy cover, in a fixed order (a pure function of its arguments), of those value pairs of the valid combinations of `axes`
    that `wanted` accepts; only combinations that hold such a pair are candidates."""
    axis_pairs = tuple(itertools.combinations(range(len(axes)), 2))
    pairs_of = {}
    for c in itertools.product(*axes):
        if valid(c):
            mine = frozenset(q for q in ((a, c[a], b, c[b]) for a, b in axis_pairs) if wanted(q))
            if mine:
                pairs_of[c] = mine
    todo = set().union(*pairs_of.values())
    chosen = []
    while todo:
        best = max(pairs_of, key=lambda c: len(pairs_of[c] & todo))   # (the first of equals: dicts keep insertion order)
        chosen.append(best)
        todo -= pairs_of[best]
    return chosen


def pairwise():
    """The pairwise cover of the first grid (FIRST_ES: the 29 cases the kernel came with, unchanged and in their order), then a
    greedy cover of every value pair that involves one of LATER_ES. Together: every pair of AXES."""
    first = _greedy(FIRST_AXES, lambda q: True)
    later = _greedy(AXES, lambda q: q[0] == 0 and q[1] in LATER_ES)
    return tuple(RouteCase(*c) for c in first + later)


CASES = pairwise()


def build_logits(E: int, T: int, seed: int) -> torch.Tensor:
    """[T, E] float64, multiples of 1/8 in [-4, 4]: the construction of the file head."""
    rng = np.random.RandomState(seed)
    out = np.empty((T, E), dtype=np.float64)
    for t in range(T):
        out[t, :] = -4.0 + rng.randint(0, 17) / 8.0                       # the background level, -4 ... -2
        hi = rng.permutation(E)[:min(E, HI_COUNT)]
        out[t, hi] = 4.0 - rng.randint(0, HI_LEVELS, size=hi.size) / 8.0  # 4 ... 3.125
    return torch.from_numpy(out)


def build_bias(E: int, S: int, seed: int) -> torch.Tensor:
    """[E] float32, multiples of 1/4: +1 on max(1, S // 2) experts, -1 on E // 8 others, 0 elsewhere."""
    rng = np.random.RandomState(seed + 7)
    order = rng.permutation(E)
    up = max(1, S // 2)
    out = np.zeros(E, dtype=np.float32)
    out[order[:up]] = 1.0
    out[order[up:up + E // 8]] = -1.0
    return torch.from_numpy(out)


def scores64(logits: torch.Tensor, scoring: str) -> torch.Tensor:
    l = logits.double()
    return torch.softmax(l, dim=-1) if scoring == "softmax" else torch.sigmoid(l)


def assert_unambiguous(logits: torch.Tensor, scoring: str, bias: Optional[torch.Tensor]) -> float:
    """Every row: two keys come from identical (logit, bias) pairs or differ by more than KEY_GAP - in float64. Returns the smallest
    gap between two different keys (inf if a row has one key class only)."""
    l = logits.double()
    b = torch.zeros(l.shape[-1], dtype=torch.float64) if bias is None else bias.double()
    assert bool((l * 8 == torch.round(l * 8)).all()) and float(l.abs().max()) <= 4.0, "logits must be multiples of 1/8 in [-4, 4]"
    assert bool((b * 4 == torch.round(b * 4)).all()), "select_bias must hold multiples of 1/4"
    key = scores64(l, scoring) + b
    assert bool(torch.isfinite(key).all())
    smallest = float("inf")
    for t in range(l.shape[0]):
        order = torch.argsort(key[t], stable=True)
        k, lo, bo = key[t][order], l[t][order], b[order]
        same = (lo[1:] == lo[:-1]) & (bo[1:] == bo[:-1])
        gap = k[1:] - k[:-1]
        assert bool((same | (gap > KEY_GAP)).all()), f"row {t}: two keys from different (logit, bias) pairs are within {KEY_GAP}"
        assert bool((gap[same] == 0).all())
        if bool((~same).any()):
            smallest = min(smallest, float(gap[~same].min()))
    return smallest


def reference(logits: torch.Tensor, S: int, scoring: str, renormalize: bool, scale: float, bias: Optional[torch.Tensor]):
    """float64: (ids int32 [T, S], weights float64 [T, S]). Ranking by (key descending, index ascending); NaN keys last, by index."""
    p = scores64(logits, scoring)
    key = p if bias is None else p + bias.double()
    kn, idx = key.numpy(), np.arange(key.shape[-1])
    ids = np.stack([np.lexsort((idx, -np.where(np.isnan(row), -np.inf, row), np.isnan(row)))[:S] for row in kn])
    ids = torch.from_numpy(ids)
    w = p.gather(-1, ids)
    if renormalize:
        total = w[:, 0].clone()
        for s in range(1, S):
            total = total + w[:, s]
        w = w / total.unsqueeze(-1)
    return ids.to(torch.int32), w * scale


class Built(NamedTuple):
    logits: torch.Tensor            # [T, E] in the case's dtype (exact)
    bias: Optional[torch.Tensor]    # [E] float32 or None
    ids: torch.Tensor               # the float64 ranking
    weights: torch.Tensor           # float64


@functools.lru_cache(maxsize=None)
def build(case: RouteCase) -> Built:
    l64 = build_logits(case.E, case.T, case.seed)
    bias = build_bias(case.E, case.S, case.seed) if case.bias else None
    logits = l64.to(case.dtype)
    assert torch.equal(logits.double(), l64)
    ids, w = reference(logits, case.S, case.scoring, case.renormalize, case.scale, bias)
    return Built(logits, bias, ids, w)


def max_rel_err(w: torch.Tensor, w64: torch.Tensor) -> float:
    return float(((w.double().cpu() - w64).abs() / w64.abs()).max())


class CountedEntry:
    """Counts the calls of bnb_mi355x_moe_topk that the Python layer makes while it is active."""

    def __enter__(self):
        from bitsandbytes_amd.backends import hip

        self.hip, self.real, self.calls = hip, hip.lib, 0
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(outer.real, name)
                if name != "bnb_mi355x_moe_topk":
                    return fn

                def counted(*args):
                    outer.calls += 1
                    return fn(*args)

                return counted

        hip.lib = Proxy()
        return self

    def __exit__(self, *exc):
        self.hip.lib = self.real
        return False
