"""CPU (-m "not gpu"): the host side of group-limited MoE routing (bitsandbytes_amd::moe_topk_grouped, bitsandbytes_amd.moe_topk_grouped /
moe_route_grouped, nn.MoERouter(n_group=...)) - C ABI and its refusals, predicate, op schema / fake kernel, the torch composition
against float64 - and the preconditions of every case tests/test_gpu_moe_route_grouped.py runs: rankings and group rankings that are
unambiguous in float64 (tests/moe_route_grouped_cases.py)."""
import ctypes as ct
import fnmatch
import inspect
import os
import re

import pytest
import torch

import moe_route_cases as C
import moe_route_grouped_cases as GC
from conftest import ROOT

SYMBOLS = ("bnb_mi355x_moe_topk_grouped", "bnb_mi355x_moe_topk_grouped_supported")
FIELDS = ["struct_bytes", "logits_dtype", "scoring", "renormalize", "rows", "experts", "top_k", "n_group", "topk_group", "group_score", "scale",
          "logits", "select_bias", "ids", "weights", "stream"]


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.moe_topk_grouped.default


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_exported_and_listed():
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "bitsandbytes_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert ce.lib, f"{ce.LIB_PATH} not built"
    dll = ct.CDLL(str(ce.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\s*\(", code, flags=re.M), f"{name} is not declared in include/bnb_mi355x.h"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), f"{name} is not covered by exports.map"
        assert name in ce.EXPORTED_SYMBOLS and hasattr(dll, name), name
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS)
    assert "Out of scope: group-limited routing" not in notes


def test_argument_block_matches_the_header():
    """ctypes' MoeTopkGroupedArgs field by field against the struct in include/bnb_mi355x.h: the fields of bnb_mi355x_moe_topk_args and
    the three of the group stage; no parenthesis inside the struct; the stream is a field, not a parameter."""
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    m = re.search(r"typedef struct bnb_mi355x_moe_topk_grouped_args \{(.*?)\} bnb_mi355x_moe_topk_grouped_args;", header, flags=re.S)
    assert m, "struct bnb_mi355x_moe_topk_grouped_args is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert "(" not in m.group(1) and ")" not in m.group(1)
    names = [re.sub(r"^\W+", "", d.strip().split()[-1]) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    assert names == [f[0] for f in ce.MoeTopkGroupedArgs._fields_] == FIELDS
    assert set(f[0] for f in ce.MoeTopkArgs._fields_) | {"n_group", "topk_group", "group_score"} == set(FIELDS)
    A = ce.MoeTopkGroupedArgs
    assert ct.sizeof(A) == 88 and A.n_group.offset == 32 and A.scale.offset == 44 and A.logits.offset == 48 and A.stream.offset == 80
    decl = re.search(r"^int bnb_mi355x_moe_topk_grouped\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert decl and "bnb_stream_t" not in decl.group(1) and decl.group(1).strip() == "const bnb_mi355x_moe_topk_grouped_args* args"
    decl = re.search(r"^int bnb_mi355x_moe_topk_grouped_supported\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert decl and [a.split()[-1] for a in decl.group(1).split(",")] == ["logits_dtype", "rows", "experts", "top_k", "n_group", "topk_group",
                                                                          "group_score"]
    assert ce.lib.bnb_mi355x_moe_topk_grouped.restype is ct.c_int32 and len(ce.lib.bnb_mi355x_moe_topk_grouped_supported.argtypes) == 7
    # the block of the ungrouped entry keeps its size: the two entries refuse each other's block
    assert ct.sizeof(ce.MoeTopkArgs) == 80


def _args(**over):
    """An argument block inside every precondition (E = 8 in 4 groups, 2 kept, top2sum); the pointers are never dereferenced on the
    host (a refused call launches nothing)."""
    from bitsandbytes_amd.cextension import MoeTopkGroupedArgs

    keep = [(ct.c_float * 64)(), (ct.c_float * 8)(), (ct.c_int * 8)(), (ct.c_float * 8)()]
    a = MoeTopkGroupedArgs(ct.sizeof(MoeTopkGroupedArgs), 0, 1, 1, 4, 8, 2, 4, 2, 1, 1.0, ct.addressof(keep[0]), ct.addressof(keep[1]),
                           ct.addressof(keep[2]), ct.addressof(keep[3]), None)
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = keep
    return a


REFUSALS = {
    "struct_bytes_of_the_ungrouped_block": dict(struct_bytes=80), "struct_bytes_large": dict(struct_bytes=96), "struct_bytes_zero": dict(struct_bytes=0),
    "null_logits": dict(logits=None), "null_ids": dict(ids=None), "null_weights": dict(weights=None),
    "dtype_low": dict(logits_dtype=-1), "dtype_high": dict(logits_dtype=3), "scoring_low": dict(scoring=-1), "scoring_high": dict(scoring=2),
    "experts_zero": dict(experts=0), "experts_1025": dict(experts=1025, n_group=25), "experts_2048": dict(experts=2048, n_group=8),
    "n_group_does_not_divide": dict(experts=8, n_group=3), "n_group_zero": dict(n_group=0), "n_group_negative": dict(n_group=-4),
    "n_group_65": dict(experts=130, n_group=65, topk_group=4), "n_group_128": dict(experts=256, n_group=128, topk_group=4),
    "topk_group_zero": dict(topk_group=0), "topk_group_negative": dict(topk_group=-1), "topk_group_above_n_group": dict(topk_group=5),
    "top_k_zero": dict(top_k=0), "top_k_above_the_kept_experts": dict(top_k=5), "top_k_17": dict(experts=64, top_k=17),
    "groups_of_one_with_top2sum": dict(n_group=8, topk_group=4, group_score=1), "group_score_low": dict(group_score=-1),
    "group_score_high": dict(group_score=2), "rows_negative": dict(rows=-1),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_non_zero_without_a_device(name, capfd):
    lib = _bnb().lib
    a = _args(**REFUSALS[name])
    assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(a)) != 0
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("bitsandbytes_amd: moe_topk_grouped: "), err


def test_misaligned_pointers_and_a_null_block_are_refused_and_no_rows_is_not(capfd):
    lib = _bnb().lib
    for field in ("logits", "ids", "weights", "select_bias"):
        a = _args()
        setattr(a, field, getattr(a, field) + 1)
        assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(a)) != 0, field
    assert lib.bnb_mi355x_moe_topk_grouped(None) != 0
    capfd.readouterr()
    # rows == 0: 0, nothing launched (no device here: a launch would not return 0), with or without pointers, in both modes
    assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(_args(rows=0))) == 0
    assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(_args(rows=0, group_score=0, n_group=8, topk_group=2, logits=None, ids=None, weights=None,
                                                          select_bias=None))) == 0
    assert capfd.readouterr().err == ""
    # ... but not past a refusal
    assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(_args(rows=0, n_group=3))) != 0
    assert lib.bnb_mi355x_moe_topk_grouped(ct.byref(_args(rows=0, top_k=5))) != 0


def _want(dt, rows, E, S, n_group, topk_group, mode):
    if not (0 <= dt <= 2 and rows >= 1 and 1 <= E <= 1024 and 1 <= n_group <= 64 and E % n_group == 0 and 1 <= topk_group <= n_group and mode in (0, 1)):
        return 0
    G = E // n_group
    return int((G >= 2 or mode == 0) and 1 <= S <= min(16, topk_group * G))


def test_predicate_edges():
    """bnb_mi355x_moe_topk_grouped_supported at the edges of every precondition: pure host logic."""
    sup = _bnb().lib.bnb_mi355x_moe_topk_grouped_supported
    for dt in (-1, 0, 1, 2, 3):
        for rows in (-1, 0, 1, 37, 4096):
            for E, n_group in ((0, 1), (1, 1), (8, 3), (8, 4), (8, 8), (64, 64), (65, 65), (130, 65), (128, 64), (1024, 16), (1024, 1), (1025, 1),
                               (1025, 25), (2048, 64), (160, 8), (64, 0), (64, -8)):
                for topk_group in sorted({0, 1, 2, n_group, n_group + 1}):
                    for S in sorted({0, 1, 2, 16, 17, topk_group * (E // n_group if n_group > 0 else 0), topk_group * (E // n_group if n_group > 0 else 0) + 1}):
                        for mode in (-1, 0, 1, 2):
                            assert sup(dt, rows, E, S, n_group, topk_group, mode) == _want(dt, rows, E, S, n_group, topk_group, mode), \
                                (dt, rows, E, S, n_group, topk_group, mode)
    for E, n_group, topk_group, S in GC.GEOMETRIES:
        assert sup(2, 1, E, S, n_group, topk_group, 0) == 1 and sup(2, 1, E, S, n_group, topk_group, 1) == int(E // n_group >= 2)
    from bitsandbytes_amd.backends import hip

    assert hip.moe_topk_grouped_supported(torch.bfloat16, 1, 256, 8, 8, 4) and hip.moe_topk_grouped_supported(torch.float32, 16, 160, 6, 8, 3, "max")
    assert hip.moe_topk_grouped_supported(torch.float16, 37, 1024, 16, 16, 4, "top2sum")
    assert not hip.moe_topk_grouped_supported(torch.float64, 1, 256, 8, 8, 4) and not hip.moe_topk_grouped_supported(torch.bfloat16, 1, 2048, 8, 8, 4)
    assert not hip.moe_topk_grouped_supported(torch.bfloat16, 1, 256, 8, 128, 4) and not hip.moe_topk_grouped_supported(torch.bfloat16, 1, 256, 8, 8, 4, "mean")
    assert not hip.moe_topk_grouped_supported(torch.bfloat16, 2 ** 31, 256, 8, 8, 4) and not hip.moe_topk_grouped_supported(torch.bfloat16, 1, 64, 8, 64, 8)
    assert hip.moe_topk_grouped_supported(torch.bfloat16, 1, 64, 8, 64, 8, "max")


# ------------------------------------------------------------------------------------------ op schema, fake kernel, signatures
def test_public_surface():
    bnb = _bnb()
    assert str(_op()._schema) == ("bitsandbytes_amd::moe_topk_grouped(Tensor logits, int top_k, int n_group, int topk_group, str group_score, "
                                  "str scoring, bool renormalize, float scale, Tensor? select_bias=None) -> (Tensor, Tensor)")
    for name in ("moe_topk_grouped", "moe_route_grouped"):
        assert callable(getattr(bnb, name)) and name in bnb.__all__
    p = inspect.signature(bnb.moe_topk_grouped).parameters
    assert list(p) == ["logits", "top_k", "n_group", "topk_group", "group_score", "scoring", "renormalize", "scale", "select_bias"]
    assert [p[n].default for n in list(p)[4:]] == ["top2sum", "sigmoid", True, 1.0, None]
    p = inspect.signature(bnb.moe_route_grouped).parameters
    assert list(p) == ["x", "router_weight", "top_k", "n_group", "topk_group", "group_score", "bias", "scoring", "renormalize", "scale",
                       "select_bias", "return_logits"]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[5:]) and p["return_logits"].default is False
    assert (p["group_score"].default, p["scoring"].default) == ("top2sum", "sigmoid")
    # what was there keeps its signature
    p = inspect.signature(bnb.moe_topk).parameters
    assert list(p) == ["logits", "top_k", "scoring", "renormalize", "scale", "select_bias"]
    assert (p["scoring"].default, p["renormalize"].default, p["scale"].default, p["select_bias"].default) == ("softmax", True, 1.0, None)
    p = inspect.signature(bnb.moe_route).parameters
    assert list(p) == ["x", "router_weight", "top_k", "bias", "scoring", "renormalize", "scale", "select_bias", "return_logits"]
    p = inspect.signature(bnb.nn.MoERouter.__init__).parameters
    assert list(p)[:9] == ["self", "hidden", "num_experts", "top_k", "scoring", "renormalize", "scale", "bias", "select_bias"]
    assert list(p)[-3:] == ["n_group", "topk_group", "group_score"] and [p[n].default for n in list(p)[-3:]] == [1, 1, "top2sum"]
    assert "moe_topk_grouped" in bnb.moe_topk.__doc__ and "is not served" not in bnb.moe_topk.__doc__


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_fake_kernel_shapes_and_dtypes(dtype):
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        for E, S, n_group, topk_group, mode in ((8, 2, 4, 2, "top2sum"), (160, 6, 8, 3, "max"), (1024, 16, 16, 4, "top2sum"), (4096, 32, 128, 64, "max"),
                                                (64, 16, 64, 16, "max"), (1, 1, 1, 1, "max")):
            logits = torch.empty((*lead, E), dtype=dtype, device="meta")
            for bias in (None, torch.empty(E, dtype=torch.float32, device="meta")):
                ids, w = _op()(logits, S, n_group, topk_group, mode, "sigmoid", True, 2.5, bias)
                assert ids.shape == w.shape == (*lead, S) and ids.dtype == torch.int32 and w.dtype == torch.float32
                assert ids.device.type == w.device.type == "meta" and ids.is_contiguous() and w.is_contiguous()


def test_fake_kernel_rejects_bad_arguments():
    logits = torch.empty((3, 64), dtype=torch.bfloat16, device="meta")
    f32 = torch.empty(64, dtype=torch.float32, device="meta")
    ok = (8, 4, "top2sum", "sigmoid", True, 1.0)
    for match, args in (("scoring must be", (logits, 2, 8, 4, "top2sum", "tanh", True, 1.0)), ("group_score must be", (logits, 2, 8, 4, "mean", "sigmoid", True, 1.0)),
                        ("top_k must be", (logits, 0, *ok)), ("top_k must be", (logits, 65, *ok)), ("top_k must be at most", (logits, 33, *ok)),
                        ("n_group must be", (logits, 2, 7, 4, "top2sum", "sigmoid", True, 1.0)), ("n_group must be", (logits, 2, 0, 1, "max", "sigmoid", True, 1.0)),
                        ("topk_group must be", (logits, 2, 8, 0, "top2sum", "sigmoid", True, 1.0)), ("topk_group must be", (logits, 2, 8, 9, "top2sum", "sigmoid", True, 1.0)),
                        ("at least 2 experts", (logits, 2, 64, 4, "top2sum", "sigmoid", True, 1.0)),
                        ("16/32-bit float", (logits.to(torch.int32), 2, *ok)), ("contiguous", (logits[:, ::2], 2, 8, 4, "top2sum", "sigmoid", True, 1.0)),
                        ("select_bias must be", (logits, 2, *ok, f32[:32])), ("select_bias must be", (logits, 2, *ok, f32.bfloat16()))):
        with pytest.raises(RuntimeError, match=match):
            _op()(*args)


# ------------------------------------------------------------------------------------------ the cases and the composition
def test_the_grid_is_covered_pairwise():
    assert GC.CASES == GC.pairwise() and len({c.name for c in GC.CASES}) == len(GC.CASES)
    assert 30 <= len(GC.CASES) <= 48
    covered = set()
    for c in GC.CASES:
        assert GC.valid(c) and c.geometry in GC.GEOMETRIES and c.T in GC.TS and c.E == c.n_group * c.G
        assert c.topk_group <= c.n_group <= GC.MAX_GROUPS and c.S <= min(GC.MAX_TOP_K, c.topk_group * c.G) and c.E <= GC.MAX_EXPERTS
        covered |= {(a, c[a], b, c[b]) for a in range(7) for b in range(a + 1, 7)}
    assert covered == GC.all_pairs()
    assert {c.geometry for c in GC.CASES} == set(GC.GEOMETRIES) and {c.dtype for c in GC.CASES} == set(C.DTYPES)
    # the geometries the kernel's structure names: groups of 1, of 2, straddling lanes (10, 20) and slots (36), NI = 1 ... 16, 64 groups
    assert {C.lane_slots(c.E) for c in GC.CASES} == {1, 2, 4, 8, 16} and {1, 2, 10, 20, 36, 64} <= {c.G for c in GC.CASES}
    assert any(c.n_group == 64 for c in GC.CASES) and any(c.G % 2 and c.G > 1 or 64 % c.G for c in GC.CASES)
    for geometry in GC.GEOMETRIES:
        mine = [c for c in GC.CASES if c.geometry == geometry]
        assert {c.scoring for c in mine} == set(C.SCORINGS) and {c.bias for c in mine} == {True, False} and {c.T for c in mine} == set(GC.TS)
        assert {c.group_score for c in mine} == ({"max"} if geometry[0] == geometry[1] else {"max", "top2sum"})


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.name)
def test_rankings_are_unambiguous_and_the_composition_agrees_with_float64(case):
    """The builder's promises, asserted in float64 for every row (none dropped): key gaps, group-score gaps, a cut inside a planted
    group tie and ids that the ungrouped ranking does not give. Then the public function on CPU tensors - the torch composition -
    against the float64 restatement of the rules: ids exactly, weights to fp32 rounding."""
    b = GC.build(case)
    assert b.logits.shape == (case.T, case.E) and b.logits.dtype == case.dtype
    assert b.gap > GC.GROUP_GAP
    gap, tied_cuts = GC.assert_unambiguous(b.logits, case.n_group, case.topk_group, case.group_score, case.scoring, b.bias)
    assert gap == b.gap
    if case.topk_group < case.n_group:
        assert tied_cuts and bool((b.kept.sum(-1) == case.topk_group).all())
        assert bool(b.differs) != GC.coincides_with_ungrouped(case)
    assert b.ids.dtype == torch.int32 and all(len(set(r.tolist())) == case.S for r in b.ids) and bool(((b.ids >= 0) & (b.ids < case.E)).all())
    assert bool(b.kept.gather(-1, (b.ids // case.G).long()).all()), "an id outside the kept groups"
    with torch.no_grad():
        ids, w = _bnb().moe_topk_grouped(b.logits, case.S, case.n_group, case.topk_group, case.group_score, case.scoring, case.renormalize,
                                         case.scale, b.bias)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (case.T, case.S)
    assert torch.equal(ids, b.ids)
    assert C.max_rel_err(w, b.weights) <= C.WEIGHT_FLOOR   # (16 fp32 ulps: moe_route_cases' estimate for |l - max| <= 8)
    if case.renormalize:
        assert torch.allclose(w.sum(-1), torch.full((case.T,), case.scale), rtol=1e-6)


def test_the_two_group_scores_choose_different_experts():
    """On the same inputs "max" keeps the lone stars and "top2sum" drops them: the ids differ (every case with high groups of two or
    more experts and dropped groups; row 0 by construction)."""
    seen = 0
    for case in GC.CASES:
        if case.G >= 2 and case.topk_group < case.n_group and GC.layout(case).highs:
            b = GC.build(case)
            other = "max" if case.group_score == "top2sum" else "top2sum"
            ids, _, kept = GC.reference(b.logits, case.S, case.n_group, case.topk_group, other, case.scoring, case.renormalize, case.scale, b.bias)
            assert not torch.equal(kept, b.kept) and not torch.equal(ids, b.ids), case.name
            with torch.no_grad():
                got, _ = _bnb().moe_topk_grouped(b.logits, case.S, case.n_group, case.topk_group, other, case.scoring, case.renormalize, case.scale, b.bias)
            assert torch.equal(got, ids)
            seen += 1
    assert seen >= 20


def test_reference_on_a_row_worked_by_hand():
    """E = 8 in 4 groups of 2, 2 kept, sigmoid. Keys by group: (0.9, 0.1) (0.6, 0.6) (0.7, 0.2) (0.6, 0.6): "max" keeps groups 0 and 2,
    "top2sum" (1.0, 1.2, 0.9, 1.2) keeps 1 and 3 - a tie, and the cut behind it. Then a dropped expert (0.9) is not a key of 0: a kept
    expert with a negative biased key goes before it."""
    p = torch.tensor([[0.9, 0.1, 0.6, 0.6, 0.7, 0.2, 0.6, 0.6]], dtype=torch.float64)
    logits = torch.log(p / (1 - p))
    ids, w, kept = GC.reference(logits, 3, 4, 2, "max", "sigmoid", False, 1.0, None)
    assert ids.tolist() == [[0, 4, 5]] and kept.tolist() == [[True, False, True, False]]
    ids, w, kept = GC.reference(logits, 3, 4, 2, "top2sum", "sigmoid", False, 1.0, None)
    assert ids.tolist() == [[2, 3, 6]] and kept.tolist() == [[False, True, False, True]] and torch.allclose(w, torch.full((1, 3), 0.6, dtype=torch.float64))
    ids, _, kept = GC.reference(logits, 2, 4, 1, "top2sum", "sigmoid", False, 1.0, None)
    assert ids.tolist() == [[2, 3]] and kept.tolist() == [[False, True, False, False]]
    bias = torch.tensor([0, 0, 0, -1.0, 0, 0, 0, 0])
    ids, w, _ = GC.reference(logits, 4, 4, 2, "top2sum", "sigmoid", False, 1.0, bias)   # (scores 1.0, 0.2, 0.9, 1.2: groups 3 and 0)
    assert ids.tolist() == [[0, 6, 7, 1]]
    for mode, want in (("max", [[0, 4, 5]]), ("top2sum", [[2, 3, 6]])):
        got, gw = _bnb().moe_topk_grouped(logits.float(), 3, 4, 2, mode, "sigmoid", False)
        assert got.tolist() == want
    got, gw = _bnb().moe_topk_grouped(logits.float(), 4, 4, 2, "top2sum", "sigmoid", False, 1.0, bias)
    assert got.tolist() == [[0, 6, 7, 1]] and torch.allclose(gw, torch.tensor([[0.9, 0.6, 0.6, 0.1]]), rtol=1e-6)
    # expert 3 of a kept group at 0.6 - 1 < 0: it still goes before every expert of the dropped groups (a 0.0 fill would not let it)
    got, _ = _bnb().moe_topk_grouped(logits.float(), 4, 4, 2, "max", "sigmoid", False, 1.0, torch.tensor([0, 0, 0.5, -1.0, 0, 0, 0, 0]))
    assert got.tolist() == [[2, 0, 1, 3]]   # ("max": 0.9, 1.1, 0.7, 0.6 keeps groups 1 and 0; expert 3's key is -0.4)


def test_composition_non_finite_rules():
    """NaN group scores go last, -inf ones in front of them, ties to the lower group; the experts of dropped groups never appear."""
    bnb = _bnb()
    nan, inf = float("nan"), float("inf")
    l = torch.zeros(2, 12)
    l[0, 0:3] = nan        # group 0: every key NaN
    l[0, 9] = 2.0
    l[1, 4] = nan          # group 1: one NaN key; "max" sees the finite ones, "top2sum" too (3 experts a group)
    l[1, 3], l[1, 5] = 1.0, 1.0
    sb = torch.zeros(12)
    sb[6:9] = -inf         # group 2: every key -inf
    for mode in ("max", "top2sum"):
        ids, w = bnb.moe_topk_grouped(l, 3, 4, 3, mode, "sigmoid", False, 1.0, sb)
        want, _, kept = GC.reference(l, 3, 4, 3, mode, "sigmoid", False, 1.0, sb)
        assert torch.equal(ids, want)
        assert kept.tolist() == [[False, True, True, True], [True, True, False, True]]
        assert ids[0].tolist() == [9, 3, 4] and ids[1].tolist() == [3, 5, 0]
    # a group whose only finite key is one expert (the others NaN): "max" is that key, "top2sum" is NaN and the group goes last
    l = torch.zeros(1, 8)
    l[0, 1], l[0, 0] = nan, 3.0
    assert GC.reference(l, 2, 4, 3, "max", "sigmoid", False, 1.0, None)[2].tolist() == [[True, True, True, False]]
    assert GC.reference(l, 2, 4, 3, "top2sum", "sigmoid", False, 1.0, None)[2].tolist() == [[False, True, True, True]]
    for mode in ("max", "top2sum"):
        assert torch.equal(bnb.moe_topk_grouped(l, 2, 4, 3, mode, "sigmoid", False)[0], GC.reference(l, 2, 4, 3, mode, "sigmoid", False, 1.0, None)[0])


@pytest.mark.parametrize("scoring", C.SCORINGS)
def test_one_group_or_every_group_kept_is_moe_topk_bit_for_bit(scoring):
    bnb = _bnb()
    gen = torch.Generator().manual_seed(3)
    for E, S in sorted({(g[0], g[3]) for g in GC.GEOMETRIES}):
        logits = (torch.randint(-32, 33, (5, E), generator=gen) / 8).bfloat16()
        sb = (torch.randint(-2, 3, (E,), generator=gen) / 4).float()
        want = bnb.moe_topk(logits, S, scoring, True, 2.5, sb)
        for n_group in sorted({1, 2 if E % 2 == 0 else 1, *(g[1] for g in GC.GEOMETRIES if g[0] == E)}):
            for mode in ("max", "top2sum"):
                if mode == "top2sum" and E // n_group < 2:
                    continue
                for topk_group in {n_group} | ({1} if n_group == 1 else set()):
                    ids, w = bnb.moe_topk_grouped(logits, S, n_group, topk_group, mode, scoring, True, 2.5, sb)
                    assert torch.equal(ids, want[0]) and torch.equal(w.view(torch.int32), want[1].view(torch.int32)), (E, n_group, mode)


def test_public_functions_check_their_arguments():
    bnb = _bnb()
    l = torch.zeros(3, 8)
    for exc, match, call in ((ValueError, "scoring", lambda: bnb.moe_topk_grouped(l, 2, 4, 2, scoring="tanh")),
                             (ValueError, "group_score", lambda: bnb.moe_topk_grouped(l, 2, 4, 2, "mean")),
                             (ValueError, "n_group", lambda: bnb.moe_topk_grouped(l, 2, 3, 2)), (ValueError, "n_group", lambda: bnb.moe_topk_grouped(l, 2, 0, 1)),
                             (ValueError, "topk_group", lambda: bnb.moe_topk_grouped(l, 2, 4, 0)), (ValueError, "topk_group", lambda: bnb.moe_topk_grouped(l, 2, 4, 5)),
                             (ValueError, "top_k", lambda: bnb.moe_topk_grouped(l, 5, 4, 2)), (ValueError, "top_k", lambda: bnb.moe_topk_grouped(l, 0, 4, 2)),
                             (ValueError, "at least 2", lambda: bnb.moe_topk_grouped(l, 2, 8, 4)),
                             (ValueError, "select_bias", lambda: bnb.moe_topk_grouped(l, 2, 4, 2, select_bias=torch.zeros(4))),
                             (ValueError, "float tensor", lambda: bnb.moe_topk_grouped(l.long(), 2, 4, 2)),
                             (RuntimeError, "inference only", lambda: bnb.moe_topk_grouped(l.clone().requires_grad_(), 2, 4, 2)),
                             (ValueError, r"\[E, K\]", lambda: bnb.moe_route_grouped(torch.zeros(3, 16), torch.zeros(8, 32), 2, 4, 2)),
                             (ValueError, "bias must be", lambda: bnb.moe_route_grouped(torch.zeros(3, 16), torch.zeros(8, 16), 2, 4, 2, bias=torch.zeros(4))),
                             (RuntimeError, "inference only", lambda: bnb.moe_route_grouped(torch.zeros(3, 16).requires_grad_(), torch.zeros(8, 16), 2, 4, 2))):
        with pytest.raises(exc, match=match):
            call()
    # groups of one are served by "max"; sizes past the kernel's go to the composition
    assert bnb.moe_topk_grouped(l, 2, 8, 4, "max")[0].shape == (3, 2)
    big = torch.randn(2, 2048)
    ids, w = bnb.moe_topk_grouped(big, 24, 128, 16)
    want, _, _ = GC.reference(big, 24, 128, 16, "top2sum", "sigmoid", True, 1.0, None)
    assert torch.equal(ids, want)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_moe_route_grouped_composes_on_cpu(dtype):
    bnb = _bnb()
    gen = torch.Generator().manual_seed(5)
    K, E, S = 64, 24, 4
    W = (torch.randn(E, K, generator=gen) / K ** 0.5).to(dtype)
    bias = torch.randn(E, generator=gen).to(dtype)
    sb = (torch.randint(-2, 3, (E,), generator=gen) / 4).float()
    with torch.no_grad():
        for lead in ((1,), (5,), (2, 3)):
            x = torch.randn(*lead, K, generator=gen).to(dtype)
            for b in (None, bias):
                logits = torch.nn.functional.linear(x, W, b)
                ids, w, got = bnb.moe_route_grouped(x, W, S, 4, 2, group_score="max", bias=b, renormalize=True, scale=2.5, select_bias=sb,
                                                    return_logits=True)
                assert torch.equal(got, logits) and ids.shape == w.shape == (*lead, S)
                assert torch.equal(got, bnb.moe_route(x, W, S, bias=b, return_logits=True)[2])
                want_ids, want_w = bnb.moe_topk_grouped(logits, S, 4, 2, "max", "sigmoid", True, 2.5, sb)
                assert torch.equal(ids, want_ids) and torch.equal(w, want_w)
                assert len(bnb.moe_route_grouped(x, W, S, 4, 2, bias=b)) == 2


# ------------------------------------------------------------------------------------------ the module
def test_module_routes_by_groups_and_round_trips_its_state_dict():
    bnb = _bnb()
    kw = dict(scoring="sigmoid", renormalize=True, scale=2.5, select_bias=True)
    router = bnb.nn.MoERouter(32, 64, 6, n_group=8, topk_group=4, **kw)
    assert list(router.state_dict()) == ["weight", "e_score_correction_bias"]
    assert "n_group=8, topk_group=4, group_score='top2sum'" in router.extra_repr()
    plain = bnb.nn.MoERouter(32, 64, 6, **kw)
    assert "n_group" not in plain.extra_repr() and plain.extra_repr() == router.extra_repr().split(", n_group")[0]
    gen = torch.Generator().manual_seed(9)
    sd = {"weight": torch.randn(64, 32, generator=gen), "e_score_correction_bias": (torch.randint(-2, 3, (64,), generator=gen) / 4).float()}
    router.load_state_dict(sd)
    other = bnb.nn.MoERouter(32, 64, 6, n_group=8, topk_group=4, group_score="max", **kw)
    other.load_state_dict(router.state_dict())
    plain.load_state_dict(router.state_dict())
    assert all(torch.equal(other.state_dict()[k], v) for k, v in sd.items())
    x = torch.randn(7, 32, generator=gen)
    with torch.no_grad():
        for module, mode in ((router, "top2sum"), (other, "max")):
            ids, w = module(x)
            want = bnb.moe_route_grouped(x, sd["weight"], 6, 8, 4, group_score=mode, scoring="sigmoid", renormalize=True, scale=2.5,
                                         select_bias=sd["e_score_correction_bias"])
            assert ids.dtype == torch.int32 and w.dtype == torch.float32 and torch.equal(ids, want[0]) and torch.equal(w, want[1])
            assert all(len(set((row // 8).tolist())) <= 4 for row in ids)
        pids, pw = plain(x)
        assert torch.equal(pids, bnb.moe_route(x, sd["weight"], 6, scoring="sigmoid", renormalize=True, scale=2.5,
                                               select_bias=sd["e_score_correction_bias"])[0])
        assert not torch.equal(pids, router(x)[0])
    for bad in (dict(n_group=7, topk_group=2), dict(n_group=8, topk_group=9), dict(n_group=8, topk_group=0), dict(n_group=64, topk_group=8),
                dict(n_group=8, topk_group=4, group_score="mean")):
        with pytest.raises(ValueError, match="MoERouter"):
            bnb.nn.MoERouter(32, 64, 6, **bad)
    with pytest.raises(ValueError, match="top_k"):
        bnb.nn.MoERouter(32, 64, 9, n_group=8, topk_group=1)
