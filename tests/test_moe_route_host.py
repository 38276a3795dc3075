"""CPU (-m "not gpu"): the host side of the MoE router (bitsandbytes_amd::moe_topk, bitsandbytes_amd.moe_topk / moe_route,
nn.MoERouter) - C ABI and its refusals, predicate, op schema / fake kernel, the torch composition against float64 - and the
preconditions of every case tests/test_gpu_moe_route.py runs: rankings that are unambiguous in float64 (tests/moe_route_cases.py)."""
import copy
import ctypes as ct
import fnmatch
import hashlib
import inspect
import os
import re

import pytest
import torch

import moe_route_cases as C
from conftest import ROOT

SYMBOLS = ("bnb_mi355x_moe_topk", "bnb_mi355x_moe_topk_supported")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.moe_topk.default


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
    assert "moe_route.hip" in open(os.path.join(ROOT, "bitsandbytes_amd", "csrc", "Makefile")).read()
    assert "//" not in code.replace("://", ""), "the header's readers strip /* */ comments only"
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS)


def test_argument_block_matches_the_header():
    """ctypes' MoeTopkArgs field by field against the struct in include/bnb_mi355x.h; no parenthesis inside the struct (the header's
    regex readers take a parenthesis for a function), and the entry point has no bnb_stream_t parameter: the stream is a field."""
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    m = re.search(r"typedef struct bnb_mi355x_moe_topk_args \{(.*?)\} bnb_mi355x_moe_topk_args;", header, flags=re.S)
    assert m, "struct bnb_mi355x_moe_topk_args is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert "(" not in m.group(1) and ")" not in m.group(1)
    names = [re.sub(r"^\W+", "", d.strip().split()[-1]) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    assert names == [f[0] for f in ce.MoeTopkArgs._fields_]
    assert names == ["struct_bytes", "logits_dtype", "scoring", "renormalize", "rows", "experts", "top_k", "scale", "logits", "select_bias",
                     "ids", "weights", "stream"]
    assert ct.sizeof(ce.MoeTopkArgs) == 80 and ce.MoeTopkArgs.logits.offset == 40 and ce.MoeTopkArgs.stream.offset == 72
    decl = re.search(r"^int bnb_mi355x_moe_topk\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert decl and "bnb_stream_t" not in decl.group(1) and decl.group(1).strip() == "const bnb_mi355x_moe_topk_args* args"
    assert ce.lib.bnb_mi355x_moe_topk.restype is ct.c_int32 and len(ce.lib.bnb_mi355x_moe_topk_supported.argtypes) == 4


def _args(**over):
    """An argument block inside every precondition; the pointers are never dereferenced on the host (a refused call launches nothing)."""
    from bitsandbytes_amd.cextension import MoeTopkArgs

    keep = [(ct.c_float * 64)(), (ct.c_float * 8)(), (ct.c_int * 8)(), (ct.c_float * 8)()]
    a = MoeTopkArgs(ct.sizeof(MoeTopkArgs), 0, 0, 1, 4, 8, 2, 1.0, ct.addressof(keep[0]), ct.addressof(keep[1]), ct.addressof(keep[2]),
                    ct.addressof(keep[3]), None)
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = keep
    return a


REFUSALS = {
    "struct_bytes_small": dict(struct_bytes=72), "struct_bytes_large": dict(struct_bytes=88), "struct_bytes_zero": dict(struct_bytes=0),
    "null_logits": dict(logits=None), "null_ids": dict(ids=None), "null_weights": dict(weights=None),
    "dtype_low": dict(logits_dtype=-1), "dtype_high": dict(logits_dtype=3), "scoring_low": dict(scoring=-1), "scoring_high": dict(scoring=2),
    "experts_zero": dict(experts=0), "experts_negative": dict(experts=-8), "experts_1025": dict(experts=1025),
    "top_k_zero": dict(top_k=0), "top_k_17": dict(experts=64, top_k=17), "top_k_above_experts": dict(experts=8, top_k=9),
    "rows_negative": dict(rows=-1),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_non_zero_without_a_device(name, capfd):
    lib = _bnb().lib
    a = _args(**REFUSALS[name])
    assert lib.bnb_mi355x_moe_topk(ct.byref(a)) != 0
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and err.startswith("bitsandbytes_amd: moe_topk: "), err


def test_misaligned_pointers_and_a_null_block_are_refused_and_no_rows_is_not(capfd):
    lib = _bnb().lib
    for field in ("logits", "ids", "weights", "select_bias"):
        a = _args()
        setattr(a, field, getattr(a, field) + 1)
        assert lib.bnb_mi355x_moe_topk(ct.byref(a)) != 0, field
    assert lib.bnb_mi355x_moe_topk(None) != 0
    capfd.readouterr()
    # rows == 0: 0, nothing launched (no device here: a launch would not return 0), with or without pointers
    assert lib.bnb_mi355x_moe_topk(ct.byref(_args(rows=0))) == 0
    assert lib.bnb_mi355x_moe_topk(ct.byref(_args(rows=0, logits=None, ids=None, weights=None, select_bias=None))) == 0
    assert capfd.readouterr().err == ""
    # ... but not past a refusal
    assert lib.bnb_mi355x_moe_topk(ct.byref(_args(rows=0, experts=1025))) != 0


def test_predicate_edges():
    """bnb_mi355x_moe_topk_supported at E in {0, 1, 1024, 1025} and S in {0, 1, 16, 17, E + 1}: pure host logic."""
    sup = _bnb().lib.bnb_mi355x_moe_topk_supported
    for dt in (0, 1, 2):
        for rows in (1, 4, 16, 37, 4096):
            for E in (0, 1, 1024, 1025):
                for S in sorted({0, 1, 16, 17, E + 1}):
                    want = int(1 <= E <= 1024 and 1 <= S <= min(E, 16))
                    assert sup(dt, rows, E, S) == want, (dt, rows, E, S)
    assert sup(2, 1, 60, 8) == 1 and sup(2, 1, 8, 8) == 1 and sup(2, 1, 8, 9) == 0 and sup(2, 1, 16, 17) == 0
    assert sup(3, 1, 64, 2) == 0 and sup(-1, 1, 64, 2) == 0 and sup(2, 0, 64, 2) == 0 and sup(2, -1, 64, 2) == 0
    from bitsandbytes_amd.backends import hip

    assert hip.moe_topk_supported(torch.bfloat16, 1, 256, 8) and hip.moe_topk_supported(torch.float32, 16, 8, 2)
    assert hip.moe_topk_supported(torch.float16, 37, 1024, 16)
    assert not hip.moe_topk_supported(torch.float64, 1, 256, 8) and not hip.moe_topk_supported(torch.bfloat16, 1, 1025, 8)
    assert not hip.moe_topk_supported(torch.bfloat16, 1, 64, 17) and not hip.moe_topk_supported(torch.bfloat16, 2 ** 31, 64, 2)


# ------------------------------------------------------------------------------------------ op schema, fake kernel
def test_public_surface():
    bnb = _bnb()
    assert str(_op()._schema) == ("bitsandbytes_amd::moe_topk(Tensor logits, int top_k, str scoring, bool renormalize, float scale, "
                                  "Tensor? select_bias=None) -> (Tensor, Tensor)")
    for name in ("moe_topk", "moe_route"):
        assert callable(getattr(bnb, name)) and name in bnb.__all__
    assert "MoERouter" in bnb.nn.__all__
    p = inspect.signature(bnb.moe_topk).parameters
    assert list(p) == ["logits", "top_k", "scoring", "renormalize", "scale", "select_bias"]
    assert (p["scoring"].default, p["renormalize"].default, p["scale"].default, p["select_bias"].default) == ("softmax", True, 1.0, None)
    p = inspect.signature(bnb.moe_route).parameters
    assert list(p) == ["x", "router_weight", "top_k", "bias", "scoring", "renormalize", "scale", "select_bias", "return_logits"]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[3:]) and p["return_logits"].default is False
    p = inspect.signature(bnb.nn.MoERouter.__init__).parameters
    assert list(p)[:9] == ["self", "hidden", "num_experts", "top_k", "scoring", "renormalize", "scale", "bias", "select_bias"]
    assert p["bias"].default is False and p["select_bias"].default is False


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_fake_kernel_shapes_and_dtypes(dtype):
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        for E, S in ((8, 2), (60, 8), (1024, 16), (4096, 32), (1, 1)):
            logits = torch.empty((*lead, E), dtype=dtype, device="meta")
            for bias in (None, torch.empty(E, dtype=torch.float32, device="meta")):
                ids, w = _op()(logits, S, "sigmoid", True, 2.5, bias)
                assert ids.shape == w.shape == (*lead, S) and ids.dtype == torch.int32 and w.dtype == torch.float32
                assert ids.device.type == w.device.type == "meta" and ids.is_contiguous() and w.is_contiguous()


def test_fake_kernel_rejects_bad_arguments():
    logits = torch.empty((3, 64), dtype=torch.bfloat16, device="meta")
    f32 = torch.empty(64, dtype=torch.float32, device="meta")
    for match, args in (("scoring must be", (logits, 2, "tanh", True, 1.0)), ("top_k must be", (logits, 0, "softmax", True, 1.0)),
                        ("top_k must be", (logits, 65, "softmax", True, 1.0)), ("16/32-bit float", (logits.to(torch.int32), 2, "softmax", True, 1.0)),
                        ("contiguous", (logits[:, ::2], 2, "softmax", True, 1.0)), ("select_bias must be", (logits, 2, "softmax", True, 1.0, f32[:32])),
                        ("select_bias must be", (logits, 2, "softmax", True, 1.0, f32.bfloat16()))):
        with pytest.raises(RuntimeError, match=match):
            _op()(*args)


# ------------------------------------------------------------------------------------------ the cases and the composition
def test_the_grid_is_covered_pairwise():
    assert C.CASES == C.pairwise() and len({c.name for c in C.CASES}) == len(C.CASES) == 61
    # the 29 cases of the first grid lead, in their order; every later case holds one of the later expert counts
    assert all(c.E in C.FIRST_ES for c in C.CASES[:29]) and all(c.E in C.LATER_ES for c in C.CASES[29:])
    first = [c.name for c in C.CASES[:29]]
    assert (first[0], first[28]) == ("E1-S1-T1-float32-softmax-renorm-nobias", "E8-S1-T1-float32-softmax-renorm-nobias")
    assert hashlib.sha256("\n".join(first).encode()).hexdigest()[:16] == "d563656429d4b8f8", "the first 29 cases changed"
    covered = set()
    for c in C.CASES:
        assert c.S <= c.E and c.E in C.ES and c.S in C.SS and c.T in C.TS
        covered |= {(a, c[a], b, c[b]) for a in range(7) for b in range(a + 1, 7)}
    assert covered == C.all_pairs()
    # what a pair cover promises: every value of every axis, and the corners the kernel's structure names
    assert {c.E for c in C.CASES} == set(C.ES) and {c.dtype for c in C.CASES} == set(C.DTYPES)
    assert any(c.E == 1024 and c.S == 16 for c in C.CASES) and any(c.E == 60 and c.T == 37 for c in C.CASES)


def test_every_template_instance_is_launched_with_both_scorings_and_all_dtypes():
    """moe_topk_kernel<T, NI> exists for NI = 1, 2, 4, 8, 16 experts per lane; the case list reaches each of them with both scorings
    and with all three logits dtypes, at the first and the last E of the instance where the grid holds one."""
    assert [C.lane_slots(E) for E in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert {C.lane_slots(c.E) for c in C.CASES} == {1, 2, 4, 8, 16}
    for ni in (1, 2, 4, 8, 16):
        mine = [c for c in C.CASES if C.lane_slots(c.E) == ni]
        assert {c.scoring for c in mine} == set(C.SCORINGS) and {c.dtype for c in mine} == set(C.DTYPES), ni
        assert {c.renormalize for c in mine} == {True, False} and {c.bias for c in mine} == {True, False}, ni


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_rankings_are_unambiguous_and_the_composition_agrees_with_float64(case):
    """The builder's promise, asserted in float64 for every row (none dropped); then the public function on CPU tensors - the torch
    composition - against the float64 restatement: ids exactly, weights to fp32 rounding."""
    b = C.build(case)
    assert b.logits.shape == (case.T, case.E) and b.logits.dtype == case.dtype
    gap = C.assert_unambiguous(b.logits, case.scoring, b.bias)
    assert gap > C.KEY_GAP
    if case.E > C.HI_COUNT:
        assert all(len(torch.unique(row)) < case.E for row in b.logits), "planted ties"
    assert b.ids.dtype == torch.int32 and all(len(set(r.tolist())) == case.S for r in b.ids) and bool(((b.ids >= 0) & (b.ids < case.E)).all())
    with torch.no_grad():
        ids, w = _bnb().moe_topk(b.logits, case.S, case.scoring, case.renormalize, case.scale, b.bias)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (case.T, case.S)
    assert torch.equal(ids, b.ids)
    assert C.max_rel_err(w, b.weights) <= C.WEIGHT_FLOOR   # (16 fp32 ulps: the cases module's estimate for |l - max| <= 8)
    if case.renormalize:
        assert torch.allclose(w.sum(-1), torch.full((case.T,), case.scale), rtol=1e-6)
    if case.bias:   # the bias reorders: an expert with +1 leads although its score is not the largest
        assert bool((b.bias[b.ids[:, 0].long()] == 1).all())


def test_composition_tie_and_nan_rules():
    """Equal keys: the lower index. A NaN key: behind every other key, -inf included; NaN keys among themselves by index. The
    reference of the cases module states the same rule."""
    bnb = _bnb()
    nan, inf = float("nan"), float("inf")
    l = torch.tensor([[0.5, 2.0, 2.0, -1.0, 2.0, 0.5]])
    ids, w = bnb.moe_topk(l, 5, "sigmoid", False)
    assert ids.tolist() == [[1, 2, 4, 0, 5]] and torch.equal(w, torch.sigmoid(l)[0, [1, 2, 4, 0, 5]].view(1, 5))
    l = torch.tensor([[nan, 1.0, nan, 3.0], [0.0, 0.0, 0.0, 0.0]])
    ids, w = bnb.moe_topk(l, 4, "sigmoid", False)
    assert ids.tolist() == [[3, 1, 0, 2], [0, 1, 2, 3]] and bool(torch.isnan(w[0, 2:]).all()) and not bool(torch.isnan(w[1]).any())
    ref_ids, _ = C.reference(l, 4, "sigmoid", False, 1.0, None)
    assert torch.equal(ref_ids, ids)
    # a NaN logit poisons a softmax row (every key NaN: ascending index), and only that row; -inf keys (a -inf bias) go before NaN keys
    l = torch.tensor([[1.0, nan, 3.0], [1.0, 2.0, 3.0]])
    ids, w = bnb.moe_topk(l, 2, "softmax", True)
    assert ids.tolist() == [[0, 1], [2, 1]] and bool(torch.isnan(w[0]).all()) and bool(torch.isfinite(w[1]).all())
    ids, _ = bnb.moe_topk(torch.tensor([[nan, 0.0, 1.0]]), 3, "sigmoid", False, select_bias=torch.tensor([0.0, -inf, 0.0]))
    assert ids.tolist() == [[2, 1, 0]]
    # a zero sum: what IEEE gives, no epsilon
    ids, w = bnb.moe_topk(torch.tensor([[-inf, -inf, -inf]]), 2, "sigmoid", True)
    assert ids.tolist() == [[0, 1]] and bool(torch.isnan(w).all())


def test_public_functions_check_their_arguments():
    bnb = _bnb()
    l = torch.zeros(3, 8)
    for exc, match, call in ((ValueError, "scoring", lambda: bnb.moe_topk(l, 2, "tanh")), (ValueError, "top_k", lambda: bnb.moe_topk(l, 9)),
                             (ValueError, "top_k", lambda: bnb.moe_topk(l, 0)), (ValueError, "select_bias", lambda: bnb.moe_topk(l, 2, select_bias=torch.zeros(4))),
                             (ValueError, "float tensor", lambda: bnb.moe_topk(l.long(), 2)),
                             (RuntimeError, "inference only", lambda: bnb.moe_topk(l.clone().requires_grad_(), 2)),
                             (ValueError, r"\[E, K\]", lambda: bnb.moe_route(torch.zeros(3, 16), torch.zeros(8, 32), 2)),
                             (ValueError, "bias must be", lambda: bnb.moe_route(torch.zeros(3, 16), torch.zeros(8, 16), 2, bias=torch.zeros(4))),
                             (RuntimeError, "inference only", lambda: bnb.moe_route(torch.zeros(3, 16).requires_grad_(), torch.zeros(8, 16), 2))):
        with pytest.raises(exc, match=match):
            call()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_moe_route_composes_on_cpu(dtype):
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
                ids, w, got = bnb.moe_route(x, W, S, bias=b, scoring="sigmoid", renormalize=True, scale=2.5, select_bias=sb, return_logits=True)
                assert torch.equal(got, logits) and ids.shape == w.shape == (*lead, S)
                want_ids, want_w = bnb.moe_topk(logits, S, "sigmoid", True, 2.5, sb)
                assert torch.equal(ids, want_ids) and torch.equal(w, want_w)
                assert len(bnb.moe_route(x, W, S, bias=b)) == 2


# ------------------------------------------------------------------------------------------ the module
def test_module_state_dict_round_trips_and_loads_a_linear_gate():
    bnb = _bnb()
    full = bnb.nn.MoERouter(32, 8, 2, scoring="sigmoid", renormalize=True, scale=2.5, bias=True, select_bias=True)
    assert list(full.state_dict()) == ["weight", "bias", "e_score_correction_bias"]
    assert full.weight.shape == (8, 32) and full.bias.shape == (8,) and full.e_score_correction_bias.dtype == torch.float32
    assert not any(p.requires_grad for p in full.parameters())
    plain = bnb.nn.MoERouter(32, 8, 2)
    assert list(plain.state_dict()) == ["weight"] and plain.bias is None and plain.e_score_correction_bias is None
    gate = torch.nn.Linear(32, 8, bias=False)
    plain.load_state_dict(gate.state_dict())
    assert torch.equal(plain.weight, gate.weight)
    gen = torch.Generator().manual_seed(9)
    sd = {"weight": torch.randn(8, 32, generator=gen), "bias": torch.randn(8, generator=gen),
          "e_score_correction_bias": torch.randint(-2, 3, (8,), generator=gen).float()}
    full.load_state_dict(sd)
    other = bnb.nn.MoERouter(32, 8, 2, scoring="sigmoid", renormalize=True, scale=2.5, bias=True, select_bias=True)
    other.load_state_dict(full.state_dict())
    assert all(torch.equal(other.state_dict()[k], v) for k, v in sd.items())
    x = torch.randn(5, 32, generator=gen)
    with torch.no_grad():
        ids, w = full(x)
        want = bnb.moe_route(x, sd["weight"], 2, bias=sd["bias"], scoring="sigmoid", renormalize=True, scale=2.5,
                             select_bias=sd["e_score_correction_bias"])
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and torch.equal(ids, want[0]) and torch.equal(w, want[1])
    # a dtype cast leaves the selection bias in fp32 with its values; a gate in fp32 under 16-bit activations is not rounded
    cast = copy.deepcopy(full).to(torch.bfloat16)
    assert cast.weight.dtype == cast.bias.dtype == torch.bfloat16 and cast.e_score_correction_bias.dtype == torch.float32
    assert torch.equal(cast.e_score_correction_bias, sd["e_score_correction_bias"]) and list(cast.state_dict()) == list(full.state_dict())
    assert copy.deepcopy(full).half().e_score_correction_bias.dtype == torch.float32
    with torch.no_grad():
        ids16, w16, logits = bnb.moe_route(x.bfloat16(), sd["weight"], 2, bias=sd["bias"], return_logits=True)
        assert logits.dtype == torch.float32 and torch.equal(logits, torch.nn.functional.linear(x.bfloat16().float(), sd["weight"], sd["bias"]))
        assert torch.equal(bnb.moe_route(x.bfloat16(), sd["weight"], 2, return_logits=True)[2], torch.nn.functional.linear(x.bfloat16().float(), sd["weight"]))
    with pytest.raises(ValueError, match="scoring"):
        bnb.nn.MoERouter(32, 8, 2, scoring="tanh")
    with pytest.raises(ValueError, match="top_k"):
        bnb.nn.MoERouter(32, 8, 9)
