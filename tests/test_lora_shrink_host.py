"""CPU (-m "not gpu"): the host side of the LoRA shrink kernel (bitsandbytes_amd::lora_shrink, bitsandbytes_amd.lora_shrink,
nn.Linear4bitLoRA.fused_shrink) - C ABI, predicate, op schema / fake kernel, the composition on CPU tensors - and the preconditions of
every case tests/test_gpu_lora_shrink.py runs: the exact-sum bound of the exact inputs."""
import ctypes as ct
import fnmatch
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import lora_shrink_cases as C
from conftest import ROOT

SYMBOLS = ("bnb_mi355x_lora_shrink", "bnb_mi355x_lora_shrink_supported")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.lora_shrink.default


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
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/bnb_mi355x.h"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), f"{name} is not covered by exports.map"
        assert name in ce.EXPORTED_SYMBOLS
        assert hasattr(dll, name), f"{name} is not exported"
    assert len(ce.lib.bnb_mi355x_lora_shrink.argtypes) == 10 and ce.lib.bnb_mi355x_lora_shrink.restype is None
    assert len(ce.lib.bnb_mi355x_lora_shrink_supported.argtypes) == 4
    assert ce.lib.bnb_mi355x_version() == b"bitsandbytes_amd 0.1.1 gfx950"
    assert "lora_shrink.hip" in open(os.path.join(ROOT, "bitsandbytes_amd", "csrc", "Makefile")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS) and "splits" in notes


def test_public_functions_exist():
    bnb = _bnb()
    assert callable(bnb.lora_shrink) and "lora_shrink" in bnb.__all__
    assert list(inspect.signature(bnb.lora_shrink).parameters) == ["x", "lora_A", "splits"]
    assert inspect.signature(bnb.lora_shrink).parameters["splits"].default is None
    assert str(_op()._schema) == "bitsandbytes_amd::lora_shrink(Tensor x, Tensor lora_a, int[]? splits=None) -> Tensor"
    assert list(inspect.signature(bnb.nn.Linear4bitLoRA.forward).parameters) == ["self", "x", "t"]
    assert inspect.signature(bnb.nn.Linear4bitLoRA.forward).parameters["t"].default is None


def test_predicate_is_host_logic():
    """Answers without a device; 0 outside each precondition, 1 on the committed MUST_SERVE list (the classes the measurements keep)."""
    sup = _bnb().lib.bnb_mi355x_lora_shrink_supported
    for cell in C.MUST_REFUSE:
        assert sup(*cell) == 0, cell
    assert C.MUST_SERVE, "the list of served classes is empty"
    for ms, rs, ks in C.MUST_SERVE:
        for dt in (1, 2):
            for M in ms:
                for R in rs:
                    for K in ks:
                        assert sup(dt, M, R, K) == 1, (dt, M, R, K)
    for ms, rs, ks in C.EXCLUDED:
        for M in ms:
            for R in rs:
                for K in ks:
                    assert sup(1, M, R, K) == 0 and sup(2, M, R, K) == 0, (M, R, K)
    from bitsandbytes_amd.backends import hip

    ms, rs, ks = C.MUST_SERVE[0]
    assert hip.lora_shrink_supported(torch.bfloat16, ms[0], rs[0], ks[0]) and hip.lora_shrink_supported(torch.float16, ms[0], rs[0], ks[0])
    assert not hip.lora_shrink_supported(torch.float32, ms[0], rs[0], ks[0]) and not hip.lora_shrink_supported(torch.float64, ms[0], rs[0], ks[0])
    assert not hip.lora_shrink_supported(torch.bfloat16, 17, rs[0], ks[0]) and not hip.lora_shrink_supported(torch.bfloat16, ms[0], 12, ks[0])
    assert hip.lora_shrink_splits_ok(None) and hip.lora_shrink_splits_ok((8,) * 8) and hip.lora_shrink_splits_ok((8, 128, 24))
    assert not hip.lora_shrink_splits_ok((8,) * 9) and not hip.lora_shrink_splits_ok((136,)) and not hip.lora_shrink_splits_ok((12, 12))
    assert not hip.lora_shrink_splits_ok(())


# ------------------------------------------------------------------------------------------ fake kernel, argument checks
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_fake_kernel_shapes_and_strides(dtype):
    K, R = 128, 48
    a = torch.empty((R, K), dtype=dtype, device="meta")
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        x = torch.empty((*lead, K), dtype=dtype, device="meta")
        M = x.numel() // K
        t = _op()(x, a)
        assert t.shape == (*lead, R) and t.dtype == dtype and t.device.type == "meta" and t.is_contiguous()
        flat = _op()(x, a, [16, 8, 24])
        assert flat.shape == (M * R,) and flat.stride() == (1,) and flat.dtype == dtype
        parts = C.parts_of(flat, M, (16, 8, 24))
        assert [tuple(p.shape) for p in parts] == [(M, 16), (M, 8), (M, 24)] and all(p.is_contiguous() for p in parts)
        assert [p.storage_offset() for p in parts] == [0, M * 16, M * 24]


def test_fake_kernel_rejects_bad_arguments():
    m = "meta"
    x = torch.empty((3, 128), dtype=torch.bfloat16, device=m)
    a = torch.empty((48, 128), dtype=torch.bfloat16, device=m)
    for match, args in (("lora_a must be", (x, a.view(-1))), ("inner dim", (x[:, :64].contiguous(), a)), ("lora_a must be a", (x, a.half())),
                        ("contiguous", (x, a.t().contiguous().t())), ("contiguous", (x[:, ::2], a[:, ::2])),
                        ("16/32-bit float", (x.to(torch.int32), a.to(torch.int32))), ("sum to R", (x, a, [16, 16])), ("sum to R", (x, a, [48, 0])),
                        ("row counts", (x, a, [8, 8, 8, 8, 8, 8])[:2] + ([4] * 12,)), ("row counts", (x, a, []))):
        with pytest.raises(RuntimeError, match=match):
            _op()(*args)


# ------------------------------------------------------------------------------------------ the public function on CPU tensors
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_public_function_composes_on_cpu(dtype):
    bnb = _bnb()
    gen = torch.Generator().manual_seed(3)
    K = 128
    a = (torch.randn(48, K, generator=gen) / K ** 0.5).to(dtype)
    with torch.no_grad():
        for lead in ((1,), (4,), (2, 3), (17,)):
            x = torch.randn(*lead, K, generator=gen).to(dtype)
            want = TF.linear(x, a)
            got = bnb.lora_shrink(x, a)
            assert got.shape == (*lead, 48) and torch.equal(got, want)
            parts = bnb.lora_shrink(x, a, splits=(16, 8, 24))
            assert isinstance(parts, tuple) and len(parts) == 3
            for p, w in zip(parts, want.split((16, 8, 24), dim=-1)):
                assert p.shape == w.shape and p.is_contiguous() and torch.equal(p, w)
        # (any split the composition can cut, not only the kernel's multiples of 8)
        assert [tuple(p.shape) for p in bnb.lora_shrink(x, a, splits=(5, 43))] == [(17, 5), (17, 43)]
    with pytest.raises(ValueError, match="sum to"):
        bnb.lora_shrink(x, a, splits=(16, 16))
    with pytest.raises(ValueError, match=r"\[R, K\]"):
        bnb.lora_shrink(x, a[:, :64])
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.lora_shrink(x.float().requires_grad_(), a.float())


def test_fused_shrink_defaults_to_false():
    src = inspect.getsource(_bnb().nn.Linear4bitLoRA.__init__)
    assert "self.fused_shrink = False" in src

    class Base:   # (from_linear needs a quantized layer on a device: the constructor alone is host logic)
        pass

    mod = _bnb().nn.Linear4bitLoRA(Base(), torch.zeros(8, 64), torch.zeros(32, 8), 1.0)
    assert mod.fused_shrink is False
    mod.fused_shrink = True
    assert mod.fused_shrink is True and "fused_shrink" not in mod.state_dict()


# ------------------------------------------------------------------------------------------ preconditions of the exact GPU cases
def test_grid_covers_what_it_names():
    by_k = {K: [c for c in C.CASES if c.K == K] for K in C.KS}
    for K, cs in by_k.items():
        assert len({c.R for c in cs if c.splits is None}) >= 3 and {c.dtype for c in cs} == set(C.DTYPES)
        assert {c.splits for c in cs if c.splits} == set(C.SPLITS)
        assert (C.R_CAP in {c.R for c in cs}) == (K in C.R_CAP_KS)
    assert {c.R for c in C.CASES if c.splits is None} == set(C.RS) | {C.R_CAP}
    assert len({c.name for c in C.CASES}) == len(C.CASES)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_inputs_are_exact(case):
    """Every fp32 partial sum of the case is exact in any order (exact_inputs.assert_exact_sums with unit 2^-6), so float64 rounded once
    is the only right answer; and the answer is not trivial: distinct rows on both sides, results that differ."""
    x, a = C.build(case)
    assert x.shape == (C.MAX_ROWS, case.K) and a.shape == (case.R, case.K) and x.dtype == a.dtype == case.dtype
    worst = X.assert_exact_sums(a, x, C.UNIT, case.dtype)
    assert worst <= case.K / 2 and 32 * case.K < 2 ** 24
    assert set(torch.unique(a.float()).tolist()) <= set(C.A_VALUES)
    assert torch.unique(x, dim=0).shape[0] == C.MAX_ROWS and torch.unique(a, dim=0).shape[0] == case.R
    want = C.reference(x, a)
    assert bool(torch.isfinite(want.float()).all())
    if case.K > 64:
        assert torch.unique(want.float(), dim=0).shape[0] == C.MAX_ROWS and torch.unique(want.float().t(), dim=0).shape[0] == case.R
    # float64 is itself exact here: an fp32 matmul of the same operands agrees before the rounding
    assert torch.equal((x.float() @ a.float().t()).double(), x.double() @ a.double().t())
