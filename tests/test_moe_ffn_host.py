"""CPU (-m "not gpu"): the host side of the fused expert FFN (bitsandbytes_amd::gemm_4bit_experts_ffn, moe_ffn_4bit) - C ABI,
geometry query, op schema / fake kernel, argument checks - and the preconditions of every case tests/test_gpu_moe_ffn.py runs: the
exact-sum bound, lossless quantization, and the share of gate values in SiLU's live range."""
import ctypes as ct
import os
import re

import pytest
import torch

import exact_inputs as X
import moe_ffn_cases as C
from conftest import ROOT
from test_experts_host import ORACLE_OPS, _meta_args

SYMBOLS = ("bnb_mi355x_gemm_4bit_experts_ffn", "bnb_mi355x_gemm_4bit_experts_ffn_supported")
OLD_SCHEMA = ("bitsandbytes_amd::gemm_4bit_experts(Tensor A, Tensor B, int[] shapeB, Tensor absmax, Tensor ids, int blocksize, "
              "str quant_type, Tensor? bias=None, Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_exported_and_listed():
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    version_script = open(os.path.join(ROOT, "bitsandbytes_amd", "csrc", "exports.map")).read()
    assert "bnb_mi355x_*;" in version_script   # (the extensions are exported by prefix)
    assert ce.lib, f"{ce.LIB_PATH} not built"
    dll = ct.CDLL(str(ce.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/bnb_mi355x.h"
        assert name in ce.EXPORTED_SYMBOLS
        assert hasattr(dll, name), f"{name} is not exported"
        assert getattr(ce.lib, name).argtypes is not None
    assert len(ce.lib.bnb_mi355x_gemm_4bit_experts_ffn.argtypes) == 23
    assert len(ce.lib.bnb_mi355x_gemm_4bit_experts_ffn_supported.argtypes) == 6
    assert len(ce.lib.bnb_mi355x_gemm_4bit_experts.argtypes) == 20   # the old entry point keeps its signature
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS) and "moe_ffn_4bit" in notes
    assert ce.lib.bnb_mi355x_version().decode() == "bitsandbytes_amd 0.1.1 gfx950"


def test_public_functions_exist():
    import inspect

    bnb = _bnb()
    assert callable(bnb.moe_ffn_4bit) and "moe_ffn_4bit" in bnb.__all__
    assert callable(bnb.nn.parametrize.moe_ffn_4bit)
    sig = inspect.signature(bnb.moe_ffn_4bit)
    assert list(sig.parameters) == ["x", "gate_up", "gate_up_state", "down", "down_state", "expert_ids", "routing_weights",
                                    "gate_up_bias", "down_bias", "gated"]
    assert sig.parameters["gated"].default == "chunked"
    sig = inspect.signature(bnb.matmul_4bit_experts)
    for name, default in (("row_scale", None), ("gated", "none")):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default


def test_old_op_schema_is_unchanged():
    assert str(torch.ops.bitsandbytes_amd.gemm_4bit_experts.default._schema) == OLD_SCHEMA
    new = str(_op()._schema)
    assert new.startswith(OLD_SCHEMA.replace("gemm_4bit_experts(", "gemm_4bit_experts_ffn(").split(") -> ")[0])
    assert 'Tensor? row_scale=None, str gated="none") -> Tensor' in new


def test_ffn_supported_is_pure_host_logic():
    """Answers without a device; equals the old predicate without gating, refuses odd N when gated."""
    lib = _bnb().lib
    old, new = lib.bnb_mi355x_gemm_4bit_experts_supported, lib.bnb_mi355x_gemm_4bit_experts_ffn_supported
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    for case in C.CASES + C.EXCLUDED:
        for gated in (0, 1, 2):
            assert new(dt[case.dtype], case.E, case.N, case.K, case.blocksize, gated) == 1, case.name
    geometries = [(2, 8, 64, 4096, 64), (2, 8, 63, 4096, 64), (2, 8, 64, 4096 + 64, 128), (2, 8, 64, 4096, 16), (2, 8, 64, 4096 * 3, 96),
                  (2, 0, 64, 4096, 64), (2, 8, 0, 4096, 64), (2, 8, 64, 0, 64), (3, 8, 64, 4096, 64), (-1, 8, 64, 4096, 64),
                  (2, 8, 64, 1 << 20, 64), (2, 70000, 64, 4096, 64), (0, 128, 1536, 2048, 32), (1, 8, 28672, 4096, 64)]
    for g in geometries:
        assert new(*g, 0) == old(*g), g
        for gated in (1, 2):
            assert new(*g, gated) == (old(*g) if g[2] % 2 == 0 else 0), (g, gated)
    assert new(2, 8, 63, 4096, 64, 0) == 1 and new(2, 8, 63, 4096, 64, 1) == 0 and new(2, 8, 63, 4096, 64, 2) == 0
    assert new(2, 8, 64, 4096, 64, 3) == 0 and new(2, 8, 64, 4096, 64, -1) == 0        # unknown layout code
    from bitsandbytes_amd.backends import hip

    assert hip.gemm_4bit_experts_ffn_supported(torch.bfloat16, 8, 28672, 4096, 64, "chunked")
    assert not hip.gemm_4bit_experts_ffn_supported(torch.bfloat16, 8, 28671, 4096, 64, "interleaved")
    assert hip.gemm_4bit_experts_ffn_supported(torch.bfloat16, 8, 28671, 4096, 64, "none")
    assert not hip.gemm_4bit_experts_ffn_supported(torch.float64, 8, 28672, 4096, 64, "chunked")
    assert not hip.gemm_4bit_experts_ffn_supported(torch.bfloat16, 8, 28672, 4096, 64, "glu")


# ------------------------------------------------------------------------------------------ fake kernel, argument checks
@pytest.mark.parametrize("per_slot", [False, True], ids=["x_TK", "x_TSK"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_fake_kernel_shapes(per_slot, dtype, nested):
    args, kw = _meta_args(per_slot=per_slot, dtype=dtype, nested=nested)            # E 8, N 96, K 128, T 3, S 2
    bias = torch.empty((8, 96), dtype=dtype, device="meta")
    for gated in ("chunked", "interleaved"):
        y = _op()(*args, gated=gated, **kw)
        assert y.shape == (3, 2, 48) and y.dtype == dtype and y.device.type == "meta"
        assert _op()(*args, bias=bias, gated=gated, **kw).shape == (3, 2, 48)
    for sdt in (torch.float32, dtype):
        w = torch.empty((3, 2), dtype=sdt, device="meta")
        y = _op()(*args, row_scale=w, bias=bias, **kw)
        assert y.shape == (3, 2, 96) and y.dtype == dtype
    assert _op()(*args, **kw).shape == (3, 2, 96)                                   # neither: the old op's result
    args, kw = _meta_args(flat=True)
    assert _op()(*args, gated="chunked", **kw).shape == (6, 48)
    assert _op()(*args, row_scale=torch.empty((6,), dtype=torch.float32, device="meta"), **kw).shape == (6, 96)
    args, kw = _meta_args(T=0)
    assert _op()(*args, gated="interleaved", **kw).shape == (0, 2, 48)


def test_fake_kernel_rejects_bad_arguments():
    m = "meta"

    def bad(match=None, build=None, **extra):
        args, kw = _meta_args(**(build or {}))
        kw.update(extra)
        with pytest.raises(RuntimeError, match=match):
            _op()(*args, **kw)

    w32 = torch.empty((3, 2), dtype=torch.float32, device=m)
    bad("gated must be one of", gated="glu")
    bad("gated must be one of", gated="")
    bad("even number of weight rows", build=dict(N=97), gated="chunked")
    bad("even number of weight rows", build=dict(N=97), gated="interleaved")
    bad("cannot be given together", gated="chunked", row_scale=w32)
    bad("cannot be given together", gated="interleaved", row_scale=w32)
    bad("shape of ids", row_scale=torch.empty((3,), dtype=torch.float32, device=m))
    bad("shape of ids", row_scale=torch.empty((2, 3), dtype=torch.float32, device=m))
    bad("shape of ids", row_scale=torch.empty((3, 2, 1), dtype=torch.float32, device=m))
    bad("shape of ids", build=dict(flat=True), row_scale=w32)
    bad("row_scale must be float32 or", row_scale=torch.empty((3, 2), dtype=torch.float16, device=m))       # A is bf16
    bad("row_scale must be float32 or", row_scale=torch.empty((3, 2), dtype=torch.float64, device=m))
    bad("row_scale must be float32 or", row_scale=torch.empty((3, 2), dtype=torch.int32, device=m))
    bad("A's device", row_scale=torch.empty((3, 2), dtype=torch.float32, device="cpu"))
    # the shared checks of gemm_4bit_experts hold here too
    bad(None, bias=torch.empty((96,), dtype=torch.bfloat16, device=m))
    bad(None, bias=torch.empty((8, 48), dtype=torch.bfloat16, device=m), gated="chunked")                  # gated bias is [E, 2 I]
    args, kw = _meta_args()
    args[4] = torch.empty((3, 2), dtype=torch.int16, device=m)
    with pytest.raises(RuntimeError):
        _op()(*args, gated="chunked", **kw)
    args, kw = _meta_args()
    args[2] = [8, 128, 96]
    with pytest.raises(RuntimeError):
        _op()(*args, row_scale=w32, **kw)


def _state(shape, bs=64):
    F = _bnb().functional
    blocks = shape[0] * shape[1] * shape[2] // bs
    return F.QuantState(absmax=torch.empty(blocks, device="meta"), shape=torch.Size(shape), dtype=torch.bfloat16, blocksize=bs,
                        quant_type="nf4", code=torch.empty(16, device="meta"))


def test_public_functions_on_meta_tensors():
    """matmul_4bit_experts with the new keywords, and the whole block, shape-checked without a device."""
    bnb = _bnb()
    E, I, H, T, S = 8, 64, 128, 3, 2
    gu = torch.empty((E * 2 * I * H // 2, 1), dtype=torch.uint8, device="meta")
    dn = torch.empty((E * H * I // 2, 1), dtype=torch.uint8, device="meta")
    gu_state, dn_state = _state([E, 2 * I, H]), _state([E, H, I])
    ids = torch.empty((T, S), dtype=torch.int32, device="meta")
    w = torch.empty((T, S), dtype=torch.float32, device="meta")
    x = torch.empty((T, H), dtype=torch.bfloat16, device="meta")
    h = bnb.matmul_4bit_experts(x, gu, gu_state, ids, gated="interleaved")
    assert h.shape == (T, S, I)
    assert bnb.matmul_4bit_experts(h, dn, dn_state, ids, row_scale=w).shape == (T, S, H)
    assert bnb.matmul_4bit_experts(x, gu, gu_state, ids).shape == (T, S, 2 * I)
    y = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w)
    assert y.shape == (T, H) and y.dtype == torch.bfloat16
    y1 = bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids[:, :1], w[:, :1], gated="interleaved")
    assert y1.shape == (T, H)
    with pytest.raises(ValueError, match="gated must be"):
        bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w, gated="none")
    with pytest.raises(ValueError, match=r"\[T, S\]"):
        bnb.moe_ffn_4bit(x, gu, gu_state, dn, dn_state, ids, w[:, :1])
    with pytest.raises(RuntimeError, match="cannot be given together"):
        bnb.matmul_4bit_experts(x, gu, gu_state, ids, row_scale=w, gated="chunked")
    wg = torch.empty((T, S), dtype=torch.float32, device="meta", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_experts(x, gu, gu_state, ids, row_scale=wg)


# ------------------------------------------------------------------------------------------ cases
def test_case_list_shapes_dtypes_statistics_and_the_one_exclusion():
    names = [c.name for c in C.CASES]
    assert len(set(names)) == len(names) == 4 * 3 * 2 - 1
    assert {(c.E, c.N, c.K, c.blocksize) for c in C.CASES} == {(5, 144, 768, 64), (4, 96, 96, 32), (3, 64, 18432, 128), (8, 512, 1024, 64)}
    assert all(c.exps == (-8, -5) for c in C.CASES if not c.nested)
    assert C.P_VALUES == (1, 2, 5, 16, 65) and all(p in C.TS_OF_P for p in C.P_VALUES)
    missing = {(E, N, K, bs, d, n) for (E, N, K, bs) in C.SHAPES for d in C.DTYPES for n in (False, True)} - \
              {(c.E, c.N, c.K, c.blocksize, c.dtype, c.nested) for c in C.CASES}
    assert missing == {(3, 64, 18432, 128, torch.float16, True)}
    # ... which does not qualify for a tolerance-free comparison: exact_inputs' own range assertion
    with pytest.raises(AssertionError, match="fp16 range"):
        C.build_case(C.EXCLUDED[0])


def test_interleave_rows_is_the_layout_permutation():
    E, N = 3, 8
    flat = torch.arange(E * N * 2).view(E * N, 2)
    il = C.interleave_rows(flat, E, N).view(E, N, 2)
    ch = flat.view(E, N, 2)
    for i in range(N // 2):
        assert torch.equal(il[:, 2 * i], ch[:, i]) and torch.equal(il[:, 2 * i + 1], ch[:, N // 2 + i])


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_preconditions_of_the_gpu_cases(case):
    """The exact-sum bound over the rows actually used (with the bias); quantize / dequantize lose nothing, in both layouts, and the
    nested reconstruction is the intended scale (oracle); plain-statistics cases: at least half of the gate values lie where SiLU is
    neither the identity nor zero (2^-4 <= |g| <= 8), with and without the bias."""
    ex = C.build_case(case)
    X.assert_exact_sums(ex.W, ex.x, ex.unit, case.dtype, extra=float(X.BIAS_MAX))
    assert ex.W.shape == (case.E * case.N, case.K) and ex.x.shape == (C.MAX_ROWS, case.K) and ex.bias.shape == (case.E * case.N,)
    X.check_quantization(ex, ORACLE_OPS)
    if not case.nested:
        # (the interleaved stack of a plain case: the same blocks, rows permuted - the quantizer returns the permuted scales)
        Wi = C.interleave_rows(ex.W, case.E, case.N).contiguous()
        packed, absmax = ORACLE_OPS.quantize_4bit(Wi, case.blocksize)
        bpr = case.K // case.blocksize
        assert torch.equal(absmax.flatten(), C.interleave_rows(ex.scale.view(-1, bpr), case.E, case.N).reshape(-1))
        back = ORACLE_OPS.dequantize_4bit(packed, absmax, case.blocksize, tuple(Wi.shape), case.dtype)
        assert torch.equal(back.view(torch.uint8), Wi.view(torch.uint8))
    shares = C.live_share(ex, case, False), C.live_share(ex, case, True)
    print(f"{case.name}: share of gate values with 2^-4 <= |g| <= 8: {shares[0]:.3f} (no bias), {shares[1]:.3f} (bias)")
    if not case.nested:
        assert min(shares) >= 0.5, shares
