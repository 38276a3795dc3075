"""CPU (-m "not gpu"): the host side of mixed-adapter LoRA decode - the shrink (bitsandbytes_amd::lora_shrink_ids,
bitsandbytes_amd.lora_shrink_ids) and, in the second half of the file, the expand epilogue (bitsandbytes_amd::gemm_4bit_lora_ids,
matmul_4bit_lora_ids, nn.Linear4bitMultiLoRA): C ABI, predicates, op schemas / fake kernels, the gather compositions on CPU tensors,
from_adapters' padding - and the preconditions of every case tests/test_gpu_lora_multi.py runs: the exact-sum bound of the exact
inputs, the id patterns."""
import ctypes as ct
import fnmatch
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import _oracle_cpu_backend
import exact_inputs as X
import lora_cases as LC
import lora_multi_cases as C
import lora_shrink_cases as SC
from conftest import ROOT

SYMBOLS = ("bnb_mi355x_lora_shrink_ids", "bnb_mi355x_lora_shrink_ids_supported")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.lora_shrink_ids.default


def _ids(vals, dtype=torch.int32, device="cpu"):
    return torch.tensor(vals, dtype=dtype, device=device)


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
    assert len(ce.lib.bnb_mi355x_lora_shrink_ids.argtypes) == 13 and ce.lib.bnb_mi355x_lora_shrink_ids.restype is None
    assert len(ce.lib.bnb_mi355x_lora_shrink_ids_supported.argtypes) == 5
    assert ce.lib.bnb_mi355x_version() == b"bitsandbytes_amd 0.1.1 gfx950"
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS)


def test_public_function_exists():
    bnb = _bnb()
    assert callable(bnb.lora_shrink_ids) and "lora_shrink_ids" in bnb.__all__
    assert list(inspect.signature(bnb.lora_shrink_ids).parameters) == ["x", "lora_A", "adapter_ids", "splits"]
    assert inspect.signature(bnb.lora_shrink_ids).parameters["splits"].default is None
    assert str(_op()._schema) == "bitsandbytes_amd::lora_shrink_ids(Tensor x, Tensor lora_a, Tensor ids, int[]? splits=None) -> Tensor"


def test_predicate_is_host_logic():
    """Answers without a device. 0 outside each precondition; for every adapter count 1 wherever the uniform launch's preconditions
    hold - on lora_shrink_cases.MUST_SERVE and on the classes its measurements exclude (the ids launch replaces a gathered bmm, not
    F.linear: no class of it is excluded) - and 0 where the uniform predicate's preconditions fail."""
    sup = _bnb().lib.bnb_mi355x_lora_shrink_ids_supported
    uniform = _bnb().lib.bnb_mi355x_lora_shrink_supported
    for cell in C.MUST_REFUSE:
        assert sup(*cell) == 0, cell
    for A_n in (1, 17, 64):
        for ms, rs, ks in SC.MUST_SERVE + SC.EXCLUDED:
            for dt in (1, 2):
                for M in ms:
                    for R in rs:
                        for K in ks:
                            assert sup(dt, M, A_n, R, K) == 1, (dt, M, A_n, R, K)
        for dt, M, R, K in SC.MUST_REFUSE:
            assert uniform(dt, M, R, K) == 0 and sup(dt, M, A_n, R, K) == 0, (dt, M, A_n, R, K)
    for case in C.CASES:
        for M in C.MS:
            assert sup(C.DT_CODE[case.dtype], M, case.A_n, case.R, case.K) == 1, (case.name, M)
    from bitsandbytes_amd.backends import hip

    assert hip.lora_shrink_ids_supported(torch.bfloat16, 4, 17, 16, 4096) and hip.lora_shrink_ids_supported(torch.float16, 16, 64, 1024, 64)
    assert not hip.lora_shrink_ids_supported(torch.float32, 4, 17, 16, 4096) and not hip.lora_shrink_ids_supported(torch.bfloat16, 4, 65, 16, 4096)
    assert not hip.lora_shrink_ids_supported(torch.bfloat16, 17, 3, 16, 4096) and not hip.lora_shrink_ids_supported(torch.bfloat16, 4, 0, 16, 4096)


# ------------------------------------------------------------------------------------------ fake kernel, argument checks
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_fake_kernel_shapes_and_strides(dtype):
    K, R, A_n = 128, 48, 5
    a = torch.empty((A_n, R, K), dtype=dtype, device="meta")
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        x = torch.empty((*lead, K), dtype=dtype, device="meta")
        M = x.numel() // K
        for idt in (torch.int32, torch.int64):
            ids = torch.empty(lead, dtype=idt, device="meta")
            t = _op()(x, a, ids)
            assert t.shape == (*lead, R) and t.dtype == dtype and t.device.type == "meta" and t.is_contiguous()
            flat = _op()(x, a, ids, [16, 8, 24])
            assert flat.shape == (M * R,) and flat.stride() == (1,) and flat.dtype == dtype


def test_fake_kernel_rejects_bad_arguments():
    m = "meta"
    x = torch.empty((3, 128), dtype=torch.bfloat16, device=m)
    a = torch.empty((5, 48, 128), dtype=torch.bfloat16, device=m)
    ids = torch.empty((3,), dtype=torch.int32, device=m)
    for match, args in (("lora_a must be", (x, a[0], ids)), ("inner dim", (x[:, :64].contiguous(), a, ids)), ("lora_a must be a", (x, a.half(), ids)),
                        ("contiguous", (x, a.transpose(1, 2).contiguous().transpose(1, 2), ids)), ("int32 or int64", (x, a, ids.to(torch.int16))),
                        ("int32 or int64", (x, a, ids.float())), ("leading dims", (x, a, ids[:2])), ("leading dims", (x, a, ids.view(3, 1))),
                        ("at most 64", (x, torch.empty((65, 8, 128), dtype=torch.bfloat16, device=m), ids)),
                        ("16/32-bit float", (x.to(torch.int32), a.to(torch.int32), ids)), ("sum to R", (x, a, ids, [16, 16])),
                        ("row counts", (x, a, ids, [4] * 12)), ("row counts", (x, a, ids, []))):
        with pytest.raises(RuntimeError, match=match):
            _op()(*args)


# ------------------------------------------------------------------------------------------ the public function on CPU tensors
@pytest.mark.parametrize("case", [c for c in C.CASES if c.K <= 2048], ids=lambda c: c.name)
def test_cpu_composition_is_exact_on_exact_inputs(case):
    """On the exact inputs the gather composition equals float64 rounded once with each row's adapter and the per-row uniform
    composition (F.linear with that row's adapter), bit for bit; a row without an adapter is zeros."""
    bnb = _bnb()
    x, stack = C.build(case)
    with torch.no_grad():
        for M in C.MS:
            for name, vals, idt in C.patterns(M, case.A_n):
                ids = _ids(vals, idt)
                want = C.reference(x[:M], stack, vals)
                got = bnb.lora_shrink_ids(x[:M], stack, ids, splits=case.splits)
                if case.splits is not None:
                    assert isinstance(got, tuple) and all(p.is_contiguous() for p in got) and [p.shape[-1] for p in got] == list(case.splits)
                    got = torch.cat(got, dim=-1)
                assert got.shape == (M, case.R) and got.dtype == case.dtype
                assert torch.equal(got, want), (M, name, X.first_mismatch(got, want))
                for m, i in enumerate(vals):
                    row = TF.linear(x[m:m + 1], stack[i]) if 0 <= i < case.A_n else torch.zeros(1, case.R, dtype=case.dtype)
                    assert torch.equal(got[m:m + 1], row), (M, name, m)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_cpu_composition_on_ordinary_data(dtype):
    """Sums that round: inside lora_shrink_cases.tolerance of the float64 product with the row's adapter (fp32: far inside); leading
    dims, 17 rows, NaN in adapters no row names and poisoned rows of a row without an adapter do not reach the result."""
    bnb = _bnb()
    K, R, A_n = 256, 24, 5
    x, a = C.ordinary(17, A_n, R, K, dtype, 3)
    a[2] = float("nan")                                   # (no row below names adapter 2)
    vals = [0, 4, -1, 1, A_n, 3, 3, 0, 1, 4, -1, 0, 2 ** 32 + 1, 1, 3, 4, 0]
    ids = _ids(vals, torch.int64)
    with torch.no_grad():
        got = bnb.lora_shrink_ids(x, a, ids)
        assert got.shape == (17, R) and not bool(torch.isnan(got).any())
        for m, i in enumerate(vals):
            if 0 <= i < A_n:
                want = x[m:m + 1].double() @ a[i].double().t()
                assert bool(((got[m:m + 1].double() - want).abs() <= SC.tolerance(want, x[m:m + 1], a[i])).all()) or dtype == torch.float32
                if dtype == torch.float32:
                    assert torch.allclose(got[m:m + 1].double(), want, rtol=1e-5, atol=1e-5)
            else:
                assert torch.equal(got[m], torch.zeros(R, dtype=dtype))
        lead = bnb.lora_shrink_ids(x[:6].view(2, 3, K), a, ids[:6].view(2, 3))
        assert lead.shape == (2, 3, R) and torch.equal(lead.view(6, R), bnb.lora_shrink_ids(x[:6], a, ids[:6]))
        parts = bnb.lora_shrink_ids(x[:6], a, ids[:6].to(torch.int32), splits=(5, 19))
        assert [tuple(p.shape) for p in parts] == [(6, 5), (6, 19)] and all(p.is_contiguous() for p in parts)


def test_public_function_rejects_bad_arguments():
    bnb = _bnb()
    x, a = C.ordinary(4, 3, 16, 128, torch.bfloat16, 5)
    ids = _ids([0, 1, 2, -1])
    for exc, match, args, kw in ((ValueError, r"\[A_n, R, K\]", (x, a[0], ids), {}), (ValueError, r"\[A_n, R, K\]", (x[:, :64], a, ids), {}),
                                 (ValueError, "adapter_ids", (x, a, ids[:3]), {}), (ValueError, "adapter_ids", (x, a, ids.float()), {}),
                                 (ValueError, "1 ... 64", (x, a.repeat(22, 1, 1), ids), {}), (ValueError, "sum to", (x, a, ids), dict(splits=(8, 4))),
                                 (RuntimeError, "inference only", (x.float().requires_grad_(), a.float(), ids), {})):
        with pytest.raises(exc, match=match):
            bnb.lora_shrink_ids(*args, **kw)


# ------------------------------------------------------------------------------------------ preconditions of the exact GPU cases
def test_grid_covers_what_it_names():
    assert {c.A_n for c in C.CASES} == set(C.ADAPTER_COUNTS) and {c.K for c in C.CASES} == {64, 2048, 4096}
    assert {c.R for c in C.CASES if c.splits is None} == {8, 24, 128} and {c.dtype for c in C.CASES} == set(C.DTYPES)
    assert {c.splits for c in C.CASES if c.splits} == {(16, 16, 16), (8, 128, 24)}
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    for K in (64, 2048, 4096):
        assert len({c.A_n for c in C.CASES if c.K == K}) >= 3 and {c.dtype for c in C.CASES if c.K == K} == set(C.DTYPES)
    for A_n in C.ADAPTER_COUNTS:
        for M in C.MS:
            pats = {name: (vals, dt) for name, vals, dt in C.patterns(M, A_n)}
            assert all(len(v) == M for v, _ in pats.values())
            assert len(set(pats["same"][0])) == 1 and all(C.in_range(pats["same"][0], A_n))
            assert len(set(pats["distinct"][0])) == min(M, A_n) and all(C.in_range(pats["distinct"][0], A_n))
            assert set(pats["first_last"][0]) <= {0, A_n - 1} and pats["first_last"][0][0] == A_n - 1
            assert not any(C.in_range(pats["none"][0], A_n))
            assert pats["alias64"][1] == torch.int64 and pats["alias64"][0][0] == 2 ** 32 + 1 and pats["distinct64"][1] == torch.int64
            if M >= 4:
                assert {-1, A_n} <= set(pats["out_of_range"][0]) and any(C.in_range(pats["out_of_range"][0], A_n))
                assert len(set(pats["two"][0])) == min(2, A_n)
            # nothing wilder than the adjacent values and the alias of the low word
            assert all(-1 <= i <= A_n or i in (2 ** 32, 2 ** 32 + 1) for v, _ in pats.values() for i in v)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_inputs_are_exact(case):
    """Every fp32 partial sum is exact in any order for every adapter of the stack (exact_inputs.assert_exact_sums, unit 2^-6), the
    adapters differ, and so do the results: a row computed with a neighbour's adapter would be seen."""
    x, stack = C.build(case)
    assert x.shape == (C.MAX_ROWS, case.K) and stack.shape == (case.A_n, case.R, case.K) and x.dtype == stack.dtype == case.dtype
    worst = X.assert_exact_sums(stack.view(-1, case.K), x, C.UNIT, case.dtype)
    assert worst <= case.K / 2 and 32 * case.K < 2 ** 24
    assert set(torch.unique(stack.float()).tolist()) <= set(C.A_VALUES)
    if case.A_n > 1 and case.K > 64:
        full = torch.stack([C.reference(x, stack, [a] * C.MAX_ROWS).float() for a in range(min(case.A_n, 4))])
        assert torch.unique(full.view(full.shape[0], -1), dim=0).shape[0] == full.shape[0]
        assert all(not torch.equal(full[0][m], full[1][m]) for m in range(C.MAX_ROWS))


# ========================================================================================== expand: gemm_4bit_lora_ids
EXPAND_SYMBOLS = ("bnb_mi355x_gemm_4bit_lora_ids", "bnb_mi355x_gemm_4bit_lora_ids_supported")


def _eop():
    return torch.ops.bitsandbytes_amd.gemm_4bit_lora_ids.default


def test_expand_symbols_and_public_names():
    from bitsandbytes_amd import cextension as ce

    bnb = _bnb()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read(), flags=re.S)
    dll = ct.CDLL(str(ce.LIB_PATH))
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPAND_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in ce.EXPORTED_SYMBOLS and hasattr(dll, name) and name in notes, name
    assert len(ce.lib.bnb_mi355x_gemm_4bit_lora_ids.argtypes) == 22 and ce.lib.bnb_mi355x_gemm_4bit_lora_ids.restype is None
    assert len(ce.lib.bnb_mi355x_gemm_4bit_lora_ids_supported.argtypes) == 8
    assert callable(bnb.matmul_4bit_lora_ids) and "matmul_4bit_lora_ids" in bnb.__all__
    assert list(inspect.signature(bnb.matmul_4bit_lora_ids).parameters) == ["x", "weight", "quant_state", "lora_t", "lora_B", "scalings", "adapter_ids", "bias"]
    assert "Linear4bitMultiLoRA" in bnb.nn.__all__
    assert list(inspect.signature(bnb.nn.Linear4bitMultiLoRA.forward).parameters) == ["self", "x", "adapter_ids", "t"]
    assert str(_eop()._schema) == ("bitsandbytes_amd::gemm_4bit_lora_ids(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, str quant_type, "
                                   "Tensor lora_t, Tensor lora_b, Tensor scalings, Tensor ids, Tensor? bias=None, Tensor? absmax_8bit=None, "
                                   "Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor")


def test_expand_predicate_equals_the_uniform_predicate():
    """Pure host logic (256 CUs without a device): for A_n = 1, 17, 64 the ids predicate answers what
    bnb_mi355x_gemm_4bit_lora_supported answers - 1 on lora_cases.MUST_SERVE for every rank and both kinds of statistics, and the same
    as the uniform one over every shape of lora_cases at every M from 1 to 17 - and 0 outside 1 <= A_n <= 64."""
    lib = _bnb().lib
    ids_sup, sup = lib.bnb_mi355x_gemm_4bit_lora_ids_supported, lib.bnb_mi355x_gemm_4bit_lora_supported
    for A_n in (1, 17, 64):
        for (N, K, bs), ms in LC.MUST_SERVE:
            for M in ms:
                for nested in (0, 1):
                    for r in LC.RANKS:
                        for dt in (1, 2):
                            assert ids_sup(dt, M, N, K, bs, nested, r, A_n) == 1 == sup(dt, M, N, K, bs, nested, r), (N, K, bs, M, nested, r, A_n)
        for N, K, bs in LC.SHAPES:
            for M in LC.MS:
                for r in (8, 12, 24, 128, 136):
                    for dt in (0, 1, 2):
                        assert ids_sup(dt, M, N, K, bs, 0, r, A_n) == sup(dt, M, N, K, bs, 0, r), (N, K, bs, M, r, dt, A_n)
    assert [m for m in (5, 6, 7, 8) if ids_sup(2, m, 2002, 1024, 64, 0, 8, 3)] == []
    for A_n in (0, -1, 65):
        assert ids_sup(2, 1, 4096, 4096, 64, 0, 8, A_n) == 0


def test_expand_fake_kernel_and_argument_checks():
    m = "meta"
    N, K, r, A_n = 64, 128, 8, 5
    B = torch.empty((N * K // 2, 1), dtype=torch.uint8, device=m)
    absmax = torch.empty((N * K // 64,), dtype=torch.float32, device=m)
    stack = torch.empty((A_n, N, r), dtype=torch.bfloat16, device=m)
    sc = torch.empty((A_n,), dtype=torch.float32, device=m)
    for lead in ((3,), (2, 5), (0,), ()):
        x = torch.empty((*lead, K), dtype=torch.bfloat16, device=m)
        t = torch.empty((*lead, r), dtype=torch.bfloat16, device=m)
        for idt in (torch.int32, torch.int64):
            out = _eop()(x, B, [N, K], absmax, 64, "nf4", t, stack, sc, torch.empty(lead, dtype=idt, device=m))
            assert out.shape == (*lead, N) and out.dtype == torch.bfloat16 and out.device.type == m
    x = torch.empty((3, K), dtype=torch.bfloat16, device=m)
    t = torch.empty((3, r), dtype=torch.bfloat16, device=m)
    ids = torch.empty((3,), dtype=torch.int32, device=m)
    for match, args in (("lora_b must be", (t, stack[0], sc, ids)), ("1 ... 64", (t, torch.empty((65, N, r), dtype=torch.bfloat16, device=m), sc, ids)),
                        ("scalings must be", (t, stack, sc[:4], ids)), ("scalings must be", (t, stack, sc.bfloat16(), ids)),
                        ("int32 or int64", (t, stack, sc, ids.float())), ("leading dims", (t, stack, sc, ids[:2])),
                        ("lora_t must be", (t[:2], stack, sc, ids)), ("must have A's dtype", (t.half(), stack, sc, ids)),
                        ("lora_b must be", (t, torch.empty((A_n, N + 1, r), dtype=torch.bfloat16, device=m), sc, ids))):
        with pytest.raises(RuntimeError, match=match):
            _eop()(x, B, [N, K], absmax, 64, "nf4", *args)


def _cpu_layer(K, N, bias, gen, dtype=torch.bfloat16):
    bnb = _bnb()
    layer = bnb.nn.Linear4bit(K, N, bias=bias, quant_type="nf4", compress_statistics=False, compute_dtype=dtype)
    W = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dtype)
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=False)
    layer.weight = bnb.nn.Params4bit.from_prequantized(packed, state.as_dict(packed=True), device="cpu", module=layer)
    if bias:
        layer.bias.data = torch.randn(N, generator=gen).to(dtype)
    return layer


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_expand_cpu_composition(dtype):
    """Off the device matmul_4bit_lora_ids composes. On exact adapter operands (t integers, B_l from lora_cases.B_VALUES, scalings
    0.5 / 2) every row equals T(float(y[m]) + s_id t64 B_id64^T) - float64 rounded once, y the plain matmul_4bit row - and the per-row
    uniform composition matmul_4bit_lora with that row's adapter; a row without an adapter is the plain row, whatever its lora_t row
    and the unused adapters hold (NaN)."""
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(3)
    N, K, r, A_n = 24, 128, 8, 3
    W = (torch.randn(N, K, generator=gen) / 8).to(dtype)
    bias = torch.randint(-4, 5, (N,), generator=gen).to(dtype)
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4")
    values = torch.tensor(LC.B_VALUES)
    stack = values[torch.randint(0, len(LC.B_VALUES), (A_n, N, r), generator=gen)].to(dtype)
    sc = torch.tensor([0.5, 2.0, 0.5])
    stack[2] = float("nan")                                   # (no row below names adapter 2)
    for lead in ((6,), (2, 3)):
        x = torch.randint(-4, 5, (*lead, K), generator=gen).to(dtype)
        t = torch.randint(-4, 5, (*lead, r), generator=gen).to(dtype)
        vals = [1, -1, 0, A_n, 0, 2 ** 32 + 1]
        t.view(-1, r)[1] = float("nan")
        ids = _ids(vals, torch.int64).view(*lead)
        with torch.no_grad():
            y = bnb.matmul_4bit(x, packed, state, bias=bias).reshape(-1, N)
            out = bnb.matmul_4bit_lora_ids(x, packed, state, t, stack, sc, ids, bias=bias)
            assert out.shape == (*lead, N) and out.dtype == dtype and not bool(torch.isnan(out).any())
            out = out.reshape(-1, N)
            for m, i in enumerate(vals):
                if 0 <= i < A_n:
                    tm = t.view(-1, r)[m:m + 1]
                    want = (y[m:m + 1].double() + float(sc[i]) * (tm.double() @ stack[i].double().t())).to(dtype)
                    assert torch.equal(out[m:m + 1], want), (lead, m)
                    uniform = bnb.matmul_4bit_lora(x.reshape(-1, K)[m:m + 1], packed, state, tm, stack[i], float(sc[i]), bias=bias)
                    assert torch.equal(out[m:m + 1], uniform), (lead, m)
                else:
                    assert torch.equal(out[m], y[m]), (lead, m)
    with pytest.raises(ValueError, match=r"\[A_n, N, r\]"):
        bnb.matmul_4bit_lora_ids(x, packed, state, t, stack[0], sc, ids)
    with pytest.raises(ValueError, match="scalings"):
        bnb.matmul_4bit_lora_ids(x, packed, state, t, stack, sc[:2], ids)
    with pytest.raises(ValueError, match="adapter_ids"):
        bnb.matmul_4bit_lora_ids(x, packed, state, t, stack, sc, ids.view(-1))
    with pytest.raises(ValueError, match="adapter_ids"):
        bnb.matmul_4bit_lora_ids(x, packed, state, t, stack, sc, ids.float())
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_lora_ids(x.float().requires_grad_(), packed, state, t, stack, sc, ids)


def test_from_adapters_pads_to_a_multiple_of_eight():
    """Ranks 4, 12 and 9 are stacked at rank 16: rows of zeros behind lora_A_i, columns of zeros behind lora_B_i - equal in value to
    the unpadded adapter (the padded t columns are exact zeros). The module holds the base by reference and has no state."""
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(5)
    K, N = 128, 96
    base = _cpu_layer(K, N, True, gen)
    adapters = [(torch.randn(r, K, generator=gen) / K ** 0.5, torch.randn(N, r, generator=gen) / 2, s) for r, s in ((4, 2.0), (12, 0.5), (9, 1.25))]
    mod = bnb.nn.Linear4bitMultiLoRA.from_adapters(base, adapters)
    assert mod.base is base and mod.state_dict() == {} and list(mod.parameters()) == []
    assert tuple(mod.lora_A.shape) == (3, 16, K) and tuple(mod.lora_B.shape) == (3, N, 16) and mod.lora_A.dtype == mod.lora_B.dtype == torch.bfloat16
    assert mod.scalings.dtype == torch.float32 and mod.scalings.tolist() == [2.0, 0.5, 1.25]
    for i, (a, b, _) in enumerate(adapters):
        r = a.shape[0]
        assert torch.equal(mod.lora_A[i, :r], a.bfloat16()) and not bool(mod.lora_A[i, r:].any())
        assert torch.equal(mod.lora_B[i, :, :r], b.bfloat16()) and not bool(mod.lora_B[i, :, r:].any())
    x = torch.randn(2, 3, K, generator=gen).bfloat16()
    vals = [2, 0, -1, 1, 3, 0]
    ids = _ids(vals).view(2, 3)
    with torch.no_grad():
        got = mod(x, ids).view(6, N)
        plain = base(x).view(6, N)
        for m, i in enumerate(vals):
            if 0 <= i < 3:
                a, b, s = adapters[i]
                one = bnb.nn.Linear4bitLoRA.from_linear(base, a, b, s)(x.view(6, K)[m:m + 1])
                assert float((got[m:m + 1].float() - one.float()).abs().max()) <= 2.0 ** -6 * float(one.float().abs().max()), (m, i)
            else:
                assert torch.equal(got[m], plain[m])
        t = bnb.lora_shrink_ids(x, mod.lora_A, ids)
        assert torch.equal(mod(x, ids, t=t).view(6, N), got)
        p1, p2 = bnb.nn.Linear4bitMultiLoRA.shrink_group(x, [mod, mod], ids)
        assert torch.equal(p1, t) and torch.equal(p2, t)
    with pytest.raises(ValueError, match="every adapter"):
        bnb.nn.Linear4bitMultiLoRA.from_adapters(base, [(torch.zeros(4, K), torch.zeros(N, 8), 1.0)])
    with pytest.raises(ValueError, match="1 ... 64"):
        bnb.nn.Linear4bitMultiLoRA.from_adapters(base, [])
    with pytest.raises(RuntimeError, match="inference only"):
        mod(torch.randn(2, K, requires_grad=True), _ids([0, 1]))


def test_expand_case_list():
    shapes = {(c.base.N, c.base.K, c.base.blocksize) for c in C.EXPAND_CASES}
    assert shapes == set(C.EXPAND_STREAM) | set(C.EXPAND_SM) | set(C.EXPAND_OTHER)
    assert {c.r for c in C.EXPAND_CASES} == set(LC.RANKS) and {c.A_n for c in C.EXPAND_CASES} == {1, 3, 17}
    assert {c.base.dtype for c in C.EXPAND_CASES} == set(C.DTYPES)
    nested = {(c.base.N, c.base.K, c.base.blocksize) for c in C.EXPAND_CASES if c.base.nested}
    assert nested == set(LC.NESTED_SHAPES)
    for c in C.EXPAND_CASES:
        t, stack, sc = C.build_expand_adapters(c)
        assert t.shape == (C.MAX_ROWS, c.r) and stack.shape == (c.A_n, c.base.N, c.r) and sc.shape == (c.A_n,) and sc.dtype == torch.float32
        assert set(torch.unique(stack.float()).tolist()) <= set(LC.B_VALUES) and float(t.float().abs().max()) <= LC.T_MAX
        assert set(sc.tolist()) <= set(LC.SCALINGS)
        # every adapter product is a multiple of the adapter unit and the term stays inside lora_cases' bound: exact in any order
        assert float((sc.view(-1, 1, 1) * stack.float().abs()).sum(-1).max()) * LC.T_MAX <= LC.ADAPTER_MAX
        if c.A_n > 1:
            a = C.expand_reference(torch.zeros(C.MAX_ROWS, c.base.N, dtype=torch.float64), None, t, stack, sc, [0] * C.MAX_ROWS, torch.float32)
            b = C.expand_reference(torch.zeros(C.MAX_ROWS, c.base.N, dtype=torch.float64), None, t, stack, sc, [1] * C.MAX_ROWS, torch.float32)
            assert all(not torch.equal(a[m], b[m]) for m in range(C.MAX_ROWS))
