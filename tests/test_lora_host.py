"""CPU (-m "not gpu"): the host side of the LoRA epilogue (bitsandbytes_amd::gemm_4bit_lora, matmul_4bit_lora, nn.Linear4bitLoRA) -
C ABI, route predicate, op schema / fake kernel, the module - and the preconditions of every case tests/test_gpu_lora.py runs: the
exact-sum bounds of base and adapter, the share of outputs whose adapter term is not zero, and the tolerance formula of the
ordinary-data test against a float32 emulation of the contract."""
import ctypes as ct
import fnmatch
import functools
import inspect
import os
import re

import pytest
import torch

import _oracle_cpu_backend
import exact_inputs as X
import lora_cases as C
from conftest import ROOT

SYMBOLS = ("bnb_mi355x_gemm_4bit_lora", "bnb_mi355x_gemm_4bit_lora_supported")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_lora.default


@functools.lru_cache(maxsize=None)
def _built(case):
    return C.build_case(case)


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
    assert len(ce.lib.bnb_mi355x_gemm_4bit_lora.argtypes) == 19 and ce.lib.bnb_mi355x_gemm_4bit_lora.argtypes[11] is ct.c_float
    assert len(ce.lib.bnb_mi355x_gemm_4bit_lora_supported.argtypes) == 7
    assert ce.lib.bnb_mi355x_version() == b"bitsandbytes_amd 0.1.1 gfx950"
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS) and "LoRA adapters" in notes and "from_linear" in notes


def test_public_functions_exist():
    bnb = _bnb()
    assert callable(bnb.matmul_4bit_lora) and "matmul_4bit_lora" in bnb.__all__
    assert list(inspect.signature(bnb.matmul_4bit_lora).parameters) == ["x", "weight", "quant_state", "lora_t", "lora_b", "scaling", "bias"]
    assert "Linear4bitLoRA" in bnb.nn.__all__
    assert list(inspect.signature(bnb.nn.Linear4bitLoRA.from_linear).parameters) == ["base", "lora_A", "lora_B", "scaling"]
    assert str(_op()._schema) == ("bitsandbytes_amd::gemm_4bit_lora(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, "
                                  "str quant_type, Tensor lora_t, Tensor lora_b, float scaling, Tensor? bias=None, "
                                  "Tensor? absmax_8bit=None, Tensor? absmax_code=None, Tensor? absmax_offset=None) -> Tensor")


def test_lora_supported_is_host_logic():
    """Answers without a device (256 CUs assumed); 1 on every cell the GPU test expects a kernel for, 0 outside the form."""
    sup = _bnb().lib.bnb_mi355x_gemm_4bit_lora_supported
    route = _bnb().lib.bnb_mi355x_gemm_4bit_route
    for (N, K, bs), ms in C.MUST_SERVE:
        for dt in (1, 2):
            for nested in (0, 1):
                for r in C.RANKS:
                    for M in ms:
                        assert sup(dt, M, N, K, bs, nested, r) == 1, (dt, M, N, K, bs, nested, r)
    for M in (1, 2, 8, 16):
        for nested in (0, 1):
            assert sup(2, M, 4096, 4096, 64, nested, 16) == 1
            assert sup(0, M, 4096, 4096, 64, nested, 16) == 0                   # fp32 activations
            assert sup(2, M, 4096, 4096, 32, nested, 16) == 0                   # blocksize 32
            assert sup(2, M, 4096, 4096, 64, nested, 12) == 0                   # r % 8 != 0
            assert sup(2, M, 4096, 4096, 64, nested, 136) == 0                  # r above the cap
            assert sup(2, M, 4096, 4096, 64, nested, 0) == 0
            assert sup(2, M, 4096, 4096 + 64, 128, nested, 16) == 0             # K % blocksize != 0
    assert sup(2, 17, 4096, 4096, 64, 0, 16) == 0 and sup(2, 0, 4096, 4096, 64, 0, 16) == 0 and sup(2, -1, 4096, 4096, 64, 0, 16) == 0
    assert sup(3, 1, 4096, 4096, 64, 0, 16) == 0 and sup(2, 1, 0, 4096, 64, 0, 16) == 0 and sup(2, 1, 4096, 0, 64, 0, 16) == 0
    # another kernel family (5 ... 8 rows of a small matrix with short rows: the register-transposed kernel) has no LoRA epilogue
    assert route(0, 2, 6, 2002, 1024, 64) == 1 and sup(2, 6, 2002, 1024, 64, 0, 16) == 0
    from bitsandbytes_amd.backends import hip

    assert hip.gemm_4bit_lora_supported(torch.bfloat16, 1, 4096, 4096, 64, True, 16)
    assert not hip.gemm_4bit_lora_supported(torch.float32, 1, 4096, 4096, 64, False, 16)
    assert not hip.gemm_4bit_lora_supported(torch.float64, 1, 4096, 4096, 64, False, 16)
    assert not hip.gemm_4bit_lora_supported(torch.bfloat16, 17, 4096, 4096, 64, False, 16)
    assert not hip.gemm_4bit_lora_supported(torch.bfloat16, 1, 4096, 4096, 64, False, 12)


# ------------------------------------------------------------------------------------------ fake kernel, argument checks
def _meta_args(N=96, K=128, bs=64, r=16, lead=(3,), dtype=torch.bfloat16):
    m = "meta"
    A = torch.empty((*lead, K), dtype=dtype, device=m)
    B = torch.empty((N * K // 2, 1), dtype=torch.uint8, device=m)
    absmax = torch.empty((N * K // bs,), dtype=torch.float32, device=m)
    t = torch.empty((*lead, r), dtype=dtype, device=m)
    b = torch.empty((N, r), dtype=dtype, device=m)
    return [A, B, [N, K], absmax, bs, "nf4", t, b, 0.5]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_fake_kernel_shapes(dtype):
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        y = _op()(*_meta_args(lead=lead, dtype=dtype))
        assert y.shape == (*lead, 96) and y.dtype == dtype and y.device.type == "meta"
    bias = torch.empty((96,), dtype=dtype, device="meta")
    assert _op()(*_meta_args(dtype=dtype), bias=bias).shape == (3, 96)
    assert _op()(*_meta_args(dtype=dtype, r=24)).shape == (3, 96)
    m = "meta"
    nested = dict(absmax_8bit=torch.empty((192,), dtype=torch.uint8, device=m), absmax_code=torch.empty((256,), dtype=torch.float32, device=m),
                  absmax_offset=torch.empty((), dtype=torch.float32, device=m))
    args = _meta_args(dtype=dtype)
    args[3] = torch.empty((1,), dtype=torch.float32, device=m)
    assert _op()(*args, **nested).shape == (3, 96)


def test_fake_kernel_rejects_bad_arguments():
    m = "meta"
    names = ["A", "B", "shapeB", "absmax", "blocksize", "quant_type", "lora_t", "lora_b", "scaling"]

    def bad(match, **change):
        args = _meta_args()
        kwargs = {k: change.pop(k) for k in ("bias", "absmax_8bit", "absmax_code", "absmax_offset") if k in change}
        for k, v in change.items():
            args[names.index(k)] = v
        with pytest.raises(RuntimeError, match=match):
            _op()(*args, **kwargs)

    bf = torch.bfloat16
    bad(r"lora_t must be \[\*, r\]", lora_t=torch.empty((3, 8), dtype=bf, device=m))
    bad(r"lora_t must be \[\*, r\]", lora_t=torch.empty((4, 16), dtype=bf, device=m))
    bad(r"lora_b must be \[N, r\]", lora_b=torch.empty((95, 16), dtype=bf, device=m))
    bad(r"lora_b must be \[N, r\]", lora_b=torch.empty((16, 96), dtype=bf, device=m))
    bad("must have A's dtype", lora_t=torch.empty((3, 16), dtype=torch.float16, device=m))
    bad("must have A's dtype", lora_b=torch.empty((96, 16), dtype=torch.float32, device=m))
    bad("contiguous", lora_t=torch.empty((16, 3), dtype=bf, device=m).t())
    bad("contiguous", lora_b=torch.empty((16, 96), dtype=bf, device=m).t())
    bad(r"\[N, K\]", shapeB=[2, 48, 128])
    bad("inner dim", A=torch.empty((3, 64), dtype=bf, device=m))
    bad("quant_type", quant_type="int4")
    bad("blocksize", blocksize=48)
    bad("float32", absmax=torch.empty((192,), dtype=torch.float16, device=m))
    bad("absmax must hold", absmax=torch.empty((191,), dtype=torch.float32, device=m))
    bad("4-bit values", B=torch.empty((96 * 64 - 1, 1), dtype=torch.uint8, device=m))
    bad("bias must be", bias=torch.empty((48,), dtype=bf, device=m))
    bad("bias must be", bias=torch.empty((96,), dtype=torch.float16, device=m))
    bad("16/32-bit float", A=torch.empty((3, 128), dtype=torch.float64, device=m))
    bad("together", absmax_8bit=torch.empty((192,), dtype=torch.uint8, device=m))
    bad("belong to nested", absmax_code=torch.empty((256,), dtype=torch.float32, device=m))


# ------------------------------------------------------------------------------------------ public function and module on the host
def _cpu_layer(i, o, bias, gen, nested=True):
    bnb = _bnb()
    layer = bnb.nn.Linear4bit(i, o, bias=bias, quant_type="nf4", compress_statistics=nested, compute_dtype=torch.bfloat16)
    W = (torch.randn(o, i, generator=gen) / i ** 0.5).bfloat16()
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=nested)
    layer.weight = bnb.nn.Params4bit.from_prequantized(packed, state.as_dict(packed=True), device="cpu", module=layer)
    if bias:
        layer.bias.data = torch.randn(o, generator=gen).bfloat16()
    return layer


def test_inference_only():
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(2)
    W = torch.randn(8, 64, generator=gen)
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4")
    x, t, b = torch.randn(2, 64, generator=gen), torch.randn(2, 8, generator=gen), torch.randn(8, 8, generator=gen)
    for grads in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
        xs, ts, bs_ = (v.clone().requires_grad_(g) for v, g in zip((x, t, b), grads))
        bias = torch.zeros(8, requires_grad=grads[3])
        with pytest.raises(RuntimeError, match="inference only"):
            bnb.matmul_4bit_lora(xs, packed, state, ts, bs_, 0.5, bias=bias)
    with pytest.raises(ValueError, match=r"\[N, r\]"):
        bnb.matmul_4bit_lora(x, packed, state, t, torch.randn(7, 8), 0.5)
    with pytest.raises(ValueError, match=r"\[N, r\]"):
        bnb.matmul_4bit_lora(x, packed, state, torch.randn(3, 8), b, 0.5)
    layer = _cpu_layer(64, 32, True, gen)
    mod = bnb.nn.Linear4bitLoRA.from_linear(layer, torch.randn(8, 64, generator=gen), torch.randn(32, 8, generator=gen), 2.0)
    with pytest.raises(RuntimeError, match="inference only"):
        mod(torch.randn(2, 64, requires_grad=True))
    with pytest.raises(ValueError, match="lora_A must be"):
        bnb.nn.Linear4bitLoRA.from_linear(layer, torch.randn(8, 32), torch.randn(32, 8), 2.0)


def test_cpu_composition_is_addmm_on_the_plain_matmul():
    """Off the device the public function is the composition: plain matmul_4bit, then torch.addmm with alpha = scaling."""
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(3)
    W = (torch.randn(24, 128, generator=gen) / 8).bfloat16()
    bias = torch.randn(24, generator=gen).bfloat16()
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4")
    for lead in ((3,), (2, 3)):
        x = torch.randn(*lead, 128, generator=gen).bfloat16()
        t = torch.randn(*lead, 8, generator=gen).bfloat16()
        b = torch.randn(24, 8, generator=gen).bfloat16()
        with torch.no_grad():
            y = bnb.matmul_4bit(x, packed, state, bias=bias)
            out = bnb.matmul_4bit_lora(x, packed, state, t, b, 0.25, bias=bias)
        assert out.shape == (*lead, 24) and out.dtype == torch.bfloat16
        assert torch.equal(out.reshape(-1, 24), torch.addmm(y.reshape(-1, 24), t.reshape(-1, 8), b.t(), alpha=0.25))


def test_module_holds_the_base_by_reference_and_stays_out_of_state_dicts():
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(5)
    K, N, r = 128, 96, 8
    for bias in (True, False):
        base = _cpu_layer(K, N, bias, gen)
        A = torch.randn(r, K, generator=gen) / K ** 0.5      # fp32 adapter, as PEFT stores it
        B_l = torch.randn(N, r, generator=gen) / 2
        mod = bnb.nn.Linear4bitLoRA.from_linear(base, A, B_l, 2.0)
        assert mod.base is base and mod.base.weight is base.weight and mod.base.weight.data_ptr() == base.weight.data_ptr()
        assert mod.state_dict() == {} and list(mod.parameters()) == []
        assert mod.lora_A.dtype == torch.bfloat16 and mod.lora_B.dtype == torch.bfloat16
        assert mod.lora_A.is_contiguous() and mod.lora_B.is_contiguous() and mod.scaling == 2.0
        assert tuple(mod.lora_A.shape) == (r, K) and tuple(mod.lora_B.shape) == (N, r)
        x = torch.randn(2, 3, K, generator=gen).bfloat16()
        with torch.no_grad():
            got = mod(x)
            t = torch.nn.functional.linear(x, A.bfloat16())
            want = bnb.matmul_4bit_lora(x, base.weight, base.weight.quant_state, t, B_l.bfloat16(), 2.0,
                                        bias=base.bias.detach() if bias else None)
            peft = base(x) + torch.nn.functional.linear(t, B_l.bfloat16()) * 2.0
        assert got.shape == (2, 3, N) and torch.equal(got, want)
        assert float((got.float() - peft.float()).abs().max()) <= 2.0 ** -6 * float(peft.float().abs().max())


# ------------------------------------------------------------------------------------------ preconditions of the GPU cases
def test_case_list():
    assert len(C.SHAPES) == 8 and C.EXCLUDED == ()
    assert len(C.CASES) == (len(C.SHAPES) + len(C.NESTED_SHAPES)) * len(C.DTYPES) == 24
    assert all(case.K % case.blocksize == 0 for case in C.CASES)
    assert all(s in C.SHAPES for s in C.NESTED_SHAPES)
    used = {r for case in C.CASES for r in case.ranks}
    assert used == set(C.RANKS) and all(len(set(case.ranks)) == 2 for case in C.CASES)
    assert all(r % 8 == 0 and 8 <= r <= 128 for r in C.RANKS)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_cases_are_exact_and_live(case):
    ex = _built(case)          # (asserts the exact-sum bound of the base: every fp32 partial sum is exact in any order)
    assert ex.x.shape == (C.MAX_ROWS, case.K) and ex.nested == case.nested
    base_worst = X.assert_exact_sums(ex.W, ex.x, ex.unit, case.dtype, extra=float(X.BIAS_MAX))
    y64 = ex.x.double() @ ex.W.double().t()
    for r, s in zip(case.ranks, C.SCALINGS):
        t, b = C.build_adapter(case, r)
        assert t.shape == (C.MAX_ROWS, r) and b.shape == (case.N, r) and t.dtype == case.dtype and b.dtype == case.dtype
        assert not bool(t.double().frac().any()) and float(t.abs().max()) <= C.T_MAX
        assert set(b.double().unique().tolist()) <= set(C.B_VALUES)
        # the adapter: every product a multiple of ADAPTER_UNIT, the sum of magnitudes within ADAPTER_MAX - exact in fp32 in any order
        mags = s * (t.double().abs().amax(dim=0) * b.double().abs()).sum(dim=1)
        assert float(mags.max()) <= C.ADAPTER_MAX and not bool((C.adapter_term64(t, b, s) / C.ADAPTER_UNIT).frac().any())
        # the total: multiples of the smaller unit, below 2^24 of them, and inside the fp16 range
        unit = min(ex.unit, C.ADAPTER_UNIT)
        assert (ex.unit / unit) % 1 == 0 and (C.ADAPTER_UNIT / unit) % 1 == 0
        total_worst = base_worst + float(mags.max())
        assert total_worst < 2.0 ** 24 * unit and (case.dtype != torch.float16 or total_worst < X.FP16_MAX), (case.name, r, total_worst)
        term = C.adapter_term64(t, b, s)
        for with_bias in (False, True):
            ref64 = y64 + term + (ex.bias.double() if with_bias else 0.0)
            ref = ref64.to(case.dtype)
            assert bool(torch.isfinite(ref).all()) and bool((ref.double() - ref64).abs().le(ref64.abs() * 2.0 ** -8 + 1e-30).all())
        live = float((term != 0).double().mean())
        print(f"{case.name} r={r} s={s}: base worst {base_worst:.1f}, adapter worst {float(mags.max()):.2f}, live {live:.3f}")
        assert live >= 0.9, (case.name, r, live)


# ------------------------------------------------------------------------------------------ the tolerance of the ordinary-data test
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
def test_tolerance_holds_for_a_float32_emulation_of_the_contract(dtype):
    """The bound of tests/test_gpu_lora.py (lora_cases.tolerance) against the contract computed in float32 on the CPU: a bound the
    reference arithmetic itself cannot meet would be no bound. 512 x 1024 NF4-scale weight, M = 16."""
    from oracle import oracle as O

    gen = torch.Generator().manual_seed(17)
    N, K, M = 512, 1024, 16
    W = (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype)
    packed, absmax = O.quantize_4bit(W, 64, "nf4")
    Wd = O.dequantize_4bit(packed, absmax, 64, "nf4", (N, K), torch.float32)
    x = torch.randn(M, K, generator=gen).to(dtype)
    bias = torch.randn(N, generator=gen).to(dtype)
    acc = x.float() @ Wd.t() + bias.float()                                      # fp32
    y = acc.to(dtype)                                                            # the plain op's output
    for r in (8, 24, 64, 128):
        A = (torch.randn(r, K, generator=gen) / K ** 0.5).to(dtype)
        b = (torch.randn(N, r, generator=gen) * 0.5).to(dtype)
        t = torch.nn.functional.linear(x, A)
        for s in (0.25, 0.5, 2.0):
            out = (acc + s * (t.float() @ b.float().t())).to(dtype)              # T((acc + bias) + s * lora), lora in fp32
            want = y.double() + C.adapter_term64(t, b, s)
            tol = C.tolerance(want, y, t, b, s, dtype)
            ratio = float(((out.double() - want).abs() / tol).max())
            comp = torch.addmm(y, t, b.t(), alpha=s)
            ratio_c = float(((comp.double() - want).abs() / tol).max())
            print(f"{dtype} r={r} s={s}: worst error / bound fused {ratio:.3f}, addmm {ratio_c:.3f}")
            assert ratio <= 1.0, (r, s, ratio)
            assert ratio_c <= 1.0, (r, s, ratio_c)   # (the composition's own arithmetic on the CPU: two roundings to T)
