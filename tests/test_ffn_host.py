"""CPU (-m "not gpu"): the host side of the dense gated-SiLU FFN (bitsandbytes_amd::gemm_4bit_gated, matmul_4bit_gated, ffn_4bit,
nn.FFN4bit, functional.interleave_gate_up_4bit) - C ABI, route predicate, op schema / fake kernel, the layout helper against the
oracle - and the preconditions of every case tests/test_gpu_ffn.py runs: the exact-sum bound, lossless quantization and the share
of gate values in SiLU's live range."""
import ctypes as ct
import functools
import inspect
import os
import re

import pytest
import torch

import _oracle_cpu_backend
import exact_inputs as X
import ffn_cases as C
from conftest import ROOT
from oracle import oracle as O
from test_experts_host import ORACLE_OPS

SYMBOLS = ("bnb_mi355x_gemm_4bit_gated", "bnb_mi355x_gemm_4bit_gated_supported")


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_gated.default


@functools.lru_cache(maxsize=None)
def _built(case):
    return C.build_case(case)


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_exported_and_listed():
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert ce.lib, f"{ce.LIB_PATH} not built"
    dll = ct.CDLL(str(ce.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/bnb_mi355x.h"
        assert name in ce.EXPORTED_SYMBOLS
        assert hasattr(dll, name), f"{name} is not exported"
    assert len(ce.lib.bnb_mi355x_gemm_4bit_gated.argtypes) == 12
    assert len(ce.lib.bnb_mi355x_gemm_4bit_gated_supported.argtypes) == 5
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS) and "Dense FFN" in notes and "ffn_4bit" in notes


def test_public_functions_exist():
    bnb = _bnb()
    for name in ("matmul_4bit_gated", "ffn_4bit"):
        assert callable(getattr(bnb, name)) and name in bnb.__all__
    assert list(inspect.signature(bnb.matmul_4bit_gated).parameters) == ["x", "gate_up", "gate_up_state", "bias"]
    assert list(inspect.signature(bnb.ffn_4bit).parameters) == ["x", "gate_up", "gate_up_state", "down", "down_state", "gate_up_bias",
                                                                "down_bias"]
    assert callable(bnb.functional.interleave_gate_up_4bit)
    sig = inspect.signature(bnb.nn.FFN4bit.from_linears)
    assert list(sig.parameters) == ["gate", "up", "down", "keep_members"] and sig.parameters["keep_members"].default is False
    assert str(_op()._schema) == ("bitsandbytes_amd::gemm_4bit_gated(Tensor A, Tensor B, int[] shapeB, Tensor absmax, int blocksize, "
                                  "str quant_type, Tensor? bias=None) -> Tensor")


def test_gated_supported_is_host_logic():
    """Answers without a device (256 CUs assumed); 1 exactly on the cells the GPU test expects a kernel for, 0 outside the form."""
    sup = _bnb().lib.bnb_mi355x_gemm_4bit_gated_supported
    route = _bnb().lib.bnb_mi355x_gemm_4bit_route
    for (N, K, bs), ms in C.MUST_SERVE:
        for dt in (1, 2):
            for M in ms:
                assert sup(dt, M, N, K, bs) == 1, (dt, M, N, K, bs)
    for M in (1, 2, 8, 16):
        assert sup(2, M, 4096, 4096, 64) == 1
        assert sup(0, M, 4096, 4096, 64) == 0                      # fp32 activations
        assert sup(2, M, 4095, 4096, 64) == 0                      # odd N: a gate row without its up row
        assert sup(2, M, 4096, 4096, 32) == 0                      # blocksize 32
        assert sup(2, M, 4096, 4096 + 64, 128) == 0                # K % blocksize != 0
        assert sup(2, M, 4096, 4096 + 32, 64) == 0
    assert sup(2, 0, 4096, 4096, 64) == 0 and sup(2, 17, 4096, 4096, 64) == 0 and sup(2, -1, 4096, 4096, 64) == 0
    assert sup(3, 1, 4096, 4096, 64) == 0 and sup(2, 1, 0, 4096, 64) == 0 and sup(2, 1, 4096, 0, 64) == 0
    # another kernel family (5 ... 8 rows of a small matrix with short rows: the register-transposed kernel) has no gated form
    assert route(0, 2, 6, 2002, 1024, 64) == 1 and sup(2, 6, 2002, 1024, 64) == 0
    from bitsandbytes_amd.backends import hip

    assert hip.gemm_4bit_gated_supported(torch.bfloat16, 1, 28672, 4096, 64)
    assert not hip.gemm_4bit_gated_supported(torch.float32, 1, 28672, 4096, 64)
    assert not hip.gemm_4bit_gated_supported(torch.float64, 1, 28672, 4096, 64)
    assert not hip.gemm_4bit_gated_supported(torch.bfloat16, 17, 28672, 4096, 64)


# ------------------------------------------------------------------------------------------ fake kernel, argument checks
def _meta_args(N=96, K=128, bs=64, lead=(3,), dtype=torch.bfloat16):
    m = "meta"
    A = torch.empty((*lead, K), dtype=dtype, device=m)
    B = torch.empty((N * K // 2, 1), dtype=torch.uint8, device=m)
    absmax = torch.empty((N * K // bs,), dtype=torch.float32, device=m)
    return [A, B, [N, K], absmax, bs, "nf4"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_fake_kernel_shapes(dtype):
    for lead in ((3,), (1,), (2, 5), (0,), ()):
        y = _op()(*_meta_args(lead=lead, dtype=dtype))
        assert y.shape == (*lead, 48) and y.dtype == dtype and y.device.type == "meta"
    bias = torch.empty((96,), dtype=dtype, device="meta")
    assert _op()(*_meta_args(dtype=dtype), bias=bias).shape == (3, 48)
    assert _op()(*_meta_args(dtype=dtype)[:5], "fp4").shape == (3, 48)


def test_fake_kernel_rejects_bad_arguments():
    m = "meta"

    def bad(match, **change):
        args = _meta_args()
        names = ["A", "B", "shapeB", "absmax", "blocksize", "quant_type"]
        bias = change.pop("bias", None)
        for k, v in change.items():
            args[names.index(k)] = v
        with pytest.raises(RuntimeError, match=match):
            _op()(*args, bias=bias)

    bad("even", shapeB=[95, 128], B=torch.empty((95 * 64, 1), dtype=torch.uint8, device=m), absmax=torch.empty((190,), dtype=torch.float32, device=m))
    bad(r"\[2 F, K\]", shapeB=[2, 48, 128])
    bad("inner dim", A=torch.empty((3, 64), dtype=torch.bfloat16, device=m))
    bad("quant_type", quant_type="int4")
    bad("blocksize", blocksize=48)
    bad("float32", absmax=torch.empty((192,), dtype=torch.float16, device=m))
    bad("absmax must hold", absmax=torch.empty((191,), dtype=torch.float32, device=m))
    bad("4-bit values", B=torch.empty((96 * 64 - 1, 1), dtype=torch.uint8, device=m))
    bad("bias must be", bias=torch.empty((48,), dtype=torch.bfloat16, device=m))
    bad("bias must be", bias=torch.empty((96,), dtype=torch.float16, device=m))
    bad("16/32-bit float", A=torch.empty((3, 128), dtype=torch.float64, device=m))


def test_inference_only():
    bnb = _bnb()
    _oracle_cpu_backend.register()
    W = torch.randn(8, 64)
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4")
    x = torch.randn(2, 64, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_gated(x, packed, state)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.ffn_4bit(x, packed, state, packed, state)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_gated(x.detach(), packed, state, bias=torch.zeros(8, requires_grad=True))
    with pytest.raises(ValueError, match=r"\[2 F, K\]"):
        bnb.matmul_4bit_gated(x.detach(), packed[:28 * 8], bnb.functional.quantize_4bit(W[:7], blocksize=64, quant_type="nf4")[1])


def test_cpu_composition_is_silu_times_up():
    """Off the device the public function is the composition: plain matmul_4bit on the interleaved matrix, torch's silu and *."""
    bnb = _bnb()
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(3)
    W = (torch.randn(24, 128, generator=gen) / 8).bfloat16()
    bias = torch.randn(24, generator=gen).bfloat16()
    x = torch.randn(3, 128, generator=gen).bfloat16()
    packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4")
    with torch.no_grad():
        y = bnb.matmul_4bit(x, packed, state, bias=bias)
        h = bnb.matmul_4bit_gated(x, packed, state, bias=bias)
    assert h.shape == (3, 12) and torch.equal(h, torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2])


# ------------------------------------------------------------------------------------------ layout helper against the oracle
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
@pytest.mark.parametrize("chunked", [False, True], ids=["members", "chunked"])
@pytest.mark.parametrize("quant_type,bs", [("nf4", 64), ("fp4", 128)])
def test_interleave_gate_up_against_the_oracle(nested, chunked, quant_type, bs):
    """Dequantizing the interleaved matrix gives the row-interleave of the members' dequantized weights, bit for bit, without
    requantization; nested statistics arrive un-nested as exactly the oracle's reconstruction."""
    Fn = _bnb().functional
    _oracle_cpu_backend.register()
    gen = torch.Generator().manual_seed(11)
    F_, K = 300, 384          # 300 x 384 / bs blocks per member: more than one group of 256 blocks, groups that end inside a row
    Wg = (torch.randn(F_, K, generator=gen) / 6).bfloat16()
    Wu = (torch.randn(F_, K, generator=gen) * 3).bfloat16()
    if chunked:
        packed_c, st_c = Fn.quantize_4bit(torch.cat([Wg, Wu]), blocksize=bs, quant_type=quant_type, compress_statistics=nested)
        assert st_c.nested == nested
        packed, st = Fn.interleave_gate_up_4bit(packed_c, st_c)
        deq_c = Fn.dequantize_4bit(packed_c, st_c)
        deq_g, deq_u = deq_c[:F_], deq_c[F_:]
        states = [st_c]
    else:
        pg, sg = Fn.quantize_4bit(Wg, blocksize=bs, quant_type=quant_type, compress_statistics=nested)
        pu, su = Fn.quantize_4bit(Wu, blocksize=bs, quant_type=quant_type, compress_statistics=nested)
        packed, st = Fn.interleave_gate_up_4bit(pg, sg, pu, su)
        deq_g, deq_u = Fn.dequantize_4bit(pg, sg), Fn.dequantize_4bit(pu, su)
        states = [sg, su]
    assert not st.nested and st.absmax.dtype == torch.float32 and tuple(st.shape) == (2 * F_, K)
    assert packed.dtype == torch.uint8 and packed.shape == (F_ * K, 1) and st.blocksize == bs and st.quant_type == quant_type
    # the oracle's own reconstruction of every member's statistics, interleaved
    recs = []
    for s in states:
        if nested:
            r = O.dequantize_blockwise(s.absmax, s.state2.absmax, s.state2.code, 256, torch.float32) + s.offset
        else:
            r = s.absmax
        recs.append(r.float().reshape(-1, K // bs))
    rec = C.interleave_rows(recs[0][:F_], recs[0][F_:]) if chunked else C.interleave_rows(recs[0], recs[1])
    assert torch.equal(st.absmax.view(torch.int32), rec.reshape(-1).view(torch.int32))
    want = C.interleave_rows(deq_g, deq_u)
    got = O.dequantize_4bit(packed, st.absmax, bs, quant_type, (2 * F_, K), torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(Fn.dequantize_4bit(packed, st).view(torch.int16), want.view(torch.int16))


def test_interleave_gate_up_refuses_what_it_cannot_permute():
    Fn = _bnb().functional
    _oracle_cpu_backend.register()
    pg, sg = Fn.quantize_4bit(torch.randn(6, 96), blocksize=64, quant_type="nf4")      # K % blocksize != 0: blocks straddle rows
    with pytest.raises(ValueError, match="whole quantization blocks"):
        Fn.interleave_gate_up_4bit(pg, sg, pg, sg)
    pg, sg = Fn.quantize_4bit(torch.randn(6, 128), blocksize=64, quant_type="nf4")
    pu, su = Fn.quantize_4bit(torch.randn(6, 128), blocksize=64, quant_type="fp4")
    with pytest.raises(ValueError, match="same shape"):
        Fn.interleave_gate_up_4bit(pg, sg, pu, su)
    with pytest.raises(ValueError, match="together"):
        Fn.interleave_gate_up_4bit(pg, sg, pu)
    p7, s7 = Fn.quantize_4bit(torch.randn(7, 128), blocksize=64, quant_type="nf4")
    with pytest.raises(ValueError, match="even row count"):
        Fn.interleave_gate_up_4bit(p7, s7)


def test_ffn4bit_from_linears_on_the_host():
    """The block over oracle-backed CPU layers: the members' composition bit for bit, both ways of keep_members; released members hold
    no packed bytes; the block adds nothing to a state dict."""
    bnb = _bnb()
    _oracle_cpu_backend.register()
    H, F_ = 128, 192
    gen = torch.Generator().manual_seed(5)

    def layer(i, o, bias):
        l = bnb.nn.Linear4bit(i, o, bias=bias, quant_type="nf4", compress_statistics=True, compute_dtype=torch.bfloat16)
        W = (torch.randn(o, i, generator=gen) / i ** 0.5).bfloat16()
        packed, state = bnb.functional.quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=True)
        l.weight = bnb.nn.Params4bit.from_prequantized(packed, state.as_dict(packed=True), device="cpu", module=l)
        if bias:
            l.bias.data = torch.randn(o, generator=gen).bfloat16()
        return l

    for keep in (True, False):
        gate, up, down = layer(H, F_, True), layer(H, F_, False), layer(F_, H, True)
        x = torch.randn(3, H, generator=gen).bfloat16()
        with torch.no_grad():
            want = down(torch.nn.functional.silu(gate(x)) * up(x))
            gate_bytes = gate.weight.numel()
            block = bnb.nn.FFN4bit.from_linears(gate, up, down, keep_members=keep)
            got = block(x)
        assert torch.equal(got, want)
        assert block.state_dict() == {} and list(block.parameters()) == []
        assert block.gate_up.numel() == 2 * gate_bytes and not block.gate_up_state.nested
        assert (gate.weight.numel(), up.weight.numel()) == ((gate_bytes, gate_bytes) if keep else (0, 0))
        assert (block.members is not None) == keep


# ------------------------------------------------------------------------------------------ preconditions of the GPU cases
def test_case_list():
    assert len(C.CASES) + len(C.EXCLUDED) == len(C.SHAPES) * len(C.DTYPES) == 18
    assert all(case.N % 2 == 0 and case.K % case.blocksize == 0 for case in C.CASES)
    for case in C.EXCLUDED:   # a case is excluded only because exact_inputs' own assertion fails for it
        with pytest.raises(AssertionError):
            C.build_case(case)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_cases_are_exact_and_live(case):
    ex = _built(case)          # (asserts the exact-sum bound: every fp32 partial sum is exact in any order)
    assert ex.x.shape == (C.MAX_ROWS, case.K) and not ex.nested
    for with_bias in (False, True):
        share = C.live_share(ex, with_bias)
        print(f"{case.name} bias={int(with_bias)}: {share:.3f} of the gate values in [2^-4, 8]")
        assert share >= 0.5, (case.name, with_bias, share)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cases_survive_quantization(shape):
    """The oracle's quantizer returns the intended scales and its dequantizer the constructed matrix, bit for bit."""
    N, K, bs = shape
    rows = slice(0, min(N, 512))      # (the construction is row-wise: a slab of rows shows what every row does)
    for dtype in C.DTYPES:
        ex = _built(C.FFNCase(N, K, bs, dtype))
        packed, absmax = ORACLE_OPS.quantize_4bit(ex.W[rows], bs)
        n = rows.stop
        assert torch.equal(absmax.flatten(), ex.scale[:n * K // bs])
        back = ORACLE_OPS.dequantize_4bit(packed, absmax, bs, (n, K), dtype)
        assert torch.equal(back.view(torch.int16), ex.W[rows].view(torch.int16))
        # and the oracle's fused matmul on it equals the float64 reference: the gate / up values the GPU test compares against
        y = O.gemm_4bit(ex.x[:3], packed, (n, K), absmax.flatten(), bs, "fp4", ex.bias[:n])[0]
        assert torch.equal(y, (ex.x[:3].double() @ ex.W[rows].double().t() + ex.bias[:n].double()).to(dtype))
