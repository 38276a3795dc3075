"""GPU: the LoRA adapter term as the epilogue of the streaming kernel and of the streaming MFMA kernel
(bitsandbytes_amd::gemm_4bit_lora, csrc/gemv4_stream.hip kLora, csrc/gemm4_mfma_sm.hip LORA), ``matmul_4bit_lora`` and
``nn.Linear4bitLoRA``.

* exact: on the operands of tests/lora_cases.py the output equals ``(x64 @ W64.T + bias64 + s * t64 @ B_l64.T)`` rounded once, bit for
  bit, for every shape, every M from 1 to 17, with and without bias, plain and nested statistics; the launch is the family the plain
  op runs on the same matrix and M (streaming kernel or streaming MFMA kernel); where the predicate says 0 the raw op raises and the
  public function composes - inside the tolerance.
* ``t == 0`` gives the plain call's bits on ordinary NF4 data: the base path inside the new instances is the plain one.
* ordinary data against float64 inside a derived per-element bound (lora_cases.tolerance), fused and composed.
* module identity, the C entry point through ctypes, determinism, graph capture, opcheck.
The preconditions are asserted on the CPU by tests/test_lora_host.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import lora_cases as C
from routed_sweep import gpu_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_lora.default


def _plain_op():
    return torch.ops.bitsandbytes.gemm_4bit.default


def _supported(dtype, M, N, K, bs, nested, r) -> bool:
    return _bnb().lib.bnb_mi355x_gemm_4bit_lora_supported(C.DT_CODE[dtype], M, N, K, bs, 1 if nested else 0, r) == 1


# ------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def _prepared(case):
    """Everything of a case that its tests share, computed once and never written to."""
    Fn = _bnb().functional
    ex = C.build_case(case)
    packed = X.check_quantization(ex, gpu_ops(), DEV)
    absmax, a8, code, off = ex.stats_args(DEV)
    x = ex.x.to(DEV)
    bias = ex.bias.to(DEV)
    y64 = x.double() @ ex.W.to(DEV).double().t()                      # [MAX_ROWS, N]; exact (exact_inputs.py)
    adapters, want = {}, {}
    for r, s in zip(case.ranks, C.SCALINGS):
        t, b = (v.to(DEV) for v in C.build_adapter(case, r))
        adapters[r] = (t, b, s)
        term = C.adapter_term64(t, b, s)
        for with_bias in (False, True):
            want[r, with_bias] = (y64 + term + (bias.double() if with_bias else 0.0)).to(case.dtype)
    shape = torch.Size((case.N, case.K))
    code4 = Fn.get_4bit_type("fp4", device=DEV)
    if case.nested:
        state2 = Fn.QuantState(absmax=absmax, code=code, blocksize=256, dtype=torch.float32)
        state = Fn.QuantState(absmax=a8, shape=shape, code=code4, blocksize=case.blocksize, quant_type="fp4", dtype=case.dtype, offset=off,
                              state2=state2)
    else:
        state = Fn.QuantState(absmax=absmax, shape=shape, code=code4, blocksize=case.blocksize, quant_type="fp4", dtype=case.dtype)
    stats = dict(absmax_8bit=a8, absmax_code=code, absmax_offset=off)
    return dict(ex=ex, packed=packed, absmax=absmax, stats=stats, x=x, bias=bias, y64=y64, adapters=adapters, want=want, state=state)


def _call(d, case, M, r, bias):
    t, b, s = d["adapters"][r]
    return _op()(d["x"][:M], d["packed"], [case.N, case.K], d["absmax"], case.blocksize, "fp4", t[:M].contiguous(), b, s, bias, **d["stats"])


def _plain(d, case, M, bias=None):
    return _plain_op()(d["x"][:M], d["packed"], [case.N, case.K], d["absmax"], case.blocksize, "fp4", bias, *d["stats"].values())


def test_named_cells_have_a_kernel():
    """The cells the issue names: the predicate answers 1 - plain and nested statistics, every rank - and the plain op on the same
    matrix runs family 1 (M = 1) / 7 (sm rows)."""
    lib = _bnb().lib
    for (N, K, bs), ms in C.MUST_SERVE:
        d = _prepared(C.LoRACase(N, K, bs, torch.bfloat16))
        for M in ms:
            for nested in (False, True):
                for r in C.RANKS:
                    assert _supported(torch.bfloat16, M, N, K, bs, nested, r) and _supported(torch.float16, M, N, K, bs, nested, r), (N, K, bs, M, nested, r)
            _plain(d, C.LoRACase(N, K, bs), M)
            assert lib.bnb_mi355x_last_gemm_kernel() == (C.K_STREAM if M == 1 else C.K_SM), (N, K, bs, M)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_lora_exact_at_every_batch_size(case):
    bnb = _bnb()
    lib = bnb.lib
    N, K, bs = case.N, case.K, case.blocksize
    d = _prepared(case)
    neither = (N, K, bs) in C.OTHER_SHAPES
    failures, fused, composed = [], 0, 0
    for M in C.MS:
        _plain(d, case, M)
        plain_family = lib.bnb_mi355x_last_gemm_kernel()
        for r in case.ranks:
            t, b, s = d["adapters"][r]
            served = _supported(case.dtype, M, N, K, bs, case.nested, r)
            assert served or M != 1, "one row always has a kernel on these shapes"
            assert not (served and M == 17)
            assert served == (plain_family in (C.K_STREAM, C.K_SM)) or M > 16, (M, r, served, plain_family)
            for with_bias in (False, True):
                bias = d["bias"] if with_bias else None
                want = d["want"][r, with_bias][:M]
                if served:
                    y = _call(d, case, M, r, bias)
                    family = lib.bnb_mi355x_last_gemm_kernel()
                    assert family == plain_family and family in (C.K_STREAM, C.K_SM), (M, family, plain_family)
                    fused += 1
                else:
                    with pytest.raises(ValueError, match="no kernel"):
                        _call(d, case, M, r, bias)
                    composed += 1
                y2 = bnb.matmul_4bit_lora(d["x"][:M], d["packed"], d["state"], t[:M], b, s, bias=bias)
                assert y2.shape == (M, N) and y2.dtype == case.dtype
                if served:
                    assert y.shape == (M, N) and y.dtype == case.dtype
                    for name, got in (("op", y), ("matmul_4bit_lora", y2)):
                        if not torch.equal(got, want):
                            row, col, g, e = X.first_mismatch(got.cpu(), want.cpu())
                            failures.append(f"M={M} r={r} bias={int(with_bias)} {name} family={plain_family}: row {row} column {col}: got {g!r}, want {e!r}")
                else:
                    # the composition rounds the base first: inside the tolerance around (plain output + adapter term)
                    yp = _plain(d, case, M, bias)
                    want64 = yp.double() + C.adapter_term64(t[:M], b, s)
                    over = (y2.double() - want64).abs() > C.tolerance(want64, yp, t[:M], b, s, case.dtype)
                    if bool(over.any()):
                        failures.append(f"M={M} r={r} bias={int(with_bias)} composition: {int(over.sum())} elements outside the tolerance")
    print(f"{case.name}: {fused} fused and {composed} composed cells, {len(failures)} wrong")
    assert fused >= 2
    if neither:
        assert composed >= 2
    assert not failures, f"{len(failures)} cells differ; first: {failures[:5]}"


# ------------------------------------------------------------------------------------------ ordinary data
def _random_weight(N, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype).to(DEV)


def _state_args(state):
    """(absmax, kwargs) of the raw ops for a library-made QuantState."""
    if not state.nested:
        return state.absmax, {}
    return state.state2.absmax, dict(absmax_8bit=state.absmax, absmax_code=state.state2.code, absmax_offset=state.offset)


@pytest.mark.parametrize("shape", [(4096, 4096), (4352, 8192)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_zero_t_gives_the_plain_call(shape, nested):
    bnb = _bnb()
    N, K = shape
    dtype = torch.bfloat16
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, N + K), blocksize=64, quant_type="nf4", compress_statistics=nested)
    absmax, kw = _state_args(state)
    gen = torch.Generator().manual_seed(N)
    x_all = torch.randn(16, K, generator=gen).to(dtype).to(DEV)
    bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
    for r in (16, 128):
        b = (torch.randn(N, r, generator=gen) * 0.5).to(dtype).to(DEV)
        for M in (1, 2, 5, 16):
            t = torch.zeros(M, r, dtype=dtype, device=DEV)
            for bs_ in (None, bias):
                y = _plain_op()(x_all[:M], packed, [N, K], absmax, 64, "nf4", bs_, *kw.values()) if nested else \
                    _plain_op()(x_all[:M], packed, [N, K], absmax, 64, "nf4", bs_)
                out = _op()(x_all[:M], packed, [N, K], absmax, 64, "nf4", t, b, 2.0, bs_, **kw)
                assert torch.equal(out, y), (shape, nested, r, M, bs_ is not None, X.first_mismatch(out.cpu(), y.cpu()))


@pytest.mark.parametrize("shape", [(4096, 4096), (2816, 2048), (4096, 2752)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
def test_ordinary_data_against_float64(shape, dtype):
    """Random NF4 weights, x ~ N(0, 1), lora_A ~ N(0, 1 / K), B_l ~ N(0, 0.25): the fused op (where served) and the composition, each
    inside lora_cases.tolerance around ``y64 + s * t64 @ B_l64.T`` with ``y`` the plain op's output. Every figure is printed."""
    bnb = _bnb()
    N, K = shape
    for nested in (False, True):
        packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, N + K + 1), blocksize=64, quant_type="nf4", compress_statistics=nested)
        absmax, kw = _state_args(state)
        gen = torch.Generator().manual_seed(K)
        bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
        for r, s in ((16, 2.0), (64, 0.5)):
            A = (torch.randn(r, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
            b = (torch.randn(N, r, generator=gen) * 0.5).to(dtype).to(DEV)
            for M in (1, 4, 16, 17):
                x = torch.randn(M, K, generator=gen).to(dtype).to(DEV)
                t = TF.linear(x, A)
                y = bnb.matmul_4bit(x, packed, state, bias=bias)
                want = y.double() + C.adapter_term64(t, b, s)
                tol = C.tolerance(want, y, t, b, s, dtype)
                results = {"composed": torch.addmm(y, t, b.t(), alpha=s), "matmul_4bit_lora": bnb.matmul_4bit_lora(x, packed, state, t, b, s, bias=bias)}
                if _supported(dtype, M, N, K, 64, nested, r):
                    results["op"] = _op()(x, packed, [N, K], absmax, 64, "nf4", t, b, s, bias, **kw)
                else:
                    assert torch.equal(results["matmul_4bit_lora"], results["composed"])
                for name, got in results.items():
                    ratio = float(((got.double() - want).abs() / tol).max())
                    print(f"{shape} {dtype} nested={int(nested)} r={r} s={s} M={M} {name}: worst error / bound {ratio:.3f}")
                    assert ratio <= 1.0, (shape, dtype, nested, r, s, M, name, ratio)


# ------------------------------------------------------------------------------------------ module identity
@pytest.mark.parametrize("nested,dtype,bias", [(True, torch.bfloat16, True), (False, torch.float16, False)], ids=["nested-bf16-bias", "plain-fp16"])
def test_module_identity(nested, dtype, bias):
    bnb = _bnb()
    K, N, r, s = 2048, 2816, 16, 2.0
    gen = torch.Generator().manual_seed(7)
    layer = bnb.nn.Linear4bit(K, N, bias=bias, quant_type="nf4", compress_statistics=nested, compute_dtype=dtype)
    W = (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype)
    layer.weight = bnb.nn.Params4bit(W, requires_grad=False, quant_type="nf4", compress_statistics=nested, blocksize=64, module=layer)
    if bias:
        layer.bias.data = torch.randn(N, generator=gen).to(dtype)
    layer = layer.to(DEV)
    A = torch.randn(r, K, generator=gen) / K ** 0.5          # fp32, as an adapter checkpoint stores them
    B_l = torch.randn(N, r, generator=gen) * 0.5
    with torch.no_grad():
        mod = bnb.nn.Linear4bitLoRA.from_linear(layer, A, B_l, s)
        assert mod.base is layer and mod.base.weight.data_ptr() == layer.weight.data_ptr() and mod.state_dict() == {}
        assert mod.lora_A.dtype == dtype and mod.lora_A.device.type == "cuda" and mod.lora_B.is_contiguous()
        Ad, Bd = A.to(DEV).to(dtype), B_l.to(DEV).to(dtype)
        for lead in ((1,), (2, 3), (16,), (17,)):
            x = torch.randn(*lead, K, generator=gen).to(dtype).to(DEV)
            got = mod(x)
            want = bnb.matmul_4bit_lora(x, layer.weight, layer.weight.quant_state, TF.linear(x, Ad), Bd, s,
                                        bias=layer.bias.detach() if bias else None)
            assert got.shape == (*lead, N) and got.dtype == dtype and torch.equal(got, want), lead
            peft = layer(x) + TF.linear(TF.linear(x, Ad), Bd) * s
            assert float((got.float() - peft.float()).abs().max()) <= 2.0 ** -5 * float(peft.float().abs().max())


# ------------------------------------------------------------------------------------------ C entry point, determinism, capture
CELLS = ((C.LoRACase(2816, 2048, 64, torch.bfloat16, True), 1, C.K_STREAM), (C.LoRACase(4352, 256, 64, torch.float16, False), 9, C.K_SM))


def test_c_entry_point_through_ctypes():
    lib = _bnb().lib
    for case, M, family in CELLS:
        d = _prepared(case)
        x = d["x"][:M].contiguous()
        r = case.ranks[0]
        t, b, s = d["adapters"][r]
        tm = t[:M].contiguous()
        st = d["stats"]
        for bias in (None, d["bias"]):
            y_op = _call(d, case, M, r, bias)
            out = torch.full((M, case.N), float("nan"), dtype=case.dtype, device=DEV)
            lib.bnb_mi355x_gemm_4bit_lora(C.DT_CODE[case.dtype], x.data_ptr(), d["packed"].data_ptr(), d["absmax"].data_ptr(),
                                          None if st["absmax_8bit"] is None else st["absmax_8bit"].data_ptr(),
                                          None if st["absmax_code"] is None else st["absmax_code"].data_ptr(),
                                          None if st["absmax_offset"] is None else st["absmax_offset"].data_ptr(), out.data_ptr(),
                                          None if bias is None else bias.data_ptr(), tm.data_ptr(), b.data_ptr(), s, r, M, case.N, case.K,
                                          case.blocksize, 1, torch.cuda.current_stream().cuda_stream)
            assert lib.bnb_mi355x_last_gemm_kernel() == family
            torch.cuda.synchronize()
            assert torch.equal(out, y_op) and torch.equal(out, d["want"][r, bias is not None][:M])


def test_thirty_launches_give_equal_bits():
    """Ordinary data (sums that round): the bits do not depend on which wavefront finishes first."""
    bnb = _bnb()
    dtype = torch.bfloat16
    for (N, K), M in (((4096, 4096), 1), ((4352, 8192), 9), ((2816, 2048), 3)):
        packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, 5), blocksize=64, quant_type="nf4", compress_statistics=True)
        absmax, kw = _state_args(state)
        gen = torch.Generator().manual_seed(6)
        x = torch.randn(M, K, generator=gen).to(dtype).to(DEV)
        t = torch.randn(M, 24, generator=gen).to(dtype).to(DEV)
        b = torch.randn(N, 24, generator=gen).to(dtype).to(DEV)
        bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
        first = _op()(x, packed, [N, K], absmax, 64, "nf4", t, b, 0.5, bias, **kw)
        for _ in range(29):
            assert torch.equal(_op()(x, packed, [N, K], absmax, 64, "nf4", t, b, 0.5, bias, **kw), first)


@pytest.mark.parametrize("M", [1, 4, 17])
def test_captured_layer_follows_x(M):
    """One torch.cuda.graph of Linear4bitLoRA's two launches - the fused launch at 1 and 4 rows, the composition at 17 -, replayed with
    new contents in x's buffer: the host read nothing."""
    bnb = _bnb()
    K, N, r, s = 512, 1408, 16, 0.5
    dtype = torch.bfloat16
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, 61), blocksize=64, quant_type="nf4", compress_statistics=True)
    gen = torch.Generator().manual_seed(63)
    A = (torch.randn(r, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
    b = (torch.randn(N, r, generator=gen) * 0.5).to(dtype).to(DEV)
    bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
    xs = [torch.randn(M, K, generator=gen).to(dtype).to(DEV) for _ in range(3)]
    call = lambda x: bnb.matmul_4bit_lora(x, packed, state, TF.linear(x, A), b, s, bias=bias)
    with torch.no_grad():
        eager = [call(x) for x in xs]
        assert not torch.equal(eager[1], eager[2])
        buf = xs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                call(buf)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = call(buf)
        for k in (1, 2):
            buf.copy_(xs[k])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager[k]), f"replay {k} did not follow x"


def test_opcheck():
    bnb = _bnb()
    N, K, r = 192, 256, 16
    bias = torch.randn(N, device=DEV).bfloat16()
    b = torch.randn(N, r, device=DEV).bfloat16()
    for nested in (False, True):
        packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, torch.bfloat16, 81), blocksize=64, quant_type="nf4", compress_statistics=nested)
        absmax, kw = _state_args(state)
        for lead in ((1,), (3,), (2, 2)):
            x = torch.randn(*lead, K, device=DEV).bfloat16()
            t = torch.randn(*lead, r, device=DEV).bfloat16()
            for kwargs in (dict(kw), dict(kw, bias=bias)):
                torch.library.opcheck(_op(), (x, packed, [N, K], absmax, 64, "nf4", t, b, 0.5), kwargs, test_utils=("test_schema", "test_faketensor"))
        assert _op()(x[:0], packed, [N, K], absmax, 64, "nf4", t[:0], b, 0.5, **kw).shape == (0, 2, N)
    # what the fake kernel cannot see: a call without a kernel is an error, never another path
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, torch.bfloat16, 81), blocksize=64, quant_type="nf4")
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(17, K, device=DEV).bfloat16(), packed, [N, K], state.absmax, 64, "nf4", torch.randn(17, r, device=DEV).bfloat16(), b, 0.5)
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(1, K, device=DEV), packed, [N, K], state.absmax, 64, "nf4", torch.randn(1, r, device=DEV), b.float(), 0.5)
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(1, K, device=DEV).bfloat16(), packed, [N, K], state.absmax, 64, "nf4", torch.randn(1, 12, device=DEV).bfloat16(),
              torch.randn(N, 12, device=DEV).bfloat16(), 0.5)
