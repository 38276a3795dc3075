"""GPU: the dense gated-SiLU FFN on one device - the gated epilogue of the streaming kernel and of the streaming MFMA kernel
(bitsandbytes_amd::gemm_4bit_gated, csrc/gemv4_stream.hip kGated, csrc/gemm4_mfma_sm.hip GATED), ``matmul_4bit_gated`` / ``ffn_4bit``
and ``nn.FFN4bit``.

* exact: on the operands of tests/exact_inputs.py (tests/ffn_cases.py: the matrix built there IS the interleaved matrix) the output
  equals ``F.silu(g) * u`` - torch's own kernels on the GPU, on the even and odd columns of the float64 reference rounded once - bit
  for bit, for every shape, every M from 1 to 17, with and without bias; the launch is the family the plain op runs on the same
  matrix and M (streaming kernel or streaming MFMA kernel); where the predicate says 0 the raw op raises and the public function
  gives the same bits through the composition.
* gated equals plain on ordinary NF4 data: ``F.silu(y[:, 0::2]) * y[:, 1::2]`` of ``matmul_4bit``'s output ``y``, bit for bit.
* member identity: ``FFN4bit.from_linears(gate, up, down)(x)`` equals ``down(F.silu(gate(x)) * up(x))`` of the three layers.
* the C entry point through ctypes, determinism, graph capture, opcheck.
The preconditions are asserted on the CPU by tests/test_ffn_host.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import ffn_cases as C
from routed_sweep import gpu_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.gemm_4bit_gated.default


def _plain_op():
    return torch.ops.bitsandbytes.gemm_4bit.default


def _supported(dtype, M, N, K, bs) -> bool:
    return _bnb().lib.bnb_mi355x_gemm_4bit_gated_supported(C.DT_CODE[dtype], M, N, K, bs) == 1


# ------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def _prepared(case):
    """Everything of a case that its tests share, computed once and never written to."""
    bnb = _bnb()
    ex = C.build_case(case)
    packed = X.check_quantization(ex, gpu_ops(), DEV)
    absmax = ex.scale.to(DEV)
    x = ex.x.to(DEV)
    bias = ex.bias.to(DEV)
    y64 = x.double() @ ex.W.to(DEV).double().t()                      # [MAX_ROWS, 2 F]; exact (exact_inputs.py)
    want = {}
    for with_bias in (False, True):
        y = (y64 + bias.double() if with_bias else y64).to(case.dtype)
        want[with_bias] = TF.silu(y[:, 0::2]) * y[:, 1::2]            # torch's kernels on T-valued tensors
    state = bnb.functional.QuantState(absmax=absmax, shape=torch.Size((case.N, case.K)), code=bnb.functional.get_4bit_type("fp4", device=DEV),
                                      blocksize=case.blocksize, quant_type="fp4", dtype=case.dtype)
    return dict(ex=ex, packed=packed, absmax=absmax, x=x, bias=bias, want=want, state=state)


def test_named_cells_have_a_kernel():
    """The cells the issue names: the predicate answers 1 and the plain op on the same matrix runs family 1 (M = 1) / 7 (sm rows)."""
    lib = _bnb().lib
    for (N, K, bs), ms in C.MUST_SERVE:
        d = _prepared(C.FFNCase(N, K, bs, torch.bfloat16))
        for M in ms:
            assert _supported(torch.bfloat16, M, N, K, bs) and _supported(torch.float16, M, N, K, bs), (N, K, bs, M)
            _plain_op()(d["x"][:M], d["packed"], [N, K], d["absmax"], bs, "fp4")
            assert lib.bnb_mi355x_last_gemm_kernel() == (C.K_STREAM if M == 1 else C.K_SM), (N, K, bs, M)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_gated_exact_at_every_batch_size(case):
    bnb = _bnb()
    lib = bnb.lib
    N, K, bs, F_ = case.N, case.K, case.blocksize, case.F
    d = _prepared(case)
    failures, fused, composed = [], 0, 0
    for M in C.MS:
        x = d["x"][:M]
        served = _supported(case.dtype, M, N, K, bs)
        assert served or M != 1, "one row always has a kernel on these shapes"
        assert not (served and M == 17)
        _plain_op()(x, d["packed"], [N, K], d["absmax"], bs, "fp4")
        plain_family = lib.bnb_mi355x_last_gemm_kernel()
        assert served == (plain_family in (C.K_STREAM, C.K_SM)) or M > 16, (M, served, plain_family)
        for with_bias in (False, True):
            bias = d["bias"] if with_bias else None
            want = d["want"][with_bias][:M]
            if served:
                y = _op()(x, d["packed"], [N, K], d["absmax"], bs, "fp4", bias)
                family = lib.bnb_mi355x_last_gemm_kernel()
                assert family == plain_family and family in (C.K_STREAM, C.K_SM), (M, family, plain_family)
                fused += 1
            else:
                with pytest.raises(ValueError, match="no kernel"):
                    _op()(x, d["packed"], [N, K], d["absmax"], bs, "fp4", bias)
                composed += 1
            y2 = bnb.matmul_4bit_gated(x, d["packed"], d["state"], bias=bias)
            for name, t in (("op", y), ("matmul_4bit_gated", y2)) if served else (("matmul_4bit_gated", y2),):
                assert t.shape == (M, F_) and t.dtype == case.dtype
                if not torch.equal(t, want):
                    r, c, got, exp = X.first_mismatch(t.cpu(), want.cpu())
                    failures.append(f"M={M} bias={int(with_bias)} {name} family={plain_family}: row {r} column {c}: got {got!r}, want {exp!r}")
    print(f"{case.name}: {fused} fused and {composed} composed cells, {len(failures)} not bit-equal")
    assert fused >= 2 and composed >= 2
    assert not failures, f"{len(failures)} cells differ; first: {failures[:5]}"


# ------------------------------------------------------------------------------------------ gated equals plain on ordinary data
def _random_weight(N, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype).to(DEV)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gated_equals_silu_of_the_plain_matmul(shape):
    bnb = _bnb()
    N, K, bs = shape
    for dtype, qt in ((torch.bfloat16, "nf4"), (torch.float16, "fp4")):
        W = _random_weight(N, K, dtype, N + K)
        packed, state = bnb.functional.quantize_4bit(W, blocksize=bs, quant_type=qt)
        gen = torch.Generator().manual_seed(N)
        x_all = torch.randn(C.MAX_ROWS, K, generator=gen).to(dtype).to(DEV)
        bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
        bad = []
        for M in C.MS:
            for b in (None, bias):
                y = bnb.matmul_4bit(x_all[:M], packed, state, bias=b)
                h = bnb.matmul_4bit_gated(x_all[:M], packed, state, bias=b)
                if not torch.equal(h, TF.silu(y[:, 0::2]) * y[:, 1::2]):
                    bad.append((M, b is not None))
        assert not bad, f"{shape} {dtype} {qt}: (M, bias) cells that differ from silu(y[:, 0::2]) * y[:, 1::2]: {bad}"


# ------------------------------------------------------------------------------------------ member identity
def _layer(in_f, out_f, dtype, seed, bias=True, nested=False, blocksize=64, quant_type="nf4"):
    bnb = _bnb()
    gen = torch.Generator().manual_seed(seed)
    layer = bnb.nn.Linear4bit(in_f, out_f, bias=bias, quant_type=quant_type, compress_statistics=nested, compute_dtype=dtype)
    W = (torch.randn(out_f, in_f, generator=gen) * (3.0 / in_f ** 0.5)).to(dtype)
    layer.weight = bnb.nn.Params4bit(W, requires_grad=False, quant_type=quant_type, compress_statistics=nested, blocksize=blocksize,
                                     module=layer)
    if bias:
        layer.bias.data = torch.randn(out_f, generator=gen).to(dtype)
    return layer.to(DEV)


def _member_identity(F_, K, H, bs, dtype, Ms, nested, keep, family=None, bias=True):
    bnb = _bnb()
    lib = bnb.lib
    gate = _layer(K, F_, dtype, 1, bias=bias, nested=nested, blocksize=bs)
    up = _layer(K, F_, dtype, 2, bias=False, nested=nested, blocksize=bs)
    down = _layer(F_, H, dtype, 3, bias=bias, nested=nested)
    gen = torch.Generator().manual_seed(4)
    xs = [torch.randn(M, K, generator=gen).to(dtype).to(DEV) for M in Ms]
    want = []
    with torch.no_grad():
        for x in xs:
            for _ in range(2):   # (the second call of a layer takes its prepared path: the reference is what a model runs)
                g = gate(x)
                fam_g = lib.bnb_mi355x_last_gemm_kernel()
                u = up(x)
                fam_u = lib.bnb_mi355x_last_gemm_kernel()
                y = down(TF.silu(g) * u)
            if family is not None:
                assert (fam_g, fam_u) == (family, family), (x.shape, fam_g, fam_u)
            want.append(y)
        block = bnb.nn.FFN4bit.from_linears(gate, up, down, keep_members=keep)
        assert not block.gate_up_state.nested and block.state_dict() == {}
        assert (gate.weight.numel() == 0) == (not keep) and (up.weight.numel() == 0) == (not keep)
        for x, w in zip(xs, want):
            if family is not None:
                bnb.matmul_4bit_gated(x, block.gate_up, block.gate_up_state, bias=block.gate_up_bias)
                assert lib.bnb_mi355x_last_gemm_kernel() == family
            y = block(x)
            assert y.shape == w.shape and y.dtype == w.dtype
            assert torch.equal(y, w), f"F={F_} K={K} M={x.shape[0]} nested={nested} keep={keep}: {X.first_mismatch(y.cpu(), w.cpu())}"
        if keep:   # the members still work on their own
            assert torch.equal(down(TF.silu(gate(xs[0])) * up(xs[0])), want[0])


@pytest.mark.parametrize("shape", C.STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_member_identity_one_row(shape, nested):
    N, K, bs = shape
    _member_identity(N // 2, K, 256, bs, torch.bfloat16, (1,), nested, keep=nested, family=C.K_STREAM)


@pytest.mark.parametrize("nested,keep,dtype", [(False, False, torch.bfloat16), (True, True, torch.float16), (True, False, torch.bfloat16)],
                         ids=["plain-released", "nested-kept-fp16", "nested-released"])
def test_member_identity_batched(nested, keep, dtype):
    _member_identity(3072, 256, 256, 64, dtype, (2, 4, 8, 16), nested, keep, family=C.K_SM)


def test_member_identity_outside_the_gated_launch():
    """17 rows and fp32 compute: the composition on the interleaved matrix, the members' bits all the same."""
    _member_identity(1001, 1024, 128, 64, torch.bfloat16, (1, 6, 17), False, True)
    _member_identity(96, 128, 64, 64, torch.float32, (1, 3), True, False)


# ------------------------------------------------------------------------------------------ C entry point, determinism, capture
CELLS = ((C.FFNCase(2816, 2048, 64, torch.bfloat16), 1, C.K_STREAM), (C.FFNCase(4352, 256, 64, torch.float16), 9, C.K_SM))


def test_c_entry_point_through_ctypes():
    lib = _bnb().lib
    for case, M, family in CELLS:
        d = _prepared(case)
        x = d["x"][:M].contiguous()
        for bias in (None, d["bias"]):
            y_op = _op()(x, d["packed"], [case.N, case.K], d["absmax"], case.blocksize, "fp4", bias)
            out = torch.full((M, case.F), float("nan"), dtype=case.dtype, device=DEV)
            lib.bnb_mi355x_gemm_4bit_gated(C.DT_CODE[case.dtype], x.data_ptr(), d["packed"].data_ptr(), d["absmax"].data_ptr(), out.data_ptr(),
                                           None if bias is None else bias.data_ptr(), M, case.N, case.K, case.blocksize, 1,
                                           torch.cuda.current_stream().cuda_stream)
            assert lib.bnb_mi355x_last_gemm_kernel() == family
            torch.cuda.synchronize()
            assert torch.equal(out, y_op) and torch.equal(out, d["want"][bias is not None][:M])


def test_twenty_launches_give_equal_bits():
    for case, M, _ in CELLS:
        d = _prepared(case)
        first = _op()(d["x"][:M], d["packed"], [case.N, case.K], d["absmax"], case.blocksize, "fp4", d["bias"])
        for _ in range(19):
            assert torch.equal(_op()(d["x"][:M], d["packed"], [case.N, case.K], d["absmax"], case.blocksize, "fp4", d["bias"]), first)


@pytest.mark.parametrize("M", [1, 4, 17])
def test_captured_block_follows_x(M):
    """One torch.cuda.graph of ffn_4bit - the fused block at 1 and 4 rows, the composition at 17 -, replayed with new contents in x's
    buffer: the host read nothing."""
    bnb = _bnb()
    H, F_ = 512, 1408
    dtype = torch.bfloat16
    packed_gu, st_gu = bnb.functional.quantize_4bit(_random_weight(2 * F_, H, dtype, 61), blocksize=64, quant_type="nf4")
    packed_dn, st_dn = bnb.functional.quantize_4bit(_random_weight(H, F_, dtype, 62), blocksize=64, quant_type="nf4")
    gen = torch.Generator().manual_seed(63)
    bgu, bdn = torch.randn(2 * F_, generator=gen).to(dtype).to(DEV), torch.randn(H, generator=gen).to(dtype).to(DEV)
    xs = [torch.randn(M, H, generator=gen).to(dtype).to(DEV) for _ in range(4)]
    call = lambda x: bnb.ffn_4bit(x, packed_gu, st_gu, packed_dn, st_dn, gate_up_bias=bgu, down_bias=bdn)
    with torch.no_grad():
        eager = [call(x) for x in xs]
        y0 = bnb.matmul_4bit(xs[0], packed_gu, st_gu, bias=bgu)
        assert torch.equal(eager[0], bnb.matmul_4bit(TF.silu(y0[:, 0::2]) * y0[:, 1::2], packed_dn, st_dn, bias=bdn))
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
        for k in (1, 2, 3):
            buf.copy_(xs[k])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager[k]), f"replay {k} did not follow x"


def test_opcheck():
    bnb = _bnb()
    N, K = 192, 256
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, torch.bfloat16, 81), blocksize=64, quant_type="nf4")
    bias = torch.randn(N, device=DEV).bfloat16()
    for lead in ((1,), (3,), (2, 2)):
        x = torch.randn(*lead, K, device=DEV).bfloat16()
        for kwargs in (dict(), dict(bias=bias)):
            torch.library.opcheck(_op(), (x, packed, [N, K], state.absmax, 64, "nf4"), kwargs, test_utils=("test_schema", "test_faketensor"))
    assert _op()(x[:0], packed, [N, K], state.absmax, 64, "nf4").shape == (0, 2, N // 2)
    # what the fake kernel cannot see: a call without a kernel is an error, never another path
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(17, K, device=DEV).bfloat16(), packed, [N, K], state.absmax, 64, "nf4")
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(1, K, device=DEV), packed, [N, K], state.absmax, 64, "nf4")
