"""GPU: the LoRA shrink matmul ``t = x @ lora_A^T`` as a kernel of the library (bitsandbytes_amd::lora_shrink, csrc/lora_shrink.hip),
``bitsandbytes_amd.lora_shrink`` and ``nn.Linear4bitLoRA.fused_shrink``.

* exact: on the operands of tests/lora_shrink_cases.py the output equals float64 rounded once, bit for bit, at every M from 1 to 16,
  with and without splits;
* a stacked call's parts are bit-equal to separate calls on the members and to the rows of the unsplit stacked call (ordinary data);
* ordinary data against float64 inside the derived bound (lora_shrink_cases.tolerance);
* the C entry point writes its part of a NaN-filled buffer and nothing else; determinism; graph capture; the module; opcheck.
The kernel is driven through the C entry point (which does not consult the predicate: a class the measurements exclude still computes
the documented result) and, wherever the predicate answers 1, through the op as well - with equal bits. The preconditions are asserted
on the CPU by tests/test_lora_shrink_host.py.
"""
import ctypes as ct
import functools

import pytest
import torch
import torch.nn.functional as TF

import exact_inputs as X
import lora_shrink_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _op():
    return torch.ops.bitsandbytes_amd.lora_shrink.default


def _supported(dtype, M, R, K) -> bool:
    return _bnb().lib.bnb_mi355x_lora_shrink_supported(C.DT_CODE[dtype], M, R, K) == 1


def _entry(x, a, out, splits=None):
    """bnb_mi355x_lora_shrink on x [M, K], a [R, K] into the M * R elements at ``out``."""
    M, K = x.shape
    n = 0 if splits is None else len(splits)
    table = (ct.c_int * n)(*splits) if n else None
    _bnb().lib.bnb_mi355x_lora_shrink(C.DT_CODE[x.dtype], x.data_ptr(), a.data_ptr(), out.data_ptr(), M, a.shape[0], K, table, n,
                                      torch.cuda.current_stream().cuda_stream)


def _shrink(x, a, splits=None):
    """The flat [M * R] output of the kernel; where the predicate serves the shape, the op's as well (asserted equal)."""
    M, R = x.shape[0], a.shape[0]
    flat = torch.empty(M * R, dtype=x.dtype, device=DEV)
    _entry(x, a, flat, splits)
    if _supported(x.dtype, M, R, x.shape[1]):
        assert torch.equal(_op()(x, a, None if splits is None else list(splits)).view(-1), flat)
    return flat


def _served_cell():
    """(M values, R, K) of one class the measurements keep, for the tests of the layers above the kernel."""
    ms, rs, ks = C.MUST_SERVE[0]
    return ms, rs[0], ks[0]


# ------------------------------------------------------------------------------------------ exact
@functools.lru_cache(maxsize=None)
def _prepared(case):
    """The case's operands on the device and its float64 reference, computed once and never written to."""
    x, a = C.build(case)
    return x.to(DEV), a.to(DEV), C.reference(x, a).to(DEV)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exact_at_every_batch_size(case):
    x, a, want = _prepared(case)
    failures = []
    for M in C.MS:
        flat = _shrink(x[:M], a, case.splits)
        if case.splits is None:
            got = [flat.view(M, case.R)]
            ref = [want[:M]]
        else:
            got = C.parts_of(flat, M, case.splits)
            ref = [want[:M, o:o + r] for o, r in zip(C.offsets(case.splits), case.splits)]
        for i, (g, w) in enumerate(zip(got, ref)):
            if not torch.equal(g, w):
                failures.append((M, i, X.first_mismatch(g.cpu(), w.cpu())))
    assert not failures, failures[:5]


# ------------------------------------------------------------------------------------------ stacked == separate
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [2752, 4096])
def test_stacked_parts_equal_separate_calls(K, dtype):
    """Ordinary data (sums that round): each part of a splits call has the bits of the member's own call and of the same rows of the
    unsplit stacked call - the order of the sum does not depend on R, on the row's place in A, on the splits or on the grid."""
    bnb = _bnb()
    gen = torch.Generator().manual_seed(K + 11)
    for splits in C.SPLITS:
        R = sum(splits)
        a = (torch.randn(R, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
        for M in (1, 5, 16):
            x = torch.randn(M, K, generator=gen).to(dtype).to(DEV)
            parts = C.parts_of(_shrink(x, a, splits), M, splits)
            unsplit = _shrink(x, a).view(M, R)
            assert not torch.equal(unsplit, torch.zeros_like(unsplit))
            public = bnb.lora_shrink(x, a, splits=splits)
            for i, (o, r) in enumerate(zip(C.offsets(splits), splits)):
                member = a[o:o + r].contiguous()
                alone = _shrink(x, member).view(M, r)
                assert torch.equal(parts[i], alone), (splits, M, i, X.first_mismatch(parts[i].cpu(), alone.cpu()))
                assert torch.equal(parts[i], unsplit[:, o:o + r]), (splits, M, i)
                assert public[i].shape == (M, r) and public[i].is_contiguous() and public[i].data_ptr() % 16 == 0
                if _supported(dtype, M, R, K):
                    assert torch.equal(public[i], alone) and torch.equal(bnb.lora_shrink(x, member), alone)


# ------------------------------------------------------------------------------------------ ordinary data against float64
@pytest.mark.parametrize("dtype", C.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", C.KS)
def test_ordinary_data_against_float64(K, dtype):
    """x ~ N(0, 1), A ~ N(0, 1 / K): inside lora_shrink_cases.tolerance around the float64 product. Every figure is printed."""
    gen = torch.Generator().manual_seed(K + 5)
    for R in (24, 136):
        a = (torch.randn(R, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
        for M in (1, 7, 16):
            x = torch.randn(M, K, generator=gen).to(dtype).to(DEV)
            want = x.double() @ a.double().t()
            got = _shrink(x, a).view(M, R)
            ratio = float(((got.double() - want).abs() / C.tolerance(want, x, a)).max())
            print(f"K={K} {dtype} R={R} M={M}: worst error / bound {ratio:.3f}")
            assert ratio <= 1.0, (K, dtype, R, M, ratio)


# ------------------------------------------------------------------------------------------ C entry point, determinism, capture
def test_c_entry_point_writes_its_part_only():
    """t inside a larger NaN-filled buffer: the part is fully written, everything outside it is still NaN, the result is the op's."""
    ms, R0, K = _served_cell()
    gen = torch.Generator().manual_seed(17)
    pad = 64
    for dtype in C.DTYPES:
        for R, splits in ((R0, None), (48, (16, 16, 16)), (160, (8, 128, 24))):
            a = (torch.randn(R, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
            for M in (ms[0], 3, 16):
                x = torch.randn(M, K, generator=gen).to(dtype).to(DEV)
                big = torch.full((pad + M * R + pad,), float("nan"), dtype=dtype, device=DEV)
                inner = big[pad:pad + M * R]
                assert inner.data_ptr() % 16 == 0
                _entry(x, a, inner, splits)
                torch.cuda.synchronize()
                assert not bool(torch.isnan(inner).any()), (dtype, R, splits, M)
                assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + M * R:]).all()), (dtype, R, splits, M)
                if _supported(dtype, M, R, K):
                    assert torch.equal(inner, _op()(x, a, None if splits is None else list(splits)).view(-1))
                else:
                    assert torch.equal(inner, _shrink(x, a, splits))


def test_thirty_launches_give_equal_bits():
    """Ordinary data: the bits do not depend on which wavefront or workgroup finishes first."""
    gen = torch.Generator().manual_seed(6)
    for M, R, K in ((1, 16, 4096), (9, 136, 2752), (16, 128, 34816)):
        x = torch.randn(M, K, generator=gen).bfloat16().to(DEV)
        a = (torch.randn(R, K, generator=gen) / K ** 0.5).bfloat16().to(DEV)
        first = _shrink(x, a)
        for _ in range(29):
            assert torch.equal(_shrink(x, a), first), (M, R, K)


def _random_weight(N, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=gen) * (3.0 / K ** 0.5)).to(dtype).to(DEV)


@pytest.mark.parametrize("M", [1, 4, 17])
def test_captured_layer_follows_x(M):
    """One torch.cuda.graph of lora_shrink + matmul_4bit_lora - the shrink kernel at 1 and 4 rows, its composition at 17 -, replayed
    with new contents in x's buffer: the host read nothing."""
    bnb = _bnb()
    _, r, K = _served_cell()
    N, s = 1408, 0.5
    dtype = torch.bfloat16
    assert _supported(dtype, M, r, K) == (M <= 16)
    packed, state = bnb.functional.quantize_4bit(_random_weight(N, K, dtype, 61), blocksize=64, quant_type="nf4", compress_statistics=True)
    gen = torch.Generator().manual_seed(63)
    A = (torch.randn(r, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)
    b = (torch.randn(N, r, generator=gen) * 0.5).to(dtype).to(DEV)
    bias = torch.randn(N, generator=gen).to(dtype).to(DEV)
    xs = [torch.randn(M, K, generator=gen).to(dtype).to(DEV) for _ in range(3)]
    call = lambda x: bnb.matmul_4bit_lora(x, packed, state, bnb.lora_shrink(x, A), b, s, bias=bias)
    with torch.no_grad():
        eager = [call(x) for x in xs]
        assert not torch.equal(eager[1], eager[2])
        if M <= 16:
            assert torch.equal(bnb.lora_shrink(xs[1], A).view(-1), _shrink(xs[1], A))
        else:
            assert torch.equal(bnb.lora_shrink(xs[1], A), TF.linear(xs[1], A))
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


# ------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("nested,dtype,bias", [(True, torch.bfloat16, True), (False, torch.float16, False)], ids=["nested-bf16-bias", "plain-fp16"])
def test_module_with_fused_shrink(nested, dtype, bias):
    bnb = _bnb()
    _, r, K = _served_cell()
    N, s = 2816, 2.0
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
        assert mod.fused_shrink is False
        Ad, Bd = A.to(DEV).to(dtype), B_l.to(DEV).to(dtype)
        other = (torch.randn(r, K, generator=gen) / K ** 0.5).to(dtype).to(DEV)    # a second layer that shares x: stacked with this one
        stacked = torch.cat([other, Ad]).contiguous()
        for lead in ((1,), (2, 3), (16,), (17,)):
            x = torch.randn(*lead, K, generator=gen).to(dtype).to(DEV)
            M = x.numel() // K
            default = mod(x)
            mod.fused_shrink = True
            got = mod(x)
            t = bnb.lora_shrink(x, Ad)
            if M <= 16:
                assert _supported(dtype, M, r, K) and torch.equal(t.view(-1), _shrink(x.view(M, K), Ad))
            want = bnb.matmul_4bit_lora(x, layer.weight, layer.weight.quant_state, t, Bd, s, bias=layer.bias.detach() if bias else None)
            assert got.shape == (*lead, N) and got.dtype == dtype and torch.equal(got, want), lead
            peft = layer(x) + TF.linear(TF.linear(x, Ad), Bd) * s
            assert float((got.float() - peft.float()).abs().max()) <= 2.0 ** -5 * float(peft.float().abs().max())
            # a caller that shrank a stacked group in one launch passes the member its part (served rows: the part has the bits of
            # the member's own call; 17 rows compose two BLAS calls of different widths, whose bits need not agree - its own t then)
            part = bnb.lora_shrink(x, stacked, splits=(r, r))[1] if M <= 16 else t
            assert part.shape == (*lead, r) and part.is_contiguous()
            assert torch.equal(mod(x, t=part), got), lead
            mod.fused_shrink = False
            assert torch.equal(mod(x), default) and torch.equal(mod(x, t=part), got)


# ------------------------------------------------------------------------------------------ opcheck
def test_opcheck():
    ms, r, K = _served_cell()
    a = (torch.randn(3 * r, K, device=DEV) / K ** 0.5).bfloat16()
    assert _supported(torch.bfloat16, 4, 3 * r, K)
    for lead in ((1,), (3,), (2, 2)):
        x = torch.randn(*lead, K, device=DEV).bfloat16()
        for kwargs in ({}, dict(splits=[r, r, r]), dict(splits=[3 * r])):
            torch.library.opcheck(_op(), (x, a), kwargs, test_utils=("test_schema", "test_faketensor"))
    assert _op()(x[:0], a).shape == (0, 2, 3 * r) and _op()(x[:0], a, [r, 2 * r]).shape == (0,)
    # what the fake kernel cannot see: a call without a kernel is an error, never another path
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(17, K, device=DEV).bfloat16(), a)
    with pytest.raises(ValueError, match="no kernel"):
        _op()(torch.randn(1, K, device=DEV), a.float())
    with pytest.raises(ValueError, match="no kernel"):
        _op()(x, a, [r + 4, 2 * r - 4])
