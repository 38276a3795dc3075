"""CPU (-m "not gpu"): the helper behind tests/test_gpu_large_offsets.py, held against what the suite already trusts, and the size
limits of every matmul family written down as asserted facts.

* the builder of tests/large_offset_cases.py writes packed bytes and statistics directly (``quantize_4bit`` stops at 2^31 - 1
  elements). At sizes a CPU holds its bytes and statistics must dequantize through the oracle to exactly the W its reference uses,
  must BE what the oracle's quantizer makes of that W (nibble order, block heads, absmax), and its decode must read the bytes of
  ``exact_inputs.build`` - the construction it restates - back to that construction's W;
* the chunked reference equals the unchunked float64 matmul;
* the period assertion fails on a deliberately periodic scale pattern;
* the ledger: for every case and batch size of the GPU module the route query, the experts query and the fused-backward query answer
  what the source predicates say (restated in large_offset_cases).
"""
import pytest
import torch

import exact_inputs as X
import large_offset_cases as L
from oracle import oracle as O

SMALL = (
    (L.LargeCase("130x768", 130, 768, 64), torch.bfloat16, False),
    (L.LargeCase("130x768-nested", 130, 768, 64), torch.bfloat16, True),
    (L.LargeCase("130x768-fp16", 130, 768, 64), torch.float16, False),
    (L.LargeCase("96x96-bs32", 96, 96, 32), torch.bfloat16, False),
)
IDS = [c.name for c, _, _ in SMALL]


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _built(case, dtype, nested, **kw):
    return L.build(case, "cpu", dtype, nested, rows=9, **kw)


# ------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("case,dtype,nested", SMALL, ids=IDS)
def test_built_operands_dequantize_through_the_oracle(case, dtype, nested):
    """oracle.dequantize_4bit of the written bytes and statistics is the W of the helper's reference, bit for bit; the nested
    statistics reconstruct the intended scales through oracle.dequantize_blockwise; and the oracle's QUANTIZER turns that W back into
    the written bytes and scales - so a swapped nibble, a block without code 1.0 at its head or a scale at the wrong block fails."""
    b = _built(case, dtype, nested)
    N, K, bs = case.N, case.K, case.blocksize
    w64 = L.rows64(b.packed, b.scale, K, bs, 0, N)
    W = w64.to(dtype)
    assert torch.equal(W.double(), w64), "code x scale is not representable in the weight dtype"
    back = O.dequantize_4bit(b.packed.view(-1, 1), b.scale, bs, "fp4", (N, K), dtype)
    assert back.dtype == dtype and torch.equal(back.view(torch.int16), W.view(torch.int16)), "the oracle reads other weights out of the bytes"
    q, absmax = O.quantize_4bit(W, bs, "fp4")
    assert torch.equal(absmax.flatten(), b.scale), "quantize_4bit: absmax is not the constructed scale (a block head is not code 1.0)"
    assert torch.equal(q.flatten(), b.packed), "quantize_4bit packs the constructed W into other bytes (nibble order)"
    heads = b.packed.view(N, K // 2)[:, ::bs // 2] >> 4
    assert bool((heads == 3).all()), "index 3 (code 1.0) sits at the head of every block, in the HIGH nibble"
    used = torch.unique(torch.cat([b.packed >> 4, b.packed & 15]))
    assert used.tolist() == sorted(X.FP4_EXACT_INDICES), "every exact FP4 index is used and no other"
    if nested:
        st = b.nest
        rec = O.dequantize_blockwise(st.absmax_8bit, st.absmax2, st.absmax_code, 256, torch.float32).float() + st.offset
        assert torch.equal(rec.flatten(), b.scale), "nested statistics do not reconstruct the intended scales"
        assert st.absmax_code.tolist() == [X.NESTED_TABLE[i % 6] for i in range(256)] and float(st.offset) == X.NESTED_OFFSET
        assert set(torch.log2(st.absmax2).tolist()) <= set(float(e) for e in X.NESTED_ABSMAX2_EXP)
        assert bool((st.absmax2[1:] != st.absmax2[:-1]).all()), "neighbouring groups of 256 blocks share an absmax2"
    else:
        lo, hi = L.EXPS[dtype]
        assert set(torch.log2(b.scale).tolist()) == set(float(e) for e in range(lo, hi + 1)), "every exponent of the range is used"
    assert b.unit == (X.build(64, bs * 2, bs, dtype, nested, 1, 2, exps=L.EXPS[dtype]).unit), "the unit of exact_inputs"


@pytest.mark.parametrize("case,dtype,nested", SMALL, ids=IDS)
def test_decode_agrees_with_exact_inputs(case, dtype, nested):
    """The other direction: the operands of ``exact_inputs.build`` - quantized by the oracle - decode through the helper's look-up
    (high nibble = even element, the FP4 table, scale per block) to that construction's W."""
    ex = X.build(case.N, case.K, case.blocksize, dtype, nested, seed=5, rows=2, exps=L.EXPS[dtype])
    q, absmax = O.quantize_4bit(ex.W, case.blocksize, "fp4")
    assert torch.equal(absmax.flatten(), ex.scale)
    w64 = L.rows64(q.flatten(), ex.scale, case.K, case.blocksize, 0, case.N)
    assert torch.equal(w64, ex.W.double())
    # a row subset, as the GPU tests gather it
    rows = [0, case.N // 2, case.N - 1]
    assert torch.equal(L.gather_rows64(q.flatten(), ex.scale, case.K, case.blocksize, rows), ex.W.double()[rows])


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case,dtype,nested", SMALL, ids=IDS)
def test_chunked_reference_is_the_float64_matmul(case, dtype, nested):
    b = _built(case, dtype, nested, chunk_rows=7)    # (7 divides neither 130 nor 96: a ragged last chunk)
    w64 = L.rows64(b.packed, b.scale, case.K, case.blocksize, 0, case.N)
    y64 = b.x.double() @ w64.t()
    assert torch.equal(b.ref[False], y64.to(dtype)) and torch.equal(b.ref[True], (y64 + b.bias.double()).to(dtype))
    assert not torch.equal(b.ref[False], b.ref[True])
    assert b.worst == X.assert_exact_sums(w64.to(dtype), b.x, b.unit, dtype, extra=float(X.BIAS_MAX)), "the bound of exact_inputs"
    assert torch.unique(b.x, dim=0).shape[0] == b.x.shape[0] and float(b.x.abs().max()) == X.X_MAX
    assert not bool(b.bias.double().frac().any())
    one = L.build(case, "cpu", dtype, nested, rows=9, packed=b.packed)   # (the bytes of an earlier build, another chunking)
    assert torch.equal(one.ref[True], b.ref[True])
    assert L.first_wrong_row(b.ref[True], b.ref[True]) is None
    y = b.ref[True].clone()
    y[3, 17] += 1
    y[1, 40] += 1
    assert L.first_wrong_row(y, b.ref[True])[:2] == (17, 3)


def test_exact_sum_bound_holds_for_the_large_cases():
    """The bound that makes the GPU comparison tolerance-free, for the K of the cases, from the value ranges alone: K products of at
    most X_MAX x the largest |weight|, plus the bias, against 2^24 units (and the fp16 range where the case runs in fp16)."""
    for K in sorted({c.K for c in L.CASES} | {L.EXPERTS_K}):
        for dtype, nested in ((torch.bfloat16, False), (torch.bfloat16, True)):
            top = (max(X.NESTED_TABLE) * 2.0 ** max(X.NESTED_ABSMAX2_EXP) + X.NESTED_OFFSET) if nested else 2.0 ** L.EXPS[dtype][1]
            assert K * X.X_MAX * top + X.BIAS_MAX < 2.0 ** 24 * L.unit_of(dtype, nested), (K, dtype, nested)
    assert 8192 * X.X_MAX * 8.0 == 2.0 ** 22 * L.unit_of(torch.bfloat16, False)   # "within 2^22 units" at K = 8192


# ------------------------------------------------------------------------------------------ the period assertion
def test_scale_pattern_is_seeded_from_the_block_index():
    case = L.LargeCase("130x768", 130, 768, 64)
    a = L.plain_scale(case.N, case.K, 64, (-2, 3), "cpu")
    assert torch.equal(a, L.plain_scale(case.N, case.K, 64, (-2, 3), "cpu"))
    L.assert_not_periodic(a, case.K, 64)
    # the second rule at a size a CPU holds: "2^32 elements" = 64 rows
    L.assert_not_periodic(a, case.K, 64, wrap_elements=64 * case.K)
    h = L.mix(torch.arange(1 << 16))
    assert int(h.min()) >= 0 and int(h.max()) < 1 << 24 and torch.unique(h).numel() > 65000
    assert torch.equal(L.mix(torch.arange(1 << 16) + (1 << 32))[:4], L.mix(torch.tensor([1 << 32, (1 << 32) + 1, (1 << 32) + 2, (1 << 32) + 3])))
    assert not torch.equal(L.mix(torch.arange(1 << 16) + (1 << 26)), h), "indices 2^26 apart draw alike"


@pytest.mark.parametrize("period", [64, 1024])
def test_period_assertion_fails_on_a_periodic_pattern(period):
    """A pattern with a power-of-two period is the one under which a wrapped block index reads the scale it should have read: the
    assertion must refuse it, by either rule."""
    case = L.LargeCase("130x768", 130, 768, 64)
    periodic = lambda b: L.mix(b % period)  # noqa: E731
    s = L.plain_scale(case.N, case.K, 64, (-2, 3), "cpu", pattern=periodic)
    with pytest.raises(AssertionError, match=f"repeats with a period of {period} blocks"):
        L.assert_not_periodic(s, case.K, 64)
    with pytest.raises(AssertionError, match="repeats with a period"):
        L.build(case, "cpu", pattern=periodic, rows=4, with_reference=False)
    with pytest.raises(AssertionError, match="repeats with a period"):
        L.build(case, "cpu", nested=True, pattern=periodic, rows=4, with_reference=False)
    # the wrap rule alone: the rows past "2^32 elements" carry the scales of the rows that far before them
    good = L.plain_scale(case.N, case.K, 64, (-2, 3), "cpu")
    bpr = case.K // 64
    copied = good.clone()
    copied[96 * bpr:97 * bpr] = good[32 * bpr:33 * bpr]   # one row, 64 rows on
    with pytest.raises(AssertionError, match="a row past 2\\^32 elements"):
        L.assert_not_periodic(copied, case.K, 64, wrap_elements=64 * case.K)


# ------------------------------------------------------------------------------------------ the ledger
def test_cases_sit_where_the_issue_puts_them():
    c = L.CASE
    assert c["below31"].elements < 2 ** 31 <= c["below31"].elements + 8192
    assert 3 * 2 ** 30 < c["mid"].elements < 2 ** 32
    assert c["below32"].elements < 2 ** 32 <= c["below32"].elements + 8192
    assert c["above32"].elements == 2 ** 32 + 130 * 8192 and c["above32_k"].elements == 2 ** 32 + 130 * 4096   # 2^32 + 130 rows
    assert L.EXPERTS.elements == 2 ** 32 + 8 * L.EXPERTS_N * L.EXPERTS_K
    assert all(c.N % 16 for c in L.CASES), "an N that is no multiple of the row tiles"
    assert L.MS == (1, 2, 4, 8, 16, 17, 64)


def test_size_limits_are_what_the_source_predicates_say():
    """bnb_mi355x_gemm_4bit_route, ..._experts_supported and ..._grad_input_supported (pure host logic) for every case and batch size of
    the GPU module, against the predicates restated in large_offset_cases - and the facts that follow from them."""
    lib = _bnb().lib
    from bitsandbytes_amd.backends import hip

    for case in L.CASES + (L.BELOW32_BS32,):
        N, K, bs = case.N, case.K, case.blocksize
        for M in L.MS:
            got = lib.bnb_mi355x_gemm_4bit_route(0, 2, M, N, K, bs)
            assert got == L.expected_route(M, N, K, bs), (case.name, M, got)
            assert lib.bnb_mi355x_gemm_4bit_route(0, 1, M, N, K, bs) == got, "fp16 routes as bf16"
            assert M <= hip.fused_max_m(N, K, bs), "every batch size of the module takes the fused route"
            assert lib.bnb_mi355x_gemm_4bit_grad_input_supported(2, M, N, K, bs) == L.expected_grad_input(M, N, K, bs) == 0, "N % 64 != 0"
            whole = N & ~63
            assert lib.bnb_mi355x_gemm_4bit_grad_input_supported(2, M, whole, K, bs) == L.expected_grad_input(M, whole, K, bs) == int(bs >= 64)
        assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, 1, N, K, bs) == L.expected_experts(1, N, K, bs) == 1
    # one row: the streaming kernel below 2^32 elements; 2 ... 16 rows: the streaming MFMA kernel to its limit; 17 and 64: an MFMA kernel
    for name in ("below31", "mid", "below32"):
        c = L.CASE[name]
        assert [lib.bnb_mi355x_gemm_4bit_route(0, 2, M, c.N, c.K, 64) for M in L.MS] == [0, 1, 1, 1, 1, 1, 1], name
    # at and past 2^32 elements: not MFMA, at every M
    for name in ("above32", "above32_k"):
        c = L.CASE[name]
        assert all(lib.bnb_mi355x_gemm_4bit_route(0, 2, M, c.N, c.K, 64) == 0 for M in range(1, 130)), name
        assert lib.bnb_mi355x_gemm_4bit_workspace_bytes(0, 2, 64, c.N, c.K, 64) == 0
    assert lib.bnb_mi355x_gemm_4bit_route(0, 2, 8, 2 ** 19, 8192, 64) == 0 and lib.bnb_mi355x_gemm_4bit_route(0, 2, 8, 2 ** 19 - 1, 8192, 64) == 1
    # the epilogue forms follow the plain call's family below 2^32 and answer "no kernel" from there on (the ops raise ValueError, the
    # public functions compose)
    b32, a32 = L.CASE["below32"], L.CASE["above32"]
    for M in (1, 4):
        assert lib.bnb_mi355x_gemm_4bit_gated_supported(2, M, b32.N - 1, b32.K, 64) == 1
        assert lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, b32.N, b32.K, 64, 0, 16) == 1
        assert lib.bnb_mi355x_gemm_4bit_lora_ids_supported(2, M, b32.N, b32.K, 64, 0, 16, 3) == 1
        assert lib.bnb_mi355x_gemm_4bit_gated_supported(2, M, a32.N, a32.K, 64) == 0
        assert lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, a32.N, a32.K, 64, 0, 16) == 0
        assert lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, a32.N, a32.K, 64, 1, 16) == 0
        assert lib.bnb_mi355x_gemm_4bit_lora_ids_supported(2, M, a32.N, a32.K, 64, 0, 16, 3) == 0
        assert not hip.gemm_4bit_gated_supported(torch.bfloat16, M, a32.N, a32.K, 64)
        assert not hip.gemm_4bit_lora_supported(torch.bfloat16, M, a32.N, a32.K, 64, False, 16)
    # a grouped launch of the streaming kernel takes no member of 2^32 elements
    import ctypes as ct

    assert lib.bnb_mi355x_gemm_4bit_grouped_route(2, 2, (ct.c_int * 2)(4096, 4096), 1, 8192, 64) == 1
    assert lib.bnb_mi355x_gemm_4bit_grouped_route(2, 2, (ct.c_int * 2)(4096, a32.N), 1, 8192, 64) == 0
    # the expert stack of the GPU module: 2^32 elements plus 8 experts, served; E N rows stop at 2^31
    assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, L.EXPERTS_E, L.EXPERTS_N, L.EXPERTS_K, 64) == 1
    assert L.expected_experts(L.EXPERTS_E, L.EXPERTS_N, L.EXPERTS_K, 64) == 1
    assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, 32768, 65536, 8192, 64) == L.expected_experts(32768, 65536, 8192, 64) == 0
    assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, 32767, 65536, 8192, 64) == L.expected_experts(32767, 65536, 8192, 64) == 1
