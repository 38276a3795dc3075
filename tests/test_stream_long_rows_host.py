"""CPU (-m "not gpu"): the operands and the case table behind tests/test_gpu_stream_long_rows.py.

* every case of tests/stream_long_rows_cases.py meets the exact-sum bound - asserted by its builder over EVERY weight row, here on the
  CPU at the sizes of the GPU module - so the GPU comparison needs no tolerance; the one family that cannot meet it (fp16 outputs with
  nested statistics) is the exact content of ``EXCLUDED``, and the bound does fail for it;
* the written bytes and statistics dequantize through the oracle to the W of the reference, bit for bit, on the first 64 rows of every
  case, and the nested statistics reconstruct the intended scales through the oracle's blockwise dequantize;
* the chunked float64 product is the unchunked one;
* every call of the table launches with the geometry written next to it (bnb_mi355x_stream_geometry, 256 CUs without a device): the
  phase counts, the clamped rows per workgroup, the wavefronts; the built-in route picks the streaming kernel where the table says
  ``public``; and the three-row gated call on the longest row is refused without a crash.
"""
import pytest
import torch

import exact_inputs as X
import large_offset_cases as L
import lora_cases as LC
import stream_long_rows_cases as C
from oracle import oracle as O

KINDS = sorted({(c.case.name, c.dtype, c.nested) for c in C.CALLS + C.FUSED_CALLS + C.RCAP2_FUSED}, key=str)
_PACKED = {}


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


def _built(name, dtype, nested, **kw):
    b = C.build(C.CASE[name], "cpu", dtype, nested, packed=_PACKED.get(name), **kw)
    if C.CASE[name].elements <= 1 << 24:
        _PACKED[name] = b.packed
    return b


@pytest.mark.parametrize("name,dtype,nested", KINDS, ids=[f"{n}-{str(d).split('.')[-1]}{'-nested' if z else ''}" for n, d, z in KINDS])
def test_case_meets_the_exact_sum_bound_and_dequantizes_through_the_oracle(name, dtype, nested):
    """``build`` asserts the bound over every weight row (the assertion decides, not the estimate of the case file); the first 64
    rows go through the oracle."""
    case = C.CASE[name]
    large = case in C.LARGE   # (no float64 copy of 3 * 10^8 weights on the CPU: the byte-arithmetic upper bound; the GPU module's build runs the other)
    b = _built(name, dtype, nested, with_reference=False, upper_bound=large)
    N, K, bs = case.N, case.K, case.blocksize
    if not large:
        upper = C.worst_sum_upper(b.packed, b.scale, N, K, bs)
        assert b.worst <= upper <= b.worst * 1.01, "the byte-arithmetic bound is the float64 one with every |x| = 1"
    print(f"{name} {dtype} nested={nested}: sum of |products| <= {b.worst} = {b.worst / b.unit:.0f} units of {b.unit} (2^24 = {2 ** 24})")
    assert b.worst > 0 and b.unit == C.unit_of(nested)
    assert set(b.x.unique().tolist()) == {-1.0, 0.0, 1.0} and torch.unique(b.x, dim=0).shape[0] == C.REF_ROWS
    rows = min(N, 64)
    w64 = L.rows64(b.packed, b.scale, K, bs, 0, rows)
    wdt = torch.bfloat16 if dtype == torch.float32 else dtype
    W = w64.to(wdt)
    assert torch.equal(W.double(), w64), "code x scale is not representable in the weight dtype"
    back = O.dequantize_4bit(b.packed[:rows * K // 2].view(-1, 1), b.scale[:rows * K // bs], bs, "fp4", (rows, K), wdt)
    assert back.dtype == wdt and torch.equal(back.view(torch.int16), W.view(torch.int16)), "the oracle reads other weights out of the bytes"
    heads = b.packed[:rows * K // 2].view(rows, K // 2)[:, ::bs // 2] >> 4
    assert bool((heads == 3).all()), "index 3 (code 1.0) sits at the head of every block, in the HIGH nibble"
    if nested:
        st = b.nest
        rec = O.dequantize_blockwise(st.absmax_8bit, st.absmax2, st.absmax_code, 256, torch.float32).float() + st.offset
        assert torch.equal(rec.flatten(), b.scale), "nested statistics do not reconstruct the intended scales"
        assert set(b.scale.unique().tolist()) == {t * a + C.NESTED_OFFSET for t in C.NESTED_TABLE for a in C.NESTED_ABSMAX2}
    else:
        lo, hi = C.EXPS
        assert set(torch.log2(b.scale).tolist()) == set(float(e) for e in range(lo, hi + 1)), "every exponent of the range is used"
        s2 = b.scale.view(N, K // bs)
        assert N == 1 or not torch.equal(s2[0], s2[1]), "two rows share a scale pattern"


def test_excluded_is_the_fp16_nested_family_and_it_does_fail():
    assert [c.name for c in C.EXCLUDED] == ["maxk-plain-float16-nested-M1", "maxk-plain-float16-nested-M2", "maxk-plain-float16-nested-M3",
                                            "maxk-plain-float16-nested-M4", "maxk-plain-float16-nested-M7"]
    assert all(c.case is C.MAXK and c.form == "plain" for c in C.EXCLUDED)
    assert all(c.dtype == torch.float16 and c.nested for c in C.EXCLUDED) and not any(c.dtype == torch.float16 and c.nested for c in C.CALLS)
    with pytest.raises(AssertionError, match="reaches the fp16 range"):
        _built("maxk", torch.float16, True, with_reference=False)
    # and exact_inputs' own ranges do not fit this K at all: |x| <= 4 against its six-value scale range, in units of its smallest product
    assert C.MAX_K * X.X_MAX * 0.5 * (sum(2.0 ** e for e in range(-2, 4)) / 6) / (2.0 ** -2 * 0.25) > 2 ** 24


def test_chunked_reference_is_the_float64_matmul():
    case = C.CASE["edge10272"]
    for dtype, nested in ((torch.bfloat16, False), (torch.bfloat16, True)):
        b = C.build(case, "cpu", dtype, nested)
        w64 = L.rows64(b.packed, b.scale, case.K, case.blocksize, 0, case.N)
        y64 = b.x.double() @ w64.t()
        assert torch.equal(b.y64, y64)
        assert torch.equal(b.ref(True, 4), (y64[:4] + b.bias.double()).to(dtype)) and not torch.equal(b.ref(True, 4), b.ref(False, 4))
        wdt = w64.to(dtype)
        assert b.worst == X.assert_exact_sums(wdt, b.x * 0 + b.x.abs().amax(dim=0), b.unit, dtype), "the bound of exact_inputs"


def test_adapter_operands_are_exact_on_top_of_the_base():
    t, stack, scalings = C.build_adapters(C.MAXK, torch.bfloat16, "cpu")
    assert t.shape == (C.REF_ROWS, C.LORA_R) and stack.shape == (2, C.MAXK.N, C.LORA_R) and scalings.tolist() == list(C.LORA_SCALINGS)
    for a in range(2):
        term = LC.adapter_term64(t, stack[a], float(scalings[a]))
        assert not bool((term / LC.ADAPTER_UNIT).frac().any()) and float(term.abs().max()) <= LC.ADAPTER_MAX
    assert LC.ADAPTER_UNIT % C.UNIT_PLAIN == 0, "adapter products are multiples of the base unit"
    assert max(max(v) for v in C.LORA_IDS.values()) == 2 and min(min(v) for v in C.LORA_IDS.values()) == 0   # both adapters, one id out of range


# ------------------------------------------------------------------------------------------ the table
def test_cases_are_the_issues():
    assert (C.MAXK.N, C.MAXK.K, C.MAXK.blocksize) == (8, 1046528, 64) and (C.RAGGED.N, C.RAGGED.K, C.RAGGED.blocksize) == (8, 1044512, 32)
    assert [(c.N, c.K, c.blocksize) for c in C.EDGES] == [(5, K, 32) for K in (32768, 32800, 20480, 20512, 10240, 10272)]
    assert (C.RCAP1.N, C.RCAP1.K) == (258, 1046528) and (C.RCAP2.N, C.RCAP2.K) == (514, 714752)
    assert C.RAGGED.K % 2048 == 32 and -(C.RAGGED.K // -2048) == 511
    plain = {(c.case.name, str(c.dtype).split(".")[-1] + ("-nested" if c.nested else ""), c.M) for c in C.CALLS}
    for kind in ("bfloat16", "float16", "bfloat16-nested"):
        assert {("maxk", kind, M) for M in (1, 2, 3, 4, 7)} <= plain
    assert {("maxk", "float32", M) for M in (1, 2, 4)} <= plain
    assert {("ragged", "bfloat16", 1), ("ragged", "bfloat16", 4), ("ragged", "float32", 4)} <= plain
    assert {("rcap1", "bfloat16", 4), ("rcap1", "bfloat16", 1), ("rcap2", "bfloat16", 4)} <= plain
    # the phase counts the issue lists
    P = {(c.case.name, c.dtype, c.M): c.geometry[3] for c in C.CALLS if not c.nested}
    assert [P[("maxk", torch.bfloat16, M)] for M in (1, 2, 3, 4, 7)] == [32, 64, 103, 103, 103]
    assert [P[("maxk", torch.float32, M)] for M in (1, 2, 4)] == [52, 103, 256]
    assert 103 * 5 - 511 == 4, "the last of 103 phases holds one segment of five"
    assert max(c.geometry[3] for c in C.CALLS) << 23 >= 1 << 31, "a phase count that sets the sign bit of the packed word"


@pytest.mark.parametrize("call", C.CALLS + C.FUSED_CALLS + C.RCAP2_FUSED, ids=lambda c: c.name)
def test_call_launches_in_its_regime(call):
    """The geometry of the launch, from the launch's own host code, is the one the case is there for; the route is the one the GPU
    module calls through."""
    lib = _lib()
    case, M = call.case, call.M
    N, K, bs = case.N, case.K, case.blocksize
    with C.tuned(lib, call.tuning):
        got = C.query(lib, call.form, call.dtype, M, N, K, bs)
        fused_ok = (call.form == "plain" or not call.public or
                    (lib.bnb_mi355x_gemm_4bit_gated_supported(2, M, N, K, bs) if call.form == "gated"
                     else lib.bnb_mi355x_gemm_4bit_lora_ids_supported(2, M, N, K, bs, 0, C.LORA_R, 2)) == 1)
    assert got is not None and fused_ok, "the streaming kernel's predicates refuse the call"
    assert got[:6] == call.geometry, f"(mb, waves, SW, P, R, grid_x) = {got[:6]}, the case is there for {call.geometry}"
    route = lib.bnb_mi355x_gemm_4bit_route(0, C.DT_CODE[call.dtype], M, N, K, bs)
    if call.form == "plain":
        assert (route == 0) == call.public or (bs == 32 and call.nested), "public: the built-in route picks the streaming kernel"
    elif call.public:
        assert route == 0
        if call.form == "gated":
            assert lib.bnb_mi355x_gemm_4bit_gated_supported(2, M, N, K, bs) == 1
        else:
            assert lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, N, K, bs, 0, C.LORA_R) == 1
            assert lib.bnb_mi355x_gemm_4bit_lora_ids_supported(2, M, N, K, bs, 0, C.LORA_R, 2) == 1
    else:
        # rcap2 at four rows: the fused forms follow the plain call's built-in route - the streaming MFMA kernel
        assert route == 1 and lib.bnb_mi355x_gemm_4bit_gated_supported(2, M, N, K, bs) == 1
        assert lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, N, K, bs, 0, C.LORA_R) == 1


def test_s349_is_rcap2s_regime_on_the_streaming_kernel():
    """The fused calls on 8 x 714752 at four rows are handed what rcap2's launch would be handed - mb, waves, SW, G, P, R and the LDS
    request - and differ from it in grid_x alone; under ROWS3 the row split asks for 3 and the slots clamp it to 2; and the built-in
    route leaves them on the streaming kernel."""
    lib = _lib()
    s, r = C.S349, C.RCAP2
    assert s.K == r.K == 714752 and -(s.K // -2048) == 349
    for form in ("plain", "gated", "lora", "lora_ids"):
        want = C.query(lib, form, torch.bfloat16, 4, r.N, r.K, 64)
        with C.tuned(lib, C.ROWS3):
            got = C.query(lib, form, torch.bfloat16, 4, s.N, s.K, 64)
        assert got[:5] + got[6:] == want[:5] + want[6:] and got[4] == 2 and (got[5], want[5]) == (4, 257), (form, got, want)
    with C.tuned(lib, C.ROWS3):
        assert C.query(lib, "lora", torch.bfloat16, 1, s.N, s.K, 64)[4] == 3, "one activation row: the three rows asked for fit"
    assert C.query(lib, "lora", torch.bfloat16, 4, s.N, s.K, 64)[4] == 1 and C.query(lib, "gated", torch.bfloat16, 4, s.N, s.K, 64)[4] == 2
    assert lib.bnb_mi355x_gemm_4bit_route(0, 2, 4, s.N, s.K, 64) == 0
    assert {c.form for c in C.FUSED_CALLS if c.case is s and c.tuning == C.ROWS3} == {"gated", "lora", "lora_ids"}


def test_clamped_rows_per_workgroup():
    """rcap1 / rcap2: the rows per workgroup the row split asks for (2 and 3) do not fit beside the image of four activation rows."""
    lib = _lib()
    for case, want_R, split in ((C.RCAP1, 1, 2), (C.RCAP2, 2, 3)):
        assert -(case.N // -L.DEFAULT_CUS) == split
        mb, waves, SW, P, R, grid, G, lds = C.query(lib, "plain", torch.bfloat16, 4, case.N, case.K, 64)
        S = -(case.K // -2048)
        fixed, ximg = 65536 + 1024 + 64, mb * SW * 2048 * 2
        assert R == want_R == (156 * 1024 - fixed - ximg - 16) // (S * mb * 4) < split, "R is the cap, below the split"
        assert S * mb * 4 >= 5584, "5.5 - 8 KiB of partial sums per weight row"
        # one activation row: unclamped
        assert C.query(lib, "plain", torch.bfloat16, 1, case.N, case.K, 64)[4] == split
    # (gate, up) pairs on rcap2: 3 -> 2, even; on rcap1 no pair fits
    assert C.query(lib, "gated", torch.bfloat16, 4, C.RCAP2.N, C.RCAP2.K, 64)[4] == 2
    assert C.query(lib, "gated", torch.bfloat16, 4, C.RCAP1.N, C.RCAP1.K, 64) is None


def test_three_row_gated_call_on_the_longest_row_is_refused():
    from bitsandbytes_amd.backends import hip

    case, dtype, M = C.UNSUPPORTED_GATED
    lib = _lib()
    assert lib.bnb_mi355x_gemm_4bit_gated_supported(C.DT_CODE[dtype], M, case.N, case.K, case.blocksize) == 0
    assert not hip.gemm_4bit_gated_supported(dtype, M, case.N, case.K, case.blocksize)
    assert C.query(lib, "gated", dtype, M, case.N, case.K, case.blocksize) is None
    assert C.query(lib, "plain", dtype, M, case.N, case.K, case.blocksize)[:6] == C._maxk_16bit(3), "the plain call of the composition is served"
    assert lib.bnb_mi355x_gemm_4bit_route(0, C.DT_CODE[dtype], M, case.N, case.K, case.blocksize) == 0
