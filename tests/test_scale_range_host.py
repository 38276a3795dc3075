"""CPU: the inputs of tests/scale_range_cases.py have the properties tests/test_gpu_scale_range.py relies on - asserted, not assumed.

  * the oracle (pinned to the live reference by tests/test_oracle_pinning.py) equals the float64 / separate-fp32 restatements on every
    builder, dtype and quant type: it is well-defined at subnormal, overflowing, inf and NaN scales;
  * the 16-bit frontiers make every finite positive value the absmax of some block and put adjacent representable values on either
    side of every positive bound;
  * they hold thousands of elements whose code tells a division from a multiplication by the reciprocal, and every tail case keeps one;
  * the dequantize inputs hold subnormal, infinite and NaN wants for every output type, an fp16 overflow and an fp16 result that
    rounds up into the smallest normal.
"""
import numpy as np
import pytest
import torch

import scale_range_cases as C
from oracle import oracle as O

QTS = ("nf4", "fp4")
IDS16 = {torch.bfloat16: "bf16", torch.float16: "fp16"}
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


def _check(got, want, blocksize=None, scale=None):
    msg = C.first_mismatch(got, want, blocksize, scale)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------ the sets
def test_scale_sets():
    s = C.scales()
    bits = C.bits_of(s)
    assert s.numel() == 1532 and np.unique(bits).size == 1532 and not (bits >> 31).any()
    assert set((bits[:-2] >> 23).tolist()) == set(range(255)) and set((bits[:-2] & 0x7FFFFF).tolist()) == set(C.MANTISSAS)
    assert torch.isinf(s[-2]) and torch.isnan(s[-1])
    f = C.finite_scales()
    assert f.numel() == 1530 and bool(torch.isfinite(f).all())
    assert int(((f != 0) & (f < 2.0**-126)).sum()) == 5, "subnormal scales"
    r = C.reciprocal_finite_scales()
    assert bool(torch.isfinite(1.0 / r).all()) and bool((r != 0).all())
    assert set(f.tolist()) - set(r.tolist()) == {x for x in f.tolist() if x == 0 or x <= 2.0**-128}
    assert int(((1.0 / r) < 2.0**-126).sum()) >= 6, "scales whose reciprocal is subnormal"
    am2 = C.nested_absmax2()
    assert am2.numel() == 64 * 6 - 1 and bool((am2 > 0).all()) and bool(torch.isfinite(am2).all())
    assert set((C.bits_of(am2) >> 23).tolist()) == set(range(0, 255, 4))


def test_same_bits_forgives_nan_payload_and_sign_of_a_wanted_zero_only():
    a = torch.tensor([1.0, float("nan"), 0.0, -0.0, 1e-40])
    assert C.same_bits(a, a.clone())
    nan2 = C.f32_from_bits([0x7FC00001])[0]
    b = a.clone()
    b[1], b[2], b[3] = nan2, -0.0, 0.0
    assert C.same_bits(b, a)
    for i, v in ((0, 1.0000001), (4, 0.0), (4, 1.0000021e-40), (2, 1e-45), (1, float("inf"))):
        c = a.clone()
        c[i] = v
        assert not C.same_bits(c, a), (i, v)
        assert f"element {i}" in C.first_mismatch(c, a, 2, torch.ones(3))
    z = torch.zeros(3)
    assert not C.same_bits(z, torch.tensor([0.0, 1e-45, 0.0])), "a wanted subnormal is not a zero"
    h = torch.tensor([6e-8, 0.0], dtype=torch.float16)
    assert not C.same_bits(torch.zeros(2, dtype=torch.float16), h) and C.same_bits(h, h.clone())
    assert not C.same_bits(torch.tensor([1, 2], dtype=torch.uint8), torch.tensor([1, 3], dtype=torch.uint8))


# ------------------------------------------------------------------------------------------ dequantize inputs
@pytest.mark.parametrize("blocksize", [64, 4096])
@pytest.mark.parametrize("quant_type", QTS)
def test_dequant4_input_layout_and_oracle(quant_type, blocksize):
    inp = C.dequant4_input(quant_type, blocksize, C.scales())
    assert inp.n % C.LINES_TILE == 0 and inp.n % 4096 == 0 and inp.packed.numel() * 2 == inp.n and inp.absmax.numel() * blocksize == inp.n
    # every block holds every nibble in both positions, every scale has all 256 byte values under it
    live = C.scales().numel() * max(512, blocksize)
    by_block = inp.packed[: live // 2].reshape(-1, blocksize // 2)
    for half in (by_block >> 4, by_block & 15):
        assert bool((torch.sort(half[:, :16], dim=1)[0] == torch.arange(16, dtype=torch.uint8)).all())
    by_scale = inp.packed[: live // 2].reshape(C.scales().numel(), -1)
    assert bool((torch.sort(by_scale[:, :256], dim=1)[0] == torch.arange(256, dtype=torch.uint8)).all())
    assert np.array_equal(np.unique(C.bits_of(inp.absmax[: live // blocksize])), np.unique(C.bits_of(C.scales())))
    for dt in C.OUT_DTYPES:
        want = C.dequant4_want(inp, dt)
        _check(O.dequantize_4bit(inp.packed, inp.absmax, blocksize, quant_type, (inp.n,), dt), want, blocksize, inp.absmax)
        _content(want, dt)


def _content(want, dt):
    """Subnormal, infinite and NaN wants; for fp16 an overflow of a finite product and a result that rounds up into 2^-14."""
    w = want.float()
    lim = 2.0**-14 if dt == torch.float16 else 2.0**-126
    assert int(((w != 0) & (w.abs() < lim)).sum()) > 1000 and int(torch.isinf(w).sum()) > 100 and int(torch.isnan(w).sum()) > 100, C.census(want)


@pytest.mark.parametrize("quant_type", QTS)
def test_dequant4_input_fp16_overflow_and_round_up_into_the_smallest_normal(quant_type):
    inp = C.dequant4_input(quant_type, 64, C.scales())
    p32 = C.dequant4_want(inp, torch.float32)
    h = C.dequant4_want(inp, torch.float16)
    assert int((torch.isfinite(p32) & torch.isinf(h)).sum()) > 1000, "finite fp32 products that overflow fp16"
    assert int(((p32.abs() < 2.0**-14) & (h.float().abs() == 2.0**-14)).sum()) > 0, "fp32 products below 2^-14 that round up to it"
    assert int(((p32.abs() < 65536.0) & torch.isinf(h)).sum()) > 0, "products below 2^16 that round up to inf"


@pytest.mark.parametrize("blocksize", [64, 4096])
def test_dequant8_input_and_oracle(blocksize):
    inp = C.dequant8_input(blocksize, C.scales())
    assert inp.n == C.scales().numel() * max(256, blocksize)
    assert bool((torch.sort(inp.codes.reshape(C.scales().numel(), -1)[:, :256], dim=1)[0] == torch.arange(256, dtype=torch.uint8)).all())
    for dt in C.OUT_DTYPES:
        want = C.dequant8_want(inp, dt)
        _check(O.dequantize_blockwise(inp.codes, inp.absmax, inp.code, blocksize, dt), want, blocksize, inp.absmax)
        _content(want, dt)


@pytest.mark.parametrize("quant_type", QTS)
def test_nested_input_and_oracle(quant_type):
    inp = C.nested_input(quant_type, 64)
    assert inp.absmax8.numel() * 64 == inp.n and inp.absmax2.numel() * 256 == inp.absmax8.numel()
    assert bool((inp.absmax8.reshape(-1, 256) == torch.arange(256, dtype=torch.uint8)).all()), "every q8 in every group of 256 blocks"
    plain = O.dequantize_blockwise(inp.absmax8, inp.absmax2, inp.code2, 256, torch.float32)
    kinds = set()
    for off in C.OFFSETS:
        scale = inp.scale(off)
        _check(plain + torch.tensor(off, dtype=torch.float32), scale, 256, inp.absmax2)
        # two roundings: the sum is not the single rounding of the exact code2 * absmax2 + offset everywhere
        fused = (inp.code2.double()[inp.absmax8.long()] * inp.absmax2.double().repeat_interleave(256) + float(np.float32(off))).float()
        if off in (0.03, -0.03):
            assert int((fused != scale).sum()) > 100, "no scale tells one fused multiply-add from two roundings"
        if bool(((scale != 0) & (scale.abs() < 2.0**-126)).any()):
            kinds.add("subnormal")
        if bool((scale < 0).any()):
            kinds.add("negative")
        for dt in C.OUT_DTYPES:
            _check(O.dequantize_4bit(inp.packed, scale, 64, quant_type, (inp.n,), dt), inp.want(off, dt), 64, scale)
    assert kinds == {"subnormal", "negative"}


# ------------------------------------------------------------------------------------------ quantize_4bit frontiers
_FRONTIER = {}


def _frontier(dtype16, quant_type):
    key = (dtype16, quant_type)
    if key not in _FRONTIER:
        _FRONTIER[key] = C.quant4_frontier(dtype16, quant_type)
    return _FRONTIER[key]


@pytest.mark.parametrize("quant_type", QTS)
@pytest.mark.parametrize("dtype16", C.DT16, ids=IDS16.get)
def test_frontier16_oracle_coverage_and_discriminating_power(dtype16, quant_type):
    blocks = _frontier(dtype16, quant_type)
    count = C.all_absmax16(dtype16).size
    assert count == (32639 if dtype16 == torch.bfloat16 else 31743) and blocks.shape == (2 * count, 64)
    q_o, am_o = O.quantize_4bit(blocks.reshape(-1), 64, quant_type)
    q_r, am_r = C.quantize4_restated(blocks.reshape(-1), 64, quant_type)
    assert torch.equal(q_o, q_r)
    _check(am_o, am_r)
    # every finite positive value of the type is the absmax of a block (both of its blocks)
    _check(am_o, blocks[:, 0].float())
    assert np.array_equal(np.unique(C.bits_of(blocks[:, 0])), C.all_absmax16(dtype16).astype(np.uint16))
    # adjacent representable values on either side of every positive bound, for every absmax from the clamp up (zero and a itself
    # are the outer pair, so the type has values on both sides; below 1e-38 - 108 bf16 values - the divisor is the clamp, not a, and
    # a * b is no bound of the block: those blocks are there for the clamp itself)
    a_bits, cand = C.frontier_candidates(dtype16, quant_type)
    b, _ = C.bounds4(quant_type)
    first_pos = int((b <= 0).sum())
    a = C.from_bits16(a_bits, dtype16).float()
    pos = C.position(C.scaled_multiply(C.from_bits16(cand, dtype16).reshape(cand.shape), a[:, None, None]), quant_type).numpy()
    clamped = a.numpy() < np.float32(C.TINY)
    assert int(clamped.sum()) == (108 if dtype16 == torch.bfloat16 else 0)
    assert (C.position(C.scaled_multiply(a, a), quant_type).numpy()[~clamped] == 15).all()
    for i in range(cand.shape[1]):
        lo, hi = pos[:, i, :-1], pos[:, i, 1:]
        step = (cand[:, i, 1:] - cand[:, i, :-1]) == 1
        straddle = (step & (lo <= first_pos + i) & (hi > first_pos + i)).any(axis=1) | clamped
        assert straddle.all(), f"bound {first_pos + i}: no adjacent pair around it for absmax bits 0x{int(a_bits[~straddle][0]):04X}"
    # the candidates are in the blocks
    have = C.bits_of(blocks).reshape(count, 128).astype(np.int64)
    assert all(np.isin(cand[r].reshape(-1), have[r]).all() for r in range(0, count, 997))
    # discriminating power
    n_flip = int(C.flips(blocks, quant_type).sum())
    n_same_divisor = int(C.flips(blocks, quant_type, same_divisor=True).sum())
    print(f"\n{IDS16[dtype16]}/{quant_type}: {blocks.numel()} elements, {n_flip} flip between multiply and divide, {n_same_divisor} of them with the clamped divisor")
    if (dtype16, quant_type) == (torch.float16, "nf4"):
        assert n_flip == 0, "recorded as 0: no fp16 ratio lies within an ulp of an NF4 bound (exempt from the tail test)"
    else:
        assert n_flip >= 5000
    if quant_type == "fp4":
        assert n_same_divisor >= 5000


@pytest.mark.parametrize("quant_type", QTS)
@pytest.mark.parametrize("dtype16", C.DT16, ids=IDS16.get)
@pytest.mark.parametrize("blocksize", [32, 256, 4096])
def test_frontier16_other_blocksizes_oracle(dtype16, quant_type, blocksize):
    sub = C.absmax16_subset(dtype16)
    shift = 7 if dtype16 == torch.bfloat16 else 10
    assert np.isin(C.all_absmax16(dtype16)[::16], sub).all()
    for e in (0, 1, (0x7F80 >> 7) - 2 if dtype16 == torch.bfloat16 else (0x7C00 >> 10) - 2, (0x7F80 >> 7) - 1 if dtype16 == torch.bfloat16 else (0x7C00 >> 10) - 1):
        assert int(((sub >> shift) == e).sum()) == (1 << shift) - (1 if e == 0 else 0)
    blocks = C.quant4_frontier(dtype16, quant_type, blocksize=blocksize, absmax_bits=sub)
    assert blocks.shape[1] == blocksize and blocks.shape[0] % sub.size == 0
    q_o, am_o = O.quantize_4bit(blocks.reshape(-1), blocksize, quant_type)
    q_r, am_r = C.quantize4_restated(blocks.reshape(-1), blocksize, quant_type)
    assert torch.equal(q_o, q_r)
    _check(am_o, am_r)
    _check(am_o, blocks[:, 0].float())


@pytest.mark.parametrize("quant_type", QTS)
def test_frontier_f32_oracle(quant_type):
    blocks = C.quant4_frontier_f32(quant_type)
    assert blocks.shape == (1529 * 5, 64)
    q_o, am_o = O.quantize_4bit(blocks.reshape(-1), 64, quant_type)
    q_r, am_r = C.quantize4_restated(blocks.reshape(-1), 64, quant_type)
    assert torch.equal(q_o, q_r)
    _check(am_o, am_r)
    _check(am_o, blocks[:, 0])
    assert int(((am_o != 0) & (am_o < 2.0**-126)).sum()) == 5 * 5 and int(((1.0 / am_o) < 2.0**-126).sum()) >= 5 * 6
    # both sides of every bound, for every normal absmax
    b, order = C.bounds4(quant_type)
    pos = C.position(C.scaled_multiply(blocks, blocks[:, :1]), quant_type).reshape(1529, -1)
    big = (blocks[::5, 0] >= 2.0**-126).numpy()
    assert int(big.sum()) == 1524
    for i in range(15):
        if quant_type == "fp4" and float(b[i]) == 0.0:
            continue  # between the two zeros: the codes on either side are FP4's two zeros, and position 8 needs s > 0 (checked below)
        both = ((pos == i).any(dim=1) & (pos == i + 1).any(dim=1)).numpy()
        assert both[big].all(), f"bound {i}"
    assert bool((pos == 8).any()) and bool((pos == 7).any())


@pytest.mark.parametrize("quant_type", QTS)
@pytest.mark.parametrize("dtype16", C.DT16, ids=IDS16.get)
def test_tail_cases_keep_a_flipping_element_and_oracle(dtype16, quant_type):
    cases = C.tail_cases(dtype16, quant_type)
    if (dtype16, quant_type) == (torch.float16, "nf4"):
        assert cases == []
        return
    assert len(cases) == 256 if quant_type == "fp4" else 200 <= len(cases) <= 256
    kinds = {"same divisor": 0, "clamped divisor": 0}
    for c in cases:
        assert c.A.numel() == 3 * 64 + c.tail and 0 < c.j < c.tail < 64
        tail = c.A[3 * 64:].reshape(1, -1)
        assert bool(C.flips(tail, quant_type)[0, c.j])
        kinds["same divisor" if bool(C.flips(tail, quant_type, same_divisor=True)[0, c.j]) else "clamped divisor"] += 1
        q_o, am_o = O.quantize_4bit(c.A, 64, quant_type)
        q_r, am_r = C.quantize4_restated(c.A, 64, quant_type)
        assert torch.equal(q_o, q_r)
        _check(am_o, am_r)
        assert float(am_o[3]) == max(float(tail[0, 0]), float(np.float32(C.TINY)))
    print(f"\n{IDS16[dtype16]}/{quant_type}: {kinds}, tails of {min(c.tail for c in cases)} ... {max(c.tail for c in cases)} elements")
    assert {c.tail % 2 for c in cases} == {0, 1}
    if quant_type == "fp4":
        assert kinds["same divisor"] >= 100, "tails in which only the division itself tells the two rules apart"
    if dtype16 == torch.bfloat16:
        assert kinds["clamped divisor"] >= 1, "tails whose absmax lies below the clamp"


# ------------------------------------------------------------------------------------------ quantize_blockwise frontier
@pytest.mark.parametrize("dtype", C.OUT_DTYPES, ids=IDS.get)
def test_quant8_frontier_oracle(dtype):
    blocks = C.quant8_frontier(dtype)
    a = C.quant8_absmax(dtype)
    assert blocks.shape == (a.numel() * 10, 256) and blocks.dtype == dtype
    code = C.dynamic_map()
    q_o, am_o = O.quantize_blockwise(blocks.reshape(-1), code, 256)
    q_r, am_r = C.quantize8_restated(blocks.reshape(-1), code, 256)
    _check(am_o, am_r)
    _check(am_o, blocks[:, 0].float())
    _check(q_o, q_r, 256, am_o)
    assert np.unique(q_o.numpy()).size >= 192, "three quarters of the map's codes are produced"
    if dtype != torch.float16:
        assert int(((am_o != 0) & (am_o < 2.0**-126)).sum()) >= 5 and int(((1.0 / am_o) < 2.0**-126).sum()) >= 5 * 5
    # the values around the bin edges are where a division and a multiplication by the reciprocal part ways (around the midpoints
    # themselves almost none do: the rule compares bin values, and the edge of a bin lies hundreds of fp32 ulps from the midpoint)
    e = C.quant8_edges(code)
    mid = (0.5 * (code[:-1] + code[1:])).double()
    assert float((e - mid).abs().max()) <= 1.0 / 65535.0 + 1e-7 and float((e - mid).abs().median()) > 2.0**-20
    n_flip = int(C.quant8_flips(blocks, code).sum())
    print(f"\n{IDS[dtype]}: {blocks.numel()} elements, {a.numel()} absmax values, {n_flip} elements flip between multiply and divide")
    # (16-bit inputs: their steps are 2^13 / 2^16 fp32 ulps wide, none lands within an ulp of an edge - 0 measured, nothing asserted)
    if dtype == torch.float32:
        assert n_flip >= 5000
