"""GPU (-m gpu): the STANDALONE quantize / dequantize kernels over the whole range of block scales, bit for bit against the oracle.

The parity tests of these kernels (test_gpu_parity.py) draw randn * 0.02 ... 0.3, so every absmax lies in about [2^-6, 2^1], and
compare dequantized values with results below 2^-126 treated as zero. Here (inputs: tests/scale_range_cases.py; their properties:
tests/test_scale_range_host.py):
  * dequantize_4bit in every launch form, dequantize_4bit_rows, the one-launch nested dequantize and dequantize_blockwise see every
    code under 1532 scales - every fp32 exponent, subnormal scales, inf and NaN - for every output type: subnormal fp16 / bf16 / fp32
    results, fp16 overflow and NaN must come out as the reference's scalar path gives them;
  * quantize_4bit sees every finite positive bf16 / fp16 value as the absmax of a block whose other elements are the representable
    values around absmax * bound, the same in fp32 at 1529 scales, and ragged tail blocks (a true division, absmax clamped to 1e-38)
    holding elements whose code tells the tail rule from the full-block rule;
  * quantize_blockwise sees the values around absmax * midpoint of the dynamic map, at every absmax whose reciprocal is finite.
Every comparison is scale_range_cases.same_bits: NaN equals NaN, either zero passes where a zero is wanted, nothing else is forgiven.
"""
import time

import pytest
import torch

import scale_range_cases as C
from conftest import gpu_ready
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
QTS = ("nf4", "fp4")
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    # (as test_gpu_parity.py) A host without any AMD GPU device node: skip. A GPU box whose torch cannot see the device, or whose
    # native library did not load, must FAIL - never pass on a fallback.
    import os

    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    import bitsandbytes_amd as bnb

    assert bnb.lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


def _F():
    import bitsandbytes_amd.functional as F

    return F


class _knob:
    """`with _knob(v): ...` - bnb_mi355x_set_tuning(v, 0, 0, 0) for the duration, reset on the way out."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        _lib().bnb_mi355x_set_tuning(self.v, 0, 0, 0)

    def __exit__(self, *exc):
        _lib().bnb_mi355x_set_tuning(0, 0, 0, 0)
        return False


def _same(got, want, what, blocksize=None, scale=None):
    msg = C.first_mismatch(got.cpu().reshape(want.shape), want, blocksize, scale)
    assert msg is None, f"{what}: {msg}"


_CACHE = {}


def _cached(key, make):
    """One input per session: the cases of a parametrised test share it (and leave it unchanged)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------ dequantize_4bit
@pytest.mark.parametrize("blocksize", [64, 4096])
@pytest.mark.parametrize("dtype", C.OUT_DTYPES, ids=IDS.get)
@pytest.mark.parametrize("quant_type", QTS)
def test_dequantize_4bit_every_code_under_every_scale(quant_type, dtype, blocksize):
    """The built-in form, every forced form (general kernel with 4 / 8 packed dwords per lane and round 4's form for 16-bit outputs;
    general kernel and the line-contiguous kernel with 2 / 8 units per lane for fp32) and the row gather over all rows."""
    t0 = time.time()
    inp = _cached(("dq4", quant_type, blocksize), lambda: C.dequant4_input(quant_type, blocksize, C.scales()))
    want = O.dequantize_4bit(inp.packed, inp.absmax, blocksize, quant_type, (inp.n,), dtype)
    q, am = inp.packed.to(DEV), inp.absmax.to(DEV)
    op = torch.ops.bitsandbytes.dequantize_4bit.default
    _same(op(q, am, blocksize, quant_type, (inp.n,), dtype), want, "built-in form", blocksize, inp.absmax)
    for knob in (14, 18, 40) if dtype != torch.float32 else (40, 32, 38):
        with _knob(knob):
            got = op(q, am, blocksize, quant_type, (inp.n,), dtype)
        _same(got, want, f"forced form {knob}", blocksize, inp.absmax)
    row_len = max(512, blocksize)
    rows = inp.n // row_len
    got = torch.ops.bitsandbytes_amd.dequantize_4bit_rows.default(q, am, torch.arange(rows, device=DEV), row_len, blocksize, quant_type, dtype)
    assert got.shape == (rows, row_len)
    _same(got, want, "dequantize_4bit_rows", blocksize, inp.absmax)
    print(f"\n{quant_type}/{IDS[dtype]}/bs{blocksize}: {C.census(want)}; 5 forms in {time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------ nested statistics
@pytest.mark.parametrize("dtype", C.OUT_DTYPES, ids=IDS.get)
@pytest.mark.parametrize("quant_type", QTS)
def test_dequantize_4bit_nested_every_q8_under_every_second_level_scale(quant_type, dtype):
    """One launch (bitsandbytes_amd::dequantize_4bit_nested through F.dequantize_4bit(q, state)) on a hand-built state: every 8-bit
    code under 383 second-level scales, five offsets. Equal to the oracle (scale = code2[q] * absmax2, rounded, + offset, rounded)
    and, bit for bit, to the three-operator sequence on the same state."""
    F = _F()
    t0 = time.time()
    inp = _cached(("nested", quant_type), lambda: C.nested_input(quant_type, 64))
    q = inp.packed.to(DEV).reshape(-1, 1)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    for off in C.OFFSETS:
        st = inp.state(off, dtype, DEV)
        assert st.nested and st.absmax.dtype == torch.uint8
        got = F.dequantize_4bit(q, st)
        assert got.shape == (inp.n,) and got.dtype == dtype
        scale = inp.scale(off)
        want = O.dequantize_4bit(inp.packed, scale, 64, quant_type, (inp.n,), dtype)
        am = torch.ops.bitsandbytes.dequantize_blockwise.default(st.absmax, st.state2.absmax, st.state2.code, 256, torch.float32)
        am = am + st.offset
        _same(am, scale, f"offset {off!r}: dequantize_blockwise + offset", 256, inp.absmax2)
        seq = torch.ops.bitsandbytes.dequantize_4bit.default(q, am, 64, quant_type, [inp.n], dtype)
        _same(got, want, f"offset {off!r}: one launch against the oracle", 64, scale)
        assert torch.equal(got.view(it), seq.view(it)), f"offset {off!r}: one launch differs from the three-operator sequence"
        print(f"\n{quant_type}/{IDS[dtype]} offset {off!r}: {C.census(want)}")
    print(f"{time.time() - t0:.2f} s")


# ------------------------------------------------------------------------------------------ dequantize_blockwise
@pytest.mark.parametrize("blocksize", [64, 4096])
@pytest.mark.parametrize("dtype", C.OUT_DTYPES, ids=IDS.get)
def test_dequantize_blockwise_every_code_under_every_scale(dtype, blocksize):
    """256 codes x 1532 scales: the built-in form (four units per lane) and the first form (knob 6)."""
    inp = _cached(("dq8", blocksize), lambda: C.dequant8_input(blocksize, C.scales()))
    want = O.dequantize_blockwise(inp.codes, inp.absmax, inp.code, blocksize, dtype)
    q, am, code = inp.codes.to(DEV), inp.absmax.to(DEV), inp.code.to(DEV)
    op = torch.ops.bitsandbytes.dequantize_blockwise.default
    _same(op(q, am, code, blocksize, dtype), want, "built-in form", blocksize, inp.absmax)
    with _knob(6):
        got = op(q, am, code, blocksize, dtype)
    _same(got, want, "first form (knob 6)", blocksize, inp.absmax)
    print(f"\n{IDS[dtype]}/bs{blocksize}: {C.census(want)}")


# ------------------------------------------------------------------------------------------ quantize_4bit
def _quantize_4bit_equals_oracle(blocks, blocksize, quant_type, what):
    F = _F()
    A = blocks.reshape(-1)
    q_o, am_o = O.quantize_4bit(A, blocksize, quant_type)
    q, st = F.quantize_4bit(A.to(DEV), blocksize=blocksize, quant_type=quant_type)
    _same(st.absmax, am_o, f"{what}: absmax")
    bad = (q.cpu().reshape(-1) != q_o.reshape(-1)).nonzero().reshape(-1)
    if bad.numel():
        i = int(bad[0])
        blk = 2 * i // blocksize
        a = A[blk * blocksize].float().reshape(1)
        raise AssertionError(
            f"{what}: {bad.numel()} of {q_o.numel()} packed bytes differ; first: byte {i} = elements {2 * i}, {2 * i + 1} "
            f"({float(A[2 * i])!r}, {float(A[2 * i + 1])!r}) of block {blk}, absmax {float(a[0])!r} (0x{int(C.bits_of(a)[0]):08X}): "
            f"got 0x{int(q.reshape(-1)[i]):02X}, want 0x{int(q_o.reshape(-1)[i]):02X}")
    return am_o


def _absmax_census(am):
    sub = int(((am != 0) & (am < 2.0**-126)).sum())
    rsub = int(((1.0 / am) < 2.0**-126).sum())
    return f"{am.numel()} blocks, {sub} with a subnormal absmax, {rsub} with a subnormal reciprocal"


@pytest.mark.parametrize("quant_type", QTS)
@pytest.mark.parametrize("dtype16", C.DT16, ids=IDS.get)
def test_quantize_4bit_every_16bit_absmax_on_the_bounds(dtype16, quant_type):
    """Blocksize 64, the whole frontier: every finite positive value of the type as absmax, the seven representable values around
    absmax * bound for every positive bound, both signs."""
    blocks = _cached(("front", dtype16, quant_type), lambda: C.quant4_frontier(dtype16, quant_type))
    am = _quantize_4bit_equals_oracle(blocks, 64, quant_type, f"{IDS[dtype16]}/{quant_type}")
    print(f"\n{IDS[dtype16]}/{quant_type}: {blocks.numel()} elements, {_absmax_census(am)}")


@pytest.mark.parametrize("blocksize", [32, 256, 4096])
@pytest.mark.parametrize("quant_type", QTS)
@pytest.mark.parametrize("dtype16", C.DT16, ids=IDS.get)
def test_quantize_4bit_16bit_absmax_subset_other_blocksizes(dtype16, quant_type, blocksize):
    """The kernel is templated on the blocksize and the block-max reduction differs (lanes of a wavefront, wavefronts through LDS, two
    chunks per block): every 16th absmax and all of the two lowest and the two highest exponents."""
    blocks = C.quant4_frontier(dtype16, quant_type, blocksize=blocksize, absmax_bits=C.absmax16_subset(dtype16))
    am = _quantize_4bit_equals_oracle(blocks, blocksize, quant_type, f"{IDS[dtype16]}/{quant_type}/bs{blocksize}")
    print(f"\n{IDS[dtype16]}/{quant_type}/bs{blocksize}: {blocks.numel()} elements, {_absmax_census(am)}")


@pytest.mark.parametrize("quant_type", QTS)
def test_quantize_4bit_fp32_at_every_scale_on_the_bounds(quant_type):
    """fp32 inputs: 1529 scales (every exponent, subnormal ones, those whose reciprocal is subnormal), the values within 8 ulps of
    scale * bound for all 15 bounds."""
    blocks = C.quant4_frontier_f32(quant_type)
    am = _quantize_4bit_equals_oracle(blocks, 64, quant_type, f"fp32/{quant_type}")
    print(f"\nfp32/{quant_type}: {blocks.numel()} elements, {_absmax_census(am)}")


@pytest.mark.parametrize("dtype16,quant_type", [(torch.bfloat16, "nf4"), (torch.bfloat16, "fp4"), (torch.float16, "fp4")],
                         ids=["bf16-nf4", "bf16-fp4", "fp16-fp4"])
def test_quantize_4bit_tail_blocks_divide_by_the_clamped_absmax(dtype16, quant_type):
    """The ragged tail block is its own path: a true division by max(absmax, 1e-38), which is also what is stored. One call per case:
    three ordinary blocks, then a tail that keeps an element whose code differs under the full-block rule or without the clamp
    (fp16 / NF4 has no such element: tests/test_scale_range_host.py)."""
    F = _F()
    cases = C.tail_cases(dtype16, quant_type)
    assert 0 < len(cases) <= 256
    clamped = 0
    for c in cases:
        q_o, am_o = O.quantize_4bit(c.A, 64, quant_type)
        q, st = F.quantize_4bit(c.A.to(DEV), blocksize=64, quant_type=quant_type)
        what = f"tail of {c.tail} elements, first {float(c.A[192])!r}, flipping element {c.j} = {float(c.A[192 + c.j])!r}"
        _same(st.absmax, am_o, f"{what}: absmax")
        assert torch.equal(q.cpu(), q_o), f"{what}: got {q.cpu().reshape(-1)[96:].tolist()}, want {q_o.reshape(-1)[96:].tolist()}"
        clamped += int(float(c.A[192]) < float(am_o[3]))
    print(f"\n{IDS[dtype16]}/{quant_type}: {len(cases)} tails, {clamped} with the absmax below the clamp")


# ------------------------------------------------------------------------------------------ quantize_blockwise
@pytest.mark.parametrize("variant", [1, 2], ids=["cell-table", "byte-table"])
@pytest.mark.parametrize("dtype", C.OUT_DTYPES, ids=IDS.get)
def test_quantize_blockwise_at_every_scale_on_the_midpoints(dtype, variant):
    """Both 8-bit encoders, forced one at a time: the representable values within 2 ulps of absmax * midpoint for the 255 midpoints of
    the dynamic map and of absmax * bin edge where the code really changes (scale_range_cases.quant8_edges), at every absmax of the
    scale set that the input type holds and whose reciprocal is finite."""
    blocks = _cached(("q8", dtype), lambda: C.quant8_frontier(dtype))
    code = C.dynamic_map()
    A = blocks.reshape(-1)
    q_o, am_o = O.quantize_blockwise(A, code, 256)
    with _knob(variant):
        q, am = torch.ops.bitsandbytes.quantize_blockwise.default(A.to(DEV), code.to(DEV), 256)
    _same(am, am_o, "absmax")
    _same(q, q_o, "codes", 256, am_o)
    print(f"\n{IDS[dtype]}: {A.numel()} elements, {_absmax_census(am_o)}")
