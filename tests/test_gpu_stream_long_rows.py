"""GPU (-m gpu): the streaming gemv (csrc/gemv4_stream.hip) at its longest rows, bit for bit.

The kernel takes K up to 511 * 2048 = 1 046 528; every other test stops at K = 53 248, four phases of the ``kMulti`` loop. Here the
operands of tests/stream_long_rows_cases.py - exact by construction at 2^20 products per row (tests/test_stream_long_rows_host.py
asserts it) - run at 32 ... 256 phases: the activation image re-issued per phase, 511 partial sums per weight row and activation row
(8 KiB at four rows), the phase count in the top nine bits of a packed ``int`` - its sign bit from P = 256 on -, a last phase of one
segment, a last segment of 32 columns, the thresholds at which the instance changes, and the clamp of the rows per workgroup to the
partial-sum slots (R = 2 -> 1, 3 -> 2). Plain, gated, LoRA and mixed-adapter LoRA launches - the fused forms at four activation rows
and r_cap = 2 on 8 x 714752, where the built-in route keeps them on this kernel; the gated call that fits no row pair runs the
composition.

Every comparison is ``torch.equal`` against the float64 product of the constructed operands rounded once (the gated and adapter
epilogues as tests/test_gpu_ffn.py and tests/lora_multi_cases.py define them). Every call is preceded by a sentinel call of the generic
kernel and must leave ``bnb_mi355x_last_gemm_kernel()`` at the streaming kernel; every call's launch geometry, from
``bnb_mi355x_stream_geometry`` on this device, must be the regime its case is there for. One extra test at the end is no
streaming-kernel case: the fused calls on 514 x 714752 itself, which the router sends to another family, held to the same references.

The two large weights (270 M and 367 M elements, 135 and 184 MB packed) are built once each and dropped when another case is asked for.
"""
import os

import pytest
import torch
import torch.nn.functional as TF

import large_offset_cases as L
import lora_multi_cases as LM
import routed_sweep as S
import stream_long_rows_cases as C
from conftest import gpu_ready
from routed_sweep import DEV, FAMILY, K_GENERIC, K_SM, K_STREAM

pytestmark = pytest.mark.gpu

_CACHE = {}
_SENTINEL = []


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    assert _bnb().lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _built(case: C.LongCase, dtype=torch.bfloat16, nested=False) -> C.Built:
    """The case on the device, built once: the packed bytes are shared by a case's dtypes and kinds of statistics; a large case evicts
    every other case."""
    if case in C.LARGE and _CACHE.get("large") != case.name:
        _CACHE.clear()
        torch.cuda.empty_cache()
        _CACHE["large"] = case.name
    key = (case.name, dtype, nested)
    if key not in _CACHE:
        _CACHE[key] = C.build(case, DEV, dtype, nested, packed=_CACHE.get(("packed", case.name)))
        _CACHE[("packed", case.name)] = _CACHE[key].packed
    return _CACHE[key]


def _sentinel():
    if not _SENTINEL:
        _SENTINEL.append(S.Sentinel(K_GENERIC))
    _SENTINEL[0]()


def _ran_stream(what):
    family = _bnb().lib.bnb_mi355x_last_gemm_kernel()
    assert family == K_STREAM, f"{what}: the {FAMILY.get(family, family)} kernel ran (generic: no fused kernel was launched), not the streaming kernel"


def _in_regime(call: C.Call):
    """The launch geometry on THIS device is the one the case is there for (the table is written for 256 CUs)."""
    case = call.case
    with torch.cuda.device(DEV), C.tuned(_bnb().lib, call.tuning):
        got = C.query(_bnb().lib, call.form, call.dtype, call.M, case.N, case.K, case.blocksize)
    assert got is not None and got[:6] == call.geometry, f"{call.name}: (mb, waves, SW, P, R, grid_x) = {got and got[:6]}, the case is there for {call.geometry}"


def _assert_equal(y, want, what):
    assert y.shape == want.shape and y.dtype == want.dtype, (what, y.shape, y.dtype)
    if not torch.equal(y, want):
        n, m, got, ref = L.first_wrong_row(y, want)
        rows_wrong = int((y != want).any(dim=0).sum())
        raise AssertionError(f"{what}: {rows_wrong} of {want.shape[1]} output columns wrong; first: column {n}, activation row {m}: got {got!r}, want {ref!r}")


# ------------------------------------------------------------------------------------------ plain
@pytest.mark.parametrize("call", C.CALLS, ids=lambda c: c.name)
def test_plain_call_is_exact(call):
    """gemm_4bit with and without bias - through the public op where the built-in route picks the streaming kernel, else through
    kernel = 3 - against the float64 reference rounded once."""
    from bitsandbytes_amd.backends import hip

    _in_regime(call)
    case, M = call.case, call.M
    b = _built(case, call.dtype, call.nested)
    N, K, bs = case.N, case.K, case.blocksize
    absmax, a8, code, off = b.stats_args()
    for with_bias in (False, True):
        bias = b.bias if with_bias else None
        _sentinel()
        with C.tuned(_bnb().lib, call.tuning):
            if call.public and call.tuning is None:
                y = torch.ops.bitsandbytes.gemm_4bit.default(b.x[:M], b.packed.view(-1, 1), [N, K], absmax, bs, "fp4", bias, a8, code, off)
            else:   # (the tuning is the calling thread's: the Python entry point makes the library call on this thread)
                y = hip._gemm_4bit_fused(b.x[:M], b.packed.view(-1, 1), (N, K), absmax, bs, "fp4", bias, a8, code, off, kernel=0 if call.public else 3)
        _ran_stream(call.name)
        _assert_equal(y, b.ref(with_bias, M), f"{call.name} bias={int(with_bias)}")


# ------------------------------------------------------------------------------------------ fused forms at the longest row
def _gated_want(b: C.Built, with_bias: bool, M: int, N: int):
    y = b.ref(with_bias, M)[:, :N]
    return TF.silu(y[:, 0::2]) * y[:, 1::2]   # torch's kernels on T-valued tensors (tests/test_gpu_ffn.py)


def _lora_want(b: C.Built, with_bias: bool, M: int, t, stack, scalings, ids):
    return LM.expand_reference(b.y64[:M], b.bias.double() if with_bias else None, t[:M], stack, scalings, ids, b.dtype)


@pytest.mark.parametrize("call", C.FUSED_CALLS, ids=lambda c: c.name)
def test_fused_call_is_exact(call):
    """The gated, LoRA and mixed-adapter LoRA instances of ``kMulti`` through their ops: at K = 1 046 528, and at S = 349 with four
    activation rows, where the partial-sum slots hold two weight rows - the pairs' R = 2 at the defaults, and the clamp 3 -> 2 under the
    rows-per-workgroup knob (the ops' kernels are Python functions that call the library on this thread, whose tuning it is)."""
    _in_regime(call)
    tuned = lambda: C.tuned(_bnb().lib, call.tuning)  # noqa: E731
    case, M = call.case, call.M
    b = _built(case, call.dtype, call.nested)
    N, K, bs = case.N, case.K, case.blocksize
    packed = b.packed.view(-1, 1)
    if call.form != "gated":
        t, stack, scalings = C.build_adapters(case, call.dtype, DEV)
    for with_bias in (False, True):
        bias = b.bias if with_bias else None
        what = f"{call.name} bias={int(with_bias)}"
        if call.form == "gated":
            _sentinel()
            with tuned():
                y = torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(b.x[:M], packed, [N, K], b.scale, bs, "fp4", bias)
            _ran_stream(what)
            _assert_equal(y, _gated_want(b, with_bias, M, N), what)
        elif call.form == "lora":
            for a in (0, 1):
                _sentinel()
                with tuned():
                    y = torch.ops.bitsandbytes_amd.gemm_4bit_lora.default(b.x[:M], packed, [N, K], b.scale, bs, "fp4", t[:M], stack[a], C.LORA_SCALINGS[a], bias)
                _ran_stream(what)
                _assert_equal(y, _lora_want(b, with_bias, M, t, stack, scalings, [a] * M), f"{what} adapter {a}")
        else:
            ids = list(C.LORA_IDS[M])
            for idt in (torch.int32, torch.int64):
                _sentinel()
                idd = torch.tensor(ids, dtype=idt, device=DEV)
                with tuned():
                    y = torch.ops.bitsandbytes_amd.gemm_4bit_lora_ids.default(b.x[:M], packed, [N, K], b.scale, bs, "fp4", t[:M], stack, scalings, idd, bias)
                _ran_stream(what)
                want = _lora_want(b, with_bias, M, t, stack, scalings, ids)
                _assert_equal(y, want, f"{what} ids {ids} {idt}")
                for m, i in enumerate(ids):
                    if i >= stack.shape[0]:
                        assert torch.equal(y[m], b.ref(with_bias, M)[m]), "a row whose id is out of range is the plain row"


def test_three_row_gated_call_composes():
    """maxk at three rows: 80 KiB of activation image leave room for the partial sums of ONE weight row, so no (gate, up) pair fits a
    workgroup. The query refuses (it used to divide by zero), the op raises, and matmul_4bit_gated composes the plain call - the
    streaming kernel at 103 phases - with silu and a multiply: the bits of the float64 reference."""
    bnb = _bnb()
    from bitsandbytes_amd.backends import hip

    case, dtype, M = C.UNSUPPORTED_GATED
    b = _built(case, dtype, False)
    N, K, bs = case.N, case.K, case.blocksize
    assert not hip.gemm_4bit_gated_supported(dtype, M, N, K, bs)
    assert C.query(bnb.lib, "gated", dtype, M, N, K, bs) is None and C.query(bnb.lib, "plain", dtype, M, N, K, bs)[:6] == C._maxk_16bit(M)
    with pytest.raises(ValueError, match="no kernel"):
        torch.ops.bitsandbytes_amd.gemm_4bit_gated.default(b.x[:M], b.packed.view(-1, 1), [N, K], b.scale, bs, "fp4", None)
    Fn = bnb.functional
    state = Fn.QuantState(absmax=b.scale, shape=torch.Size((N, K)), code=Fn.get_4bit_type("fp4", device=DEV), blocksize=bs, quant_type="fp4", dtype=dtype)
    for with_bias in (False, True):
        bias = b.bias if with_bias else None
        _sentinel()
        y = bnb.matmul_4bit_gated(b.x[:M], b.packed, state, bias=bias)
        _ran_stream("the composition's plain call")
        plain = bnb.matmul_4bit(b.x[:M], b.packed, state, bias=bias)
        _assert_equal(plain, b.ref(with_bias, M), f"plain bias={int(with_bias)}")
        assert torch.equal(y, TF.silu(plain[..., 0::2]) * plain[..., 1::2]), "matmul_4bit_gated is not its unfused composition"
        _assert_equal(y, _gated_want(b, with_bias, M, N), f"composed gated bias={int(with_bias)}")


# ------------------------------------------------------------------------------------------ the fused forms on rcap2
def test_fused_calls_on_rcap2_are_exact_in_whichever_family_runs():
    """An extra (the streaming kernel's fused instances at S = 349, four rows and r_cap = 2 run in test_fused_call_is_exact, on s349):
    514 x 714752 ITSELF at four rows through the public functions. The fused entry points follow the plain call's built-in route, which
    today sends this size and M to the streaming MFMA kernel; whichever fused family runs is recorded and held to the same references
    (the generic kernel - no fused launch - is the one failure)."""
    bnb = _bnb()
    for call in C.RCAP2_FUSED:
        _in_regime(call)
    case, M = C.RCAP2, 4
    b = _built(case)
    N, K, bs = case.N, case.K, case.blocksize
    t, stack, scalings = C.build_adapters(case, torch.bfloat16, DEV)
    Fn = bnb.functional
    state = Fn.QuantState(absmax=b.scale, shape=torch.Size((N, K)), code=Fn.get_4bit_type("fp4", device=DEV), blocksize=bs, quant_type="fp4",
                          dtype=torch.bfloat16)
    _sentinel()
    y = bnb.matmul_4bit_gated(b.x[:M], b.packed, state, bias=b.bias)
    family = bnb.lib.bnb_mi355x_last_gemm_kernel()
    print(f"[long-rows] rcap2 gated M=4: family {FAMILY.get(family, family)}")
    assert family in (K_STREAM, K_SM)
    _assert_equal(y, _gated_want(b, True, M, N), "rcap2 gated")
    _sentinel()
    y = bnb.matmul_4bit_lora(b.x[:M], b.packed, state, t[:M], stack[1], C.LORA_SCALINGS[1], bias=b.bias)
    family = bnb.lib.bnb_mi355x_last_gemm_kernel()
    print(f"[long-rows] rcap2 lora M=4: family {FAMILY.get(family, family)}")
    assert family in (K_STREAM, K_SM)
    _assert_equal(y, _lora_want(b, True, M, t, stack, scalings, [1] * M), "rcap2 lora")
