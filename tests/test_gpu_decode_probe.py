"""GPU: every packed byte value through the decode table of every fused 4-bit kernel, read back bit for bit
(tests/decode_probe_cases.py; preconditions on the CPU: tests/test_decode_probe_host.py).

One-hot activation rows (for the fused backward: gradient rows) make the matmul return the weights themselves,
``y[m, n] = round_T(code[nibble(n, k_m)] * s(n, k_m) * v_m)``: a single non-zero term per output, exact through any K split, workspace
and finalize launch. Hand-packed bytes put all 256 table entries - every NF4 and FP4 code in both nibbles - in front of every copy of
the table; every k of a case is probed once, as many rows per call as the family is meant for. Each family is forced the way its
geometry tests force it (the ``kernel=`` argument, the knob-1 codes of test_gpu_parity._forced, the public experts op, the C entry
point of the fused backward), and every call asserts the family that ran: a fall-back is a failure. No tolerance anywhere: integer
views must be equal, except that either zero passes where the want is zero.
"""
import os
import time

import pytest
import torch

import decode_probe_cases as P
from conftest import gpu_ready

pytestmark = pytest.mark.gpu

DEV = "cuda"
_id = lambda cs: cs.name


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


def _hip():
    from bitsandbytes_amd.backends import hip

    return hip


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host (set BNB_REQUIRE_GPU=1 to make this an error)", allow_module_level=False)
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    assert _bnb().lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    yield


def _report(cs, launches, pr_list, t0):
    reads = min(int(torch.bincount(pr.bytes.reshape(-1).long(), minlength=256).min()) for pr in pr_list) * len(pr_list)
    print(f"decode-probe family={cs.family} case={cs.name} launches={launches} min_reads_of_a_byte_value={reads} "
          f"wall_ms={(time.perf_counter() - t0) * 1e3:.0f}")


def _forward(cs, kernel):
    """The full probe of a dense forward case: K one-hot rows, ``cs.rows`` per call (0: one call), under the case's knob."""
    bnb, hip = _bnb(), _hip()
    t0 = time.perf_counter()
    pr = P.build(cs)
    N, K = cs.N, cs.K
    ks = torch.arange(K)
    x, v = P.one_hot_rows(ks, K, cs.dtype)
    want = pr.want_forward(ks, v).to(DEV)
    xd, packed = x.to(DEV), pr.packed.to(DEV)
    absmax, a8, code2, offset = pr.stats_args(DEV)
    code16 = pr.code16.to(DEV) if cs.quant == "code16" else None
    got = torch.empty(K, N, dtype=cs.dtype, device=DEV)
    step = cs.rows or K
    launches = 0
    try:
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, cs.knob)
        for m0 in range(0, K, step):
            m1 = min(K, m0 + step)
            hip._gemm_4bit_fused(xd[m0:m1], packed, (N, K), absmax, cs.blocksize, P.op_quant_type(cs), None, a8, code2, offset,
                                 kernel=kernel, out=got[m0:m1], code16=code16)
            ran = bnb.lib.bnb_mi355x_last_gemm_kernel()
            assert ran == P.FAMILY_ID[cs.family], f"rows {m0}..{m1}: kernel family {ran} ran, the case is about {cs.family}"
            launches += 1
    finally:
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, 0)
    mm = P.first_mismatch(pr, got.cpu(), want.cpu(), ks) if bool(P.mismatches(got, want).any()) else None
    assert mm is None, str(mm)
    _report(cs, launches, [pr], t0)


@pytest.mark.parametrize("cs", P.CASES["stream"], ids=_id)
def test_stream_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=1)


@pytest.mark.parametrize("cs", P.CASES["sm"], ids=_id)
def test_mfma_sm_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=2)


@pytest.mark.parametrize("cs", P.CASES["rt"], ids=_id)
def test_mfma_rt_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=2)


@pytest.mark.parametrize("cs", P.CASES["kq"], ids=_id)
def test_mfma_kq_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=2)


@pytest.mark.parametrize("cs", P.CASES["pc"], ids=_id)
def test_mfma_pc_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=2)


@pytest.mark.parametrize("cs", P.CASES["tall"], ids=_id)
def test_mfma_tall_kernel_decodes_every_byte(cs):
    _forward(cs, kernel=2)


@pytest.mark.parametrize("cs", P.CASES["experts"], ids=_id)
def test_experts_kernel_decodes_every_byte(cs):
    """matmul_4bit_experts' kernel builds its table in another shape than the others (literals per thread, no lane exchange): E = 3
    experts, one probe row per slot, every expert probed at every k, one masked slot per token (zeros, whatever its row holds)."""
    bnb, hip = _bnb(), _hip()
    t0 = time.perf_counter()
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default
    pr = P.build(cs)
    assert hip.gemm_4bit_experts_supported(cs.dtype, cs.E, cs.N, cs.K, cs.blocksize)
    x, ids, v = P.experts_probe(cs)
    want = P.experts_want(pr, ids, v)
    absmax, a8, code2, offset = pr.stats_args(DEV)
    y = op(x.to(DEV), pr.packed.to(DEV), [cs.E, cs.N, cs.K], absmax, ids.to(DEV), cs.blocksize, cs.quant, None, a8, code2, offset)
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == P.FAMILY_ID["experts"]
    assert y.shape == want.shape and y.dtype == cs.dtype
    T, S = ids.shape
    masked = ((ids < 0) | (ids >= cs.E)).reshape(-1)
    got, want = y.cpu().reshape(T * S, cs.N), want.reshape(T * S, cs.N)
    assert not bool(got[masked].any()), "a masked slot is not a row of zeros"
    keep = (~masked).nonzero().flatten()
    mm = P.first_mismatch(pr, got[keep], want[keep], torch.arange(T).repeat_interleave(S)[keep], expert=ids.reshape(-1)[keep])
    assert mm is None, str(mm)
    _report(cs, 1, [pr], t0)


@pytest.mark.parametrize("cs", P.CASES["grad_input"], ids=_id)
def test_fused_backward_decodes_every_byte(cs):
    """gemm_4bit_grad_input through its C entry point (the operator keeps the fused kernel to 128 rows; the entry point takes any M):
    ``g[m, m] = v_m`` returns the whole weight, row by row. 'single': the built-in plan of this shape, one N slice, no workspace.
    'sliced': the plan asks for one slice per 32-row block (the slice count of bnb_mi355x_set_tuning, the kernel's own sweep knob: the
    built-in plan slices from 1024 weight rows on) and the caller hands a workspace of three slabs - the entry point then runs as many
    slices as fit, three of unequal length, through the workspace and the finalize launch."""
    bnb, hip = _bnb(), _hip()
    lib = bnb.lib
    t0 = time.perf_counter()
    M, N, K = cs.N, cs.N, cs.K
    dt = hip._DT_CODE[cs.dtype]
    assert lib.bnb_mi355x_gemm_4bit_grad_input_supported(dt, M, N, K, cs.blocksize) == 1
    ns = torch.arange(N)
    g, v = P.one_hot_rows(ns, N, cs.dtype)
    gd = g.to(DEV)
    slab = M * K * 4
    probes = []
    try:
        if cs.plan == "sliced":
            lib.bnb_mi355x_set_tuning(0, N // 32, 0, 0)
            assert lib.bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) == (N // 32) * slab
            ws_bytes = 3 * slab
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        else:
            assert lib.bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K) == 0, "the built-in plan of this shape is one slice"
            ws, ws_bytes = None, 0
        for fi in range(cs.fills if cs.fill == "random" else 1):
            pr = P.build(cs, fi)
            probes.append(pr)
            packed = pr.packed.to(DEV)
            absmax, a8, code2, offset = pr.stats_args(DEV)
            out = torch.empty(M, K, dtype=cs.dtype, device=DEV)
            assert gd.data_ptr() % 16 == 0 and packed.data_ptr() % 16 == 0
            lib.bnb_mi355x_gemm_4bit_grad_input(dt, gd.data_ptr(), packed.data_ptr(), absmax.data_ptr(), hip._ptr(a8), hip._ptr(code2),
                                                hip._ptr(offset), out.data_ptr(), M, N, K, cs.blocksize, hip._QT_CODE[cs.quant],
                                                hip._ptr(ws), ws_bytes, hip._stream(gd))
            got = out.cpu()
            mm = P.first_mismatch(pr, got, pr.want_backward(ns, v), ns, backward=True)
            assert mm is None, f"fill {fi}: {mm}"
    finally:
        lib.bnb_mi355x_set_tuning(0, 0, 0, 0)
    _report(cs, len(probes) * (2 if cs.plan == "sliced" else 1), probes, t0)
