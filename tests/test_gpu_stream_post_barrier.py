"""GPU: the in-lane row sum of the M = 1 streaming gemv (csrc/gemv4_stream.hip) equals the form it replaces, bit for bit.

The row sum of an item is finished in the vector unit and stored by lane 63 (wave_sum_n_lane63; before: four v_readlane, the rows
combined on SGPR values, stored by lane 0). The association is the same and fp32 addition commutes, so no output bit may move. What it
replaces is still in the library, in two places:
  * the sweep twins of the stream-tuning knob `nt` (bf16; NF4 fp32 absmax on the exact and the general instance, FP4 nested on the
    general one): 4 = readlane sum on the instance the launch selects, 5 = on the general instance where the exact one would run;
  * the two-row instances (MB = 2: readlane sum, for every type and table): a call with x stacked twice yields the one-row result in
    both rows - the kernel's sums do not depend on the launch geometry - and serves f16, FP4 and every other instance without a twin.
The fused forms are compared through what they are defined as: gated = silu(gate) * up of the plain rows, LoRA with t = 0 = plain.
Shapes: the smallest that reach each path - exact, exact under a CU-count override, general with R not a multiple of G, K = 8192 (four
segment columns), ragged last segments (lanes past the row's end)."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from conftest import gpu_ready

pytestmark = pytest.mark.gpu
BF16, F16 = 2, 1
DT_CODE = {torch.bfloat16: BF16, torch.float16: F16}


def _bnb():
    import bitsandbytes_amd as bnb

    assert bnb.lib, "libbitsandbytes_mi355x.so is not loaded: GPU tests must run on the native HIP path"
    return bnb


@pytest.fixture(scope="module", autouse=True)
def _knobs_at_rest():
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    yield
    _bnb().lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)
    _bnb().lib.bnb_mi355x_set_cu_count(0)


class knob:
    """``with knob(nt):`` - the calling thread's stream launches select the sweep twin of that value; always back to rest."""

    def __init__(self, nt):
        self.nt = nt

    def __enter__(self):
        _bnb().lib.bnb_mi355x_set_stream_tuning(0, 0, 0, self.nt, 0)

    def __exit__(self, *exc):
        _bnb().lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)


@functools.lru_cache(maxsize=None)
def _layer(N, K, bs, qt, nested, dtype):
    """One quantized matrix and its activation row, made once and never written to."""
    import bitsandbytes_amd.functional as F

    g = torch.Generator(device="cuda").manual_seed(N * 31 + K * 7 + bs)
    W = (torch.randn(N, K, device="cuda", generator=g) / K**0.5).to(dtype)
    q, st = F.quantize_4bit(W, blocksize=bs, quant_type=qt, compress_statistics=nested)
    x = torch.randn(1, K, device="cuda", generator=g).to(dtype)
    return q, st, x


def _plain(q, st, x):
    from bitsandbytes_amd.backends import hip

    if st.nested:
        return hip._gemm_4bit_fused(x, q, st.shape, st.state2.absmax, st.blocksize, st.quant_type, None, st.absmax, st.state2.code, st.offset, kernel=3)
    return hip._gemm_4bit_fused(x, q, st.shape, st.absmax, st.blocksize, st.quant_type, None, None, None, None, kernel=3)


def _exact(dtype, N, K, bs):
    return _bnb().lib.bnb_mi355x_gemv_4bit_stream_exact(DT_CODE[dtype], 1, N, K, bs, 0) == 1


TWIN_SHAPES = [  # (N, K, exact instance)
    (4096, 4096, True), (14336, 4096, True),       # exact
    (1376, 4096, False),                           # general
    (11008, 4096, False),                          # general, R = 43 not a multiple of G = 8
    (8192, 8192, False),                           # general, four segment columns
    (512, 11008, False), (256, 2112, False),       # general, ragged last segment (lanes past the row's end)
]


@pytest.mark.parametrize("nested", [False, True], ids=["nf4-bs64", "fp4-bs128-nested"])
@pytest.mark.parametrize("N,K,exact", TWIN_SHAPES, ids=lambda v: str(v))
def test_shipped_form_equals_the_readlane_twin(N, K, exact, nested):
    """bf16, the two sweep configurations: the built-in launch against the readlane twin on the instance the launch selects (nt = 4) and
    on the general instance (nt = 5), and against the built-in general instance (nt = 2)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q, st, x = _layer(N, K, 128 if nested else 64, "fp4" if nested else "nf4", nested, torch.bfloat16)
    if cus == 256 and not nested:
        assert _exact(torch.bfloat16, N, K, 64) == exact
    ref = _plain(q, st, x).clone()
    assert _bnb().lib.bnb_mi355x_last_gemm_kernel() == 1, "the streaming kernel did not run"
    for nt in (4, 5, 2):
        with knob(nt):
            got = _plain(q, st, x).clone()
        assert torch.equal(ref, got), f"{N} x {K}: knob nt = {nt} differs in {int((ref != got).sum())} of {N} outputs"
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 0


def test_exact_instance_under_a_cu_count_override():
    """512 x 4096 planned for 32 compute units: 16 rows per workgroup, the exact instance, 32 workgroups."""
    lib = _bnb().lib
    q, st, x = _layer(512, 4096, 64, "nf4", False, torch.bfloat16)
    lib.bnb_mi355x_set_cu_count(32)
    try:
        assert _exact(torch.bfloat16, 512, 4096, 64)
        ref = _plain(q, st, x).clone()
        for nt in (4, 5):
            with knob(nt):
                got = _plain(q, st, x).clone()
            assert torch.equal(ref, got), f"knob nt = {nt} differs in {int((ref != got).sum())} outputs"
    finally:
        lib.bnb_mi355x_set_cu_count(0)
    assert torch.equal(ref, _plain(q, st, x))  # (the 256-CU plan: 2 rows per workgroup, the general instance)


TWO_ROW_CELLS = [(dt, qt, bs, nested, N, K)
                 for dt in (torch.bfloat16, torch.float16)
                 for qt, bs, nested in (("nf4", 64, False), ("fp4", 64, False), ("fp4", 128, True))
                 for N, K in ((4096, 4096), (1376, 4096), (256, 2112))]
TWO_ROW_CELLS.append((torch.float16, "nf4", 64, False, 8192, 8192))  # (four segment columns: bf16 has its twin above)


@pytest.mark.parametrize("dtype,qt,bs,nested,N,K", TWO_ROW_CELLS,
                         ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, bool) else ("nested" if v else "fp32-absmax"))
def test_one_row_equals_the_two_row_instance(dtype, qt, bs, nested, N, K):
    """Every type and table: the one-row launch (in-lane sum, lane 63 stores) against both rows of the two-row launch on x stacked
    twice (MB = 2: readlane sum, lane 0 stores)."""
    q, st, x = _layer(N, K, bs, qt, nested, dtype)
    one = _plain(q, st, x)
    two = _plain(q, st, torch.cat([x, x]).contiguous())
    assert torch.equal(two[0], two[1])
    assert torch.equal(one[0], two[0]), f"differs in {int((one[0] != two[0]).sum())} of {N} outputs"


def test_gated_equals_silu_of_the_twin_rows():
    """8192 x 4096 interleaved (gate, up) rows, the exact gated instance: silu(gate) * up of the readlane twin's plain rows."""
    q, st, x = _layer(8192, 4096, 64, "nf4", False, torch.bfloat16)
    got = torch.ops.bitsandbytes_amd.gemm_4bit_gated(x, q, st.shape, st.absmax, st.blocksize, st.quant_type)
    with knob(4):
        y = _plain(q, st, x)
    want = TF.silu(y[:, 0::2]) * y[:, 1::2]
    assert torch.equal(got, want), f"differs in {int((got != want).sum())} of 4096 outputs"


@pytest.mark.parametrize("N,K", [(4096, 4096), (1376, 4096)], ids=lambda v: str(v))
def test_lora_with_a_zero_shrink_equals_the_twin(N, K):
    """r = 16, t = 0: T((acc + 0) + scaling * 0) is the plain result - of the readlane twin, exact and general LoRA instance."""
    q, st, x = _layer(N, K, 64, "nf4", False, torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(5)
    lora_b = torch.randn(N, 16, device="cuda", generator=g).bfloat16()
    lora_t = torch.zeros(1, 16, device="cuda", dtype=torch.bfloat16)
    got = torch.ops.bitsandbytes_amd.gemm_4bit_lora(x, q, st.shape, st.absmax, st.blocksize, st.quant_type, lora_t, lora_b, 2.0)
    with knob(4):
        want = _plain(q, st, x)
    assert torch.equal(got, want), f"differs in {int((got != want).sum())} of {N} outputs"
