"""CPU (-m "not gpu"): the exact-input builder of the routed sweep (tests/exact_inputs.py) keeps its promises for every case of
tests/test_gpu_routed_sweep.py - checked against the oracle, so that a mismatch on the GPU is a finding about a kernel and never
about the inputs."""
import pytest
import torch

import exact_inputs as X
from oracle import oracle as O

ORACLE_OPS = X.QuantOps(
    quantize_4bit=lambda W, bs: O.quantize_4bit(W, bs, "fp4"),
    dequantize_4bit=lambda q, absmax, bs, shape, dtype: O.dequantize_4bit(q, absmax, bs, "fp4", shape, dtype),
    dequantize_blockwise=lambda codes, absmax, table, bs: O.dequantize_blockwise(codes, absmax, table, bs, torch.float32),
)


def test_the_exact_codes_are_what_the_fp4_table_holds():
    table = O.get_4bit_code("fp4")
    assert [float(table[i]) for i in X.FP4_EXACT_INDICES] == list(X.FP4_EXACT_VALUES)


@pytest.mark.parametrize("case", X.SWEEP_CASES, ids=lambda c: c.name)
def test_builder_preconditions_and_oracle_equals_float64(case):
    """For every case of the routed sweep, at a handful of rows: quantize / dequantize lose nothing, the nested reconstruction is the
    intended scale, the exact-sum bound holds (asserted inside build) - and the oracle's gemm_4bit, handed the same statistics the
    GPU op gets, equals the float64 reference bit for bit, with and without bias."""
    ex = X.build(case.N, case.K, case.blocksize, case.dtype, case.nested, case.seed, rows=5, exps=case.exps)
    assert ex.W.dtype == case.dtype and ex.x.shape == (5, case.K) and ex.scale.numel() == case.N * case.K // case.blocksize
    packed = X.check_quantization(ex, ORACLE_OPS)
    absmax, a8, code, off = ex.stats_args("cpu")
    for with_bias in (False, True):
        y = O.gemm_4bit(ex.x, packed, (case.N, case.K), absmax, case.blocksize, "fp4", ex.bias if with_bias else None,
                        absmax_8bit=a8, absmax_code=code, absmax_offset=off)[0]
        ref = ex.reference(with_bias)
        assert y.dtype == ref.dtype and torch.equal(y, ref), (case.name, with_bias, X.first_mismatch(y, ref))


def test_the_bound_refuses_what_would_round():
    """The guard is alive: scales up to 2^13 over K = 4096 leave the 2^24-unit range, and build() says so."""
    with pytest.raises(AssertionError, match="2\\^24 units"):
        X.build(64, 4096, 64, torch.bfloat16, False, seed=1, rows=3, exps=(-12, 13))


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_backward_inputs_are_exact_too(nested):
    """The transposed product of the fused backward (g @ W) under the same bound, against the oracle's dequantize."""
    ex = X.build(1216, 384, 64, torch.bfloat16, nested, seed=3, rows=2)
    g, ref = X.grad_inputs(ex, 7, seed=4)
    packed = X.check_quantization(ex, ORACLE_OPS)
    Wd = O.dequantize_4bit(packed, ex.scale, 64, "fp4", (ex.N, ex.K), torch.float32)
    assert torch.equal((g.float() @ Wd).to(torch.bfloat16), ref)


def test_sweep_ms_leaves_no_gap():
    for fmax in (4, 16, 128, 512, 640, 1024):
        ms = X.sweep_ms(fmax)
        assert ms[: fmax + 1] == list(range(1, fmax + 2)) and len(ms) >= fmax + 3 and ms == sorted(set(ms))
        assert ms[-1] > 1024 and any(m % 64 == 1 and m > fmax + 1 for m in ms)
