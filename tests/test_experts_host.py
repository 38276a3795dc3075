"""CPU (-m "not gpu"): the host side of the expert-indexed fused matmul (bitsandbytes_amd::gemm_4bit_experts) - C ABI, geometry
query, op schema / fake kernel, argument checks - and the exact-input preconditions of every case tests/test_gpu_experts.py runs,
so that a case that does not qualify for a tolerance-free comparison fails here and not on the GPU."""
import ctypes as ct
import os
import re

import pytest
import torch

import exact_inputs as X
import experts_cases as C
from conftest import ROOT
from oracle import oracle as O

ORACLE_OPS = X.QuantOps(
    quantize_4bit=lambda W, bs: O.quantize_4bit(W, bs, "fp4"),
    dequantize_4bit=lambda q, absmax, bs, shape, dtype: O.dequantize_4bit(q, absmax, bs, "fp4", shape, dtype),
    dequantize_blockwise=lambda codes, absmax, table, bs: O.dequantize_blockwise(codes, absmax, table, bs, torch.float32),
)
SYMBOLS = ("bnb_mi355x_gemm_4bit_experts", "bnb_mi355x_gemm_4bit_experts_supported")
K_EXPERTS = 9


def _bnb():
    import bitsandbytes_amd as bnb

    return bnb


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_exported_and_listed():
    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert ce.lib, f"{ce.LIB_PATH} not built"
    dll = ct.CDLL(str(ce.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/bnb_mi355x.h"
        assert name in ce.EXPORTED_SYMBOLS
        assert hasattr(dll, name), f"{name} is not exported"
        assert getattr(ce.lib, name).argtypes is not None
    # the family code of bnb_mi355x_last_gemm_kernel() is documented in the header and in the integration notes
    assert re.search(r"\b9 expert-indexed kernel", header)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in notes for name in SYMBOLS)
    assert ce.lib.bnb_mi355x_version().decode() == "bitsandbytes_amd 0.1.1 gfx950"


def test_public_functions_exist():
    bnb = _bnb()
    assert callable(bnb.matmul_4bit_experts) and "matmul_4bit_experts" in bnb.__all__
    assert callable(bnb.nn.parametrize.matmul_4bit_experts)
    assert "gemm_4bit_experts" in dir(torch.ops.bitsandbytes_amd) or torch.ops.bitsandbytes_amd.gemm_4bit_experts is not None


def test_supported_is_pure_host_logic():
    """Answers without a device, for every geometry of the GPU cases - and refuses what the kernel does not serve."""
    lib = _bnb().lib
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    for case in C.EXACT_CASES:
        assert lib.bnb_mi355x_gemm_4bit_experts_supported(dt[case.dtype], case.E, case.N, case.K, case.blocksize) == 1, case.name
    for bs in (32, 64, 128, 256, 512, 1024, 2048, 4096):
        assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, 8, 64, 4096, bs) == 1
    assert lib.bnb_mi355x_gemm_4bit_experts_supported(2, 8, 64, 8192, 8192) == 1        # any power of two that divides K
    for dtype, E, N, K, bs in [(2, 8, 64, 4096 + 64, 128),   # K % blocksize != 0
                               (2, 8, 64, 4096, 16),         # blocksize below 32
                               (2, 8, 64, 4096 * 3, 96),     # not a power of two
                               (2, 0, 64, 4096, 64), (2, 8, 0, 4096, 64), (2, 8, 64, 0, 64),
                               (3, 8, 64, 4096, 64), (-1, 8, 64, 4096, 64),   # unknown dtype code
                               (2, 8, 64, 1 << 20, 64),      # rows beyond the segment-sum storage of a workgroup
                               (2, 70000, 64, 4096, 64)]:    # more experts than grid.y holds
        assert lib.bnb_mi355x_gemm_4bit_experts_supported(dtype, E, N, K, bs) == 0, (dtype, E, N, K, bs)
    from bitsandbytes_amd.backends import hip

    assert hip.gemm_4bit_experts_supported(torch.bfloat16, 8, 14336, 4096, 64)
    assert not hip.gemm_4bit_experts_supported(torch.float64, 8, 14336, 4096, 64)
    assert not hip.gemm_4bit_experts_supported(torch.bfloat16, 8, 14336, 4100, 64)


# ------------------------------------------------------------------------------------------ op schema, fake kernel
def _meta_args(E=8, N=96, K=128, bs=64, T=3, S=2, per_slot=False, idt=torch.int32, dtype=torch.bfloat16, nested=False, flat=False):
    m = "meta"
    blocks = E * N * K // bs
    A = torch.empty((T * S, K) if flat else ((T, S, K) if per_slot else (T, K)), dtype=dtype, device=m)
    B = torch.empty((E * N * K // 2, 1), dtype=torch.uint8, device=m)
    ids = torch.empty((T * S,) if flat else (T, S), dtype=idt, device=m)
    kw = {}
    if nested:
        absmax = torch.empty((-(blocks // -256),), dtype=torch.float32, device=m)
        kw = dict(absmax_8bit=torch.empty((blocks,), dtype=torch.uint8, device=m), absmax_code=torch.empty((256,), dtype=torch.float32, device=m),
                  absmax_offset=torch.empty((), dtype=torch.float32, device=m))
    else:
        absmax = torch.empty((blocks,), dtype=torch.float32, device=m)
    return [A, B, [E, N, K], absmax, ids, bs, "nf4"], kw


@pytest.mark.parametrize("per_slot", [False, True], ids=["x_TK", "x_TSK"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_fake_kernel_shapes(per_slot, idt, dtype, nested):
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default
    args, kw = _meta_args(per_slot=per_slot, idt=idt, dtype=dtype, nested=nested)
    y = op(*args, **kw)
    assert y.shape == (3, 2, 96) and y.dtype == dtype and y.device.type == "meta"
    bias = torch.empty((8, 96), dtype=dtype, device="meta")
    assert op(*args, bias=bias, **kw).shape == (3, 2, 96)


def test_fake_kernel_flat_ids_and_empty_call():
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default
    args, kw = _meta_args(flat=True)
    assert op(*args, **kw).shape == (6, 96)
    args, kw = _meta_args(T=0)
    assert op(*args, **kw).shape == (0, 2, 96)


def test_fake_kernel_rejects_bad_arguments():
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default

    def bad(mutate, **build):
        args, kw = _meta_args(**build)
        mutate(args, kw)
        with pytest.raises(RuntimeError):
            op(*args, **kw)

    def set_arg(i, v):
        return lambda a, kw: a.__setitem__(i, v)

    m = "meta"
    bad(set_arg(0, torch.empty((3, 2, 2, 128), dtype=torch.bfloat16, device=m)))             # x rank 4
    bad(set_arg(0, torch.empty((128,), dtype=torch.bfloat16, device=m)))                     # x rank 1
    bad(set_arg(0, torch.empty((3, 128), dtype=torch.int8, device=m)))                       # x dtype
    bad(set_arg(0, torch.empty((4, 128), dtype=torch.bfloat16, device=m)))                   # tokens of x != tokens of ids
    bad(set_arg(0, torch.empty((3, 3, 128), dtype=torch.bfloat16, device=m)))                # slots of x != slots of ids
    bad(set_arg(4, torch.empty((3, 2, 1), dtype=torch.int32, device=m)))                     # ids rank 3
    bad(set_arg(4, torch.empty((3, 2), dtype=torch.int16, device=m)))                        # ids dtype
    bad(set_arg(4, torch.empty((3, 2), dtype=torch.float32, device=m)))
    bad(set_arg(2, [8 * 96, 128]))                                                           # a 2D state
    bad(set_arg(2, [8, 128, 96]))                                                            # [E, K, N]: x inner dim is not shapeB[2]
    bad(set_arg(5, 48))                                                                      # blocksize not a power of two
    bad(set_arg(5, 16))
    bad(set_arg(6, "int4"))
    bad(set_arg(3, torch.empty((7,), dtype=torch.float32, device=m)))                        # absmax count
    bad(set_arg(1, torch.empty((5, 1), dtype=torch.uint8, device=m)))                        # packed bytes count
    bad(lambda a, kw: (a.__setitem__(2, [8, 96, 160]), a.__setitem__(0, torch.empty((3, 160), dtype=torch.bfloat16, device=m)),
                       a.__setitem__(1, torch.empty((8 * 96 * 80, 1), dtype=torch.uint8, device=m)),
                       a.__setitem__(3, torch.empty((8 * 96 * 160 // 64,), dtype=torch.float32, device=m))))   # K % blocksize != 0
    bad(lambda a, kw: kw.__setitem__("bias", torch.empty((96,), dtype=torch.bfloat16, device=m)))             # bias [N]
    bad(lambda a, kw: kw.__setitem__("bias", torch.empty((8, 97), dtype=torch.bfloat16, device=m)))
    bad(lambda a, kw: kw.__setitem__("bias", torch.empty((8, 96), dtype=torch.float32, device=m)))            # bias dtype
    bad(lambda a, kw: kw.__setitem__("absmax_code", None), nested=True)                                       # half a nested state
    bad(lambda a, kw: kw.__setitem__("absmax_8bit", torch.empty((5,), dtype=torch.uint8, device=m)), nested=True)
    bad(set_arg(0, torch.empty((6, 2, 128), dtype=torch.bfloat16, device=m)), flat=True)                      # [T, S, K] needs 2D ids


def test_public_api_rejects_what_is_out_of_scope():
    bnb = _bnb()
    F = bnb.functional

    def state(shape):
        blocks = shape[0] * shape[1] * (shape[2] if len(shape) > 2 else 1) // 64
        return F.QuantState(absmax=torch.empty(blocks, device="meta"), shape=torch.Size(shape), dtype=torch.bfloat16, blocksize=64,
                            quant_type="nf4", code=torch.empty(16, device="meta"))

    packed = torch.empty((8 * 96 * 128 // 2, 1), dtype=torch.uint8, device="meta")
    ids = torch.empty((3, 2), dtype=torch.int32, device="meta")
    x = torch.empty((3, 128), dtype=torch.bfloat16, device="meta")
    y = bnb.matmul_4bit_experts(x, packed, state([8, 96, 128]), ids)
    assert y.shape == (3, 2, 96)
    with pytest.raises(ValueError, match=r"\[E, K, N\]"):          # contraction over the unpacked dimension
        bnb.matmul_4bit_experts(x, packed, state([8, 128, 96]), ids)
    with pytest.raises(ValueError, match="3D"):
        bnb.matmul_4bit_experts(x, packed, state([8 * 96, 128]), ids)
    with pytest.raises(ValueError):
        bnb.matmul_4bit_experts(x, packed, None, ids)
    xg = torch.empty((3, 128), dtype=torch.bfloat16, device="meta", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        bnb.matmul_4bit_experts(xg, packed, state([8, 96, 128]), ids)
    with torch.no_grad():
        assert bnb.matmul_4bit_experts(xg, packed, state([8, 96, 128]), ids).shape == (3, 2, 96)


def test_op_traces_under_fake_tensor_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        args, kw = _meta_args(nested=True, per_slot=True, idt=torch.int64)
        args = [a.to("cpu") if isinstance(a, torch.Tensor) else a for a in args]   # (fake CPU tensors: no device needed)
        kw = {k: v.to("cpu") for k, v in kw.items()}
        y = torch.ops.bitsandbytes_amd.gemm_4bit_experts.default(*args, **kw)
        assert y.shape == (3, 2, 96)


# ------------------------------------------------------------------------------------------ id patterns, exact inputs
def test_id_patterns_are_what_they_say():
    gen = torch.Generator().manual_seed(5)
    for E in (4, 8, 128):
        for P in C.P_VALUES:
            T, S = C.TS_OF_P[P]
            assert T * S == P
            one = C.make_ids("one", P, E, gen)
            assert one.unique().numel() == 1 and 0 <= int(one[0]) < E
            d = C.make_ids("distinct", P, E, gen)
            assert d[: min(P, E)].unique().numel() == min(P, E) and int(d.min()) >= 0 and int(d.max()) < E
            ends = C.make_ids("ends", P, E, gen)
            assert set(ends.tolist()) <= {0, E - 1}
            r = C.make_ids("random", P, E, gen)
            assert int(r.min()) >= 0 and int(r.max()) < E
            mk = C.make_ids("masked", P, E, gen)
            assert set(mk.tolist()) <= set(range(E)) | {-1, E, E + 7}
    mk = C.make_ids("masked", 200, 8, gen)
    assert {-1, 8, 15} <= set(mk.tolist()) and len(set(mk.tolist()) & set(range(8))) == 8
    r = C.make_ids("random", 200, 8, gen)
    assert r.unique().numel() < 200   # repeats


def test_case_list_covers_what_the_kernel_distinguishes():
    names = [c.name for c in C.EXACT_CASES]
    assert len(set(names)) == len(names)
    shapes = {(c.E, c.N, c.K) for c in C.EXACT_CASES}
    assert {(8, 14336, 4096), (8, 4096, 14336), (128, 768, 2048), (128, 2048, 768), (16, 1024, 1024), (5, 130, 768), (4, 96, 96)} <= shapes
    medium = [c for c in C.EXACT_CASES if (c.E, c.N, c.K) == (16, 1024, 1024)]
    assert {(c.dtype, c.blocksize, c.nested) for c in medium} == {(d, b, n) for d in (torch.bfloat16, torch.float16, torch.float32)
                                                                   for b in (32, 64, 128) for n in (False, True)}
    assert all(c.K <= 4096 for c in C.EXACT_CASES if c.dtype == torch.float16)
    assert any(c.nested and (c.N * c.K // c.blocksize) % 256 != 0 for c in C.EXACT_CASES)   # second-level groups straddle experts


@pytest.mark.parametrize("case", C.EXACT_CASES, ids=lambda c: c.name)
def test_exact_preconditions_of_the_gpu_cases(case):
    """For every GPU case: the exact-sum bound holds for the worst (activation row, weight row) pair of the stack, with the bias
    (assert_exact_sums, inside build and once more here over the rows actually used); quantize / dequantize lose nothing and the
    nested reconstruction is the intended scale (oracle); and the oracle's gemm_4bit on one expert's slice of the un-nested statistics
    equals the float64 reference bit for bit."""
    ex = C.build_case(case)
    worst = X.assert_exact_sums(ex.W, ex.x, ex.unit, case.dtype, extra=float(X.BIAS_MAX))
    assert worst <= case.K * X.X_MAX * float(ex.W.abs().max()) + X.BIAS_MAX
    assert ex.W.shape == (case.E * case.N, case.K) and ex.x.shape == (C.MAX_ROWS, case.K) and ex.bias.shape == (case.E * case.N,)
    if case.large:
        # (the oracle's single-threaded quantizer over half a billion weights is left to the GPU test's check_quantization; one
        # expert's slice is checked here)
        rows = slice((case.E - 1) * case.N, case.E * case.N)
        packed, absmax = ORACLE_OPS.quantize_4bit(ex.W[rows], case.blocksize)
        bpe = case.N * case.K // case.blocksize
        assert torch.equal(absmax.flatten(), ex.scale[(case.E - 1) * bpe:])
    else:
        packed_all = X.check_quantization(ex, ORACLE_OPS)
        e = case.E - 1
        packed = packed_all.view(case.E, -1)[e].reshape(-1, 1)
        rows = slice(e * case.N, (e + 1) * case.N)
    bpe = case.N * case.K // case.blocksize
    scale_e = ex.scale[(case.E - 1) * bpe:case.E * bpe]
    y = O.gemm_4bit(ex.x[:5], packed, (case.N, case.K), scale_e, case.blocksize, "fp4", ex.bias[rows])[0]
    ref = (ex.x[:5].double() @ ex.W[rows].double().t() + ex.bias[rows].double()).to(case.dtype)
    assert torch.equal(y, ref), (case.name, X.first_mismatch(y, ref))
