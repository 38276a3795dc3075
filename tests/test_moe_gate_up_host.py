"""CPU: the host side of the token-major MoE gate / up launch - C ABI, predicate, plan, op schema and fake kernel - and the premise
under which tests/test_gpu_moe_gate_up.py compares bit for bit (tests/moe_gate_up_cases.py)."""
import ctypes as ct
import os
import re

import pytest
import torch

import exact_inputs as X
import moe_gate_up_cases as C
from conftest import ROOT
from test_experts_host import _meta_args

SYMBOLS = ("bnb_mi355x_gemm_4bit_experts_gate_up", "bnb_mi355x_gemm_4bit_experts_gate_up_supported",
           "bnb_mi355x_gemm_4bit_experts_gate_up_plan")


def test_symbols_are_declared_exported_and_listed():
    from bitsandbytes_amd import cextension as ce

    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read(), flags=re.S)
    dll = ct.CDLL(str(ce.LIB_PATH))
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/bnb_mi355x.h"
        assert name in ce.EXPORTED_SYMBOLS and hasattr(dll, name), name


def test_predicate():
    from bitsandbytes_amd.backends.hip import gemm_4bit_experts_gate_up_supported as _supported

    bf = torch.bfloat16
    for c in C.CASES:
        for S in sorted({s for _, s in C.TS}):
            assert _supported(c.dtype, c.E, c.N, c.K, c.blocksize, S, "chunked") and _supported(c.dtype, c.E, c.N, c.K, c.blocksize, S, "interleaved")
    assert _supported(bf, 256, 4096, 7168, 64, 8, "chunked") and _supported(bf, 8, 28672, 4096, 64, 2, "interleaved")
    for E, N, K, bs, S in ((8, 63, 768, 64, 2), (8, 64, 768, 64, 0), (8, 64, 768, 64, 17), (8, 64, 768, 16, 2), (8, 64, 800, 64, 2)):
        assert not _supported(bf, E, N, K, bs, S, "chunked"), (E, N, K, bs, S)
    assert not _supported(torch.float64, 8, 64, 768, 64, 2, "chunked") and not _supported(bf, 8, 64, 768, 64, 2, "none")


@pytest.mark.parametrize("cus", [1, 256])
def test_plan_has_the_lane_map_of_the_down_kernel(cus, request):
    import bitsandbytes_amd as bnb

    bnb.lib.bnb_mi355x_set_cu_count(cus)
    request.addfinalizer(lambda: bnb.lib.bnb_mi355x_set_cu_count(0))
    for K in (96, 768, 1024, 2048, 2560, 7168, 18432):
        for T, S in C.TS:
            up, down = (ct.c_int * 4)(), (ct.c_int * 4)()
            assert bnb.lib.bnb_mi355x_gemm_4bit_experts_gate_up_plan(T, S, 4096, K, up) == 1
            assert bnb.lib.bnb_mi355x_gemm_4bit_experts_combine_plan(T, S, 4096, K, down) == 1
            assert list(up)[:3] == list(down)[:3] and 1 <= up[3] <= 32 and (2 * up[3]) % (64 // up[0]) == 0, (K, T, S, list(up))


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_op_schema_and_fake_shapes(nested):
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts_gate_up.default
    assert 'Tensor? absmax_offset=None, str gated="chunked") -> Tensor' in str(op._schema)
    args, kw = _meta_args(nested=nested)                                             # E 8, N 96, K 128, T 3, S 2
    for gated in ("chunked", "interleaved"):
        y = op(*args, gated=gated, bias=torch.empty((8, 96), dtype=args[0].dtype, device="meta"), **kw)
        assert y.shape == (3, 2, 48) and y.dtype == args[0].dtype and y.device.type == "meta"
    with pytest.raises(RuntimeError, match="gated must be"):
        op(*args, gated="none", **kw)
    args, kw = _meta_args(per_slot=True, nested=nested)
    with pytest.raises(RuntimeError, match=r"A must be \[T, K\]"):
        op(*args, **kw)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_every_exact_case_builds_with_live_gate_values(case):
    ex = C.build_case(case)
    X.assert_exact_sums(ex.W, ex.x, ex.unit, case.dtype, extra=float(X.BIAS_MAX))
    shares = C.live_share(ex, case, False), C.live_share(ex, case, True)
    print(f"{case.name}: share of gate values with 2^-4 <= |g| <= 8: {shares[0]:.3f} (no bias), {shares[1]:.3f} (bias)")
    assert case.nested or min(shares) >= 0.5, shares
