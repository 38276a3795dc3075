"""CPU: the host side of LLM.int8() inference - op schemas, fake kernels, the absence of CPU kernels, the C header, the layer's
state-dict format check. No compute (there is no GPU here)."""
import os
import re

import pytest
import torch

import bitsandbytes_amd as bnb
from conftest import ROOT

OPS = torch.ops.bitsandbytes

# the reference's schemas (bitsandbytes/_ops.py:9-139)
SCHEMAS = {
    "int8_vectorwise_quant": "(Tensor A, float threshold=0.0) -> (Tensor, Tensor, Tensor?)",
    "int8_linear_matmul": "(Tensor A, Tensor B) -> Tensor",
    "int8_linear_matmul.out": "(Tensor A, Tensor B, Tensor! out) -> ()",
    "int8_mm_dequant": "(Tensor A, Tensor row_stats, Tensor col_stats, ScalarType? dtype=None, Tensor? bias=None) -> Tensor",
    "int8_scaled_mm": "(Tensor A, Tensor B, Tensor row_stats, Tensor col_stats, Tensor? bias=None, ScalarType? dtype=None) -> Tensor",
    "int8_mixed_scaled_mm": "(Tensor A, Tensor CA, Tensor CB, Tensor SCA, Tensor SCB, Tensor? outlier_cols=None, Tensor? bias=None) -> (Tensor, Tensor?)",
    "int8_vectorwise_dequant": "(Tensor A, Tensor stats) -> Tensor",
}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_op_exists_with_the_reference_schema(name):
    base, _, overload = name.partition(".")
    op = getattr(getattr(OPS, base), overload or "default")
    want = torch._C.parse_schema(f"bitsandbytes::{base}{'.' + overload if overload else ''}{SCHEMAS[name]}")
    assert str(op._schema) == str(want)


def test_fake_kernels_give_shapes_and_dtypes():
    A, B = torch.empty(2, 3, 32, dtype=torch.int8, device="meta"), torch.empty(5, 32, dtype=torch.int8, device="meta")
    rs, cs = torch.empty(6, device="meta"), torch.empty(5, device="meta")
    x = torch.empty(6, 32, dtype=torch.bfloat16, device="meta")
    q, stats, outliers = OPS.int8_vectorwise_quant.default(x, 0.0)
    assert (q.shape, q.dtype, stats.shape, stats.dtype, outliers) == (x.shape, torch.int8, (6,), torch.float32, None)
    C = OPS.int8_linear_matmul.default(A, B)
    assert (C.shape, C.dtype) == ((2, 3, 5), torch.int32)
    assert OPS.int8_linear_matmul.out(A, B, out=torch.empty(2, 3, 5, dtype=torch.int32, device="meta")) is None
    y = OPS.int8_mm_dequant.default(C, rs, cs)
    assert (y.shape, y.dtype) == ((2, 3, 5), torch.float16)
    y = OPS.int8_scaled_mm.default(A, B, rs, cs, None, torch.bfloat16)
    assert (y.shape, y.dtype) == ((2, 3, 5), torch.bfloat16)
    w = OPS.int8_vectorwise_dequant.default(B, cs)
    assert (w.shape, w.dtype) == (B.shape, torch.float32)
    with pytest.raises(RuntimeError):
        OPS.int8_linear_matmul.default(A.float(), B)


@pytest.mark.parametrize("call", [
    lambda: OPS.int8_vectorwise_quant.default(torch.randn(2, 16), 0.0),
    lambda: OPS.int8_linear_matmul.default(torch.ones(2, 16, dtype=torch.int8), torch.ones(3, 16, dtype=torch.int8)),
    lambda: OPS.int8_mm_dequant.default(torch.ones(2, 3, dtype=torch.int32), torch.ones(2), torch.ones(3)),
    lambda: OPS.int8_scaled_mm.default(torch.ones(2, 16, dtype=torch.int8), torch.ones(3, 16, dtype=torch.int8), torch.ones(2), torch.ones(3)),
    lambda: OPS.int8_vectorwise_dequant.default(torch.ones(3, 16, dtype=torch.int8), torch.ones(3)),
], ids=["quant", "matmul", "mm_dequant", "scaled_mm", "dequant"])
def test_no_cpu_kernel(call):
    with pytest.raises(NotImplementedError):
        call()


def test_header_declares_the_entry_points_and_functional_has_the_wrappers():
    text = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    for name in ("bnb_mi355x_int8_vectorwise_quant", "bnb_mi355x_gemm_int8", "bnb_mi355x_int8_mm_dequant"):
        assert re.search(rf"^int {name}\(", text, flags=re.M) and name in bnb.cextension.EXPORTED_SYMBOLS
    for name in ("int8_vectorwise_quant", "int8_linear_matmul", "int8_mm_dequant", "int8_vectorwise_dequant"):
        assert callable(getattr(bnb.functional, name))


def test_linear8bitlt_state_dict_format():
    layer = bnb.nn.Linear8bitLt(16, 4, bias=False)
    assert isinstance(layer.weight, bnb.nn.Int8Params) and layer.weight.CB is None
    sd = {"weight": torch.zeros(4, 16, dtype=torch.int8), "SCB": torch.ones(4)}
    for fmt in ("col_turing", torch.tensor(1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="row"):
            layer.load_state_dict({**sd, "weight_format": fmt})
    for fmt in ("row", torch.tensor(0, dtype=torch.uint8)):
        layer.load_state_dict({**sd, "weight_format": fmt})
        assert layer.weight.CB.dtype == torch.int8 and torch.equal(layer.weight.SCB, sd["SCB"])
    with pytest.raises(NotImplementedError):
        bnb.nn.Linear8bitLt(16, 4, has_fp16_weights=True)
