"""CPU (-m "not gpu"): the host side of the sync-free LLM.int8() mixed decomposition (bitsandbytes_amd::int8_vectorwise_quant_mask,
bitsandbytes_amd::int8_outlier_addmm_) - op schemas, fake kernels, no CPU kernel, C ABI names."""
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import bitsandbytes_amd  # noqa: F401  (defines the ops)
from conftest import ROOT

OPS = torch.ops.bitsandbytes_amd
SYMBOLS = ("bnb_mi355x_int8_vectorwise_quant_mask", "bnb_mi355x_int8_outlier_addmm")


def test_schemas():
    assert str(OPS.int8_vectorwise_quant_mask.default._schema) == \
        "bitsandbytes_amd::int8_vectorwise_quant_mask(Tensor A, float threshold) -> (Tensor, Tensor, Tensor)"
    assert str(OPS.int8_outlier_addmm_.default._schema) == \
        "bitsandbytes_amd::int8_outlier_addmm_(Tensor(a!) out, Tensor A, Tensor CB, Tensor SCB, Tensor mask) -> ()"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=str)
@pytest.mark.parametrize("K,words", [(7, 1), (64, 2), (80, 3), (8208, 257)])
def test_fake_shapes_and_dtypes(dtype, K, words):
    with FakeTensorMode():
        A = torch.empty(2, 3, K, dtype=dtype)
        q, stats, mask = OPS.int8_vectorwise_quant_mask.default(A, 6.0)
        assert (q.shape, q.dtype) == (A.shape, torch.int8) and (stats.shape, stats.dtype) == ((6,), torch.float32)
        assert (mask.shape, mask.dtype) == ((words,), torch.int32)
        with pytest.raises(RuntimeError, match="threshold must be positive"):
            OPS.int8_vectorwise_quant_mask.default(A, 0.0)
        if dtype != torch.float32 and K % 16 == 0:
            out = torch.empty(2, 3, 5, dtype=dtype)
            args = (A, torch.empty(5, K, dtype=torch.int8), torch.empty(5), mask)
            assert OPS.int8_outlier_addmm_.default(out, *args) is None
            with pytest.raises(RuntimeError, match="mask must hold"):
                OPS.int8_outlier_addmm_.default(out, *args[:3], torch.empty(words + 1, dtype=torch.int32))
            with pytest.raises(RuntimeError, match="out must be"):
                OPS.int8_outlier_addmm_.default(out[..., :4], *args)


def test_no_cpu_kernels():
    A = torch.zeros(2, 64, dtype=torch.float16)
    with pytest.raises(NotImplementedError):
        OPS.int8_vectorwise_quant_mask.default(A, 6.0)
    with pytest.raises(NotImplementedError):
        OPS.int8_outlier_addmm_.default(torch.zeros(2, 5, dtype=torch.float16), A, torch.zeros(5, 64, dtype=torch.int8), torch.ones(5),
                                        torch.zeros(2, dtype=torch.int32))


def test_entry_points_are_declared_and_listed():
    from bitsandbytes_amd import cextension as ce

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(const {name}_args\* args\);", header, flags=re.M), name
        assert name in ce.EXPORTED_SYMBOLS and hasattr(ce.lib, name)
