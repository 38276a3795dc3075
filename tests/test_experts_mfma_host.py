"""CPU: the host side of the expert-indexed MFMA launch - predicate, op schema and fake kernel - and the premise under which
tests/test_gpu_experts_mfma.py compares bit for bit (tests/experts_mfma_cases.py)."""
import pytest
import torch

import experts_mfma_cases as C
import moe_ffn_cases as M
from test_experts_host import _meta_args


def test_predicate():
    from bitsandbytes_amd.backends.hip import gemm_4bit_experts_mfma_supported as _supported

    bf = torch.bfloat16
    for c in C.CASES:
        assert all(_supported(c.dtype, c.E, c.N, c.K, c.blocksize, g) for g in ("none", "chunked", "interleaved")), c.name
    assert _supported(bf, 8, 28672, 4096, 64, "chunked") and _supported(torch.float16, 128, 2048, 768, 128, "none")
    assert not _supported(torch.float32, 8, 64, 768, 64, "none")       # fp32
    assert not _supported(bf, 8, 64, 768, 32, "none")                  # blocksize 32
    assert not _supported(bf, 8, 64, 96, 32, "none") and not _supported(bf, 8, 64, 800, 16, "none")   # K % 64 != 0
    assert not _supported(bf, 8, 64, 320, 128, "none")                 # K % blocksize != 0
    assert _supported(bf, 8, 63, 768, 64, "none") and not _supported(bf, 8, 63, 768, 64, "chunked")   # N odd when gated
    assert not _supported(bf, 65536, 64, 768, 64, "none") and not _supported(bf, 8, 64, 1 << 18, 64, "none")   # the size limits
    assert not _supported(bf, 8, 64, 768, 64, "x")


@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_op_schema_and_fake_shapes(nested):
    op = torch.ops.bitsandbytes_amd.gemm_4bit_experts_mfma.default
    assert str(op._schema).split("(", 1)[1] == str(torch.ops.bitsandbytes_amd.gemm_4bit_experts_ffn.default._schema).split("(", 1)[1]
    for per_slot in (False, True):
        args, kw = _meta_args(per_slot=per_slot, nested=nested)                      # E 8, N 96, K 128, T 3, S 2
        scale = torch.empty((3, 2), dtype=torch.float32, device="meta")
        assert op(*args, **kw).shape == (3, 2, 96) and op(*args, row_scale=scale, **kw).shape == (3, 2, 96)
        assert op(*args, gated="chunked", **kw).shape == (3, 2, 48) and op(*args, gated="interleaved", **kw).dtype == args[0].dtype
        with pytest.raises(RuntimeError, match="cannot be given together"):
            op(*args, gated="chunked", row_scale=scale, **kw)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_every_exact_case_builds(case):
    """exact_inputs.build asserts the exact-sum bound for every activation row against every expert."""
    ex = M.build_case(case)
    assert ex.x.shape[0] >= max(C.TS_OF_P) and ex.W.shape == (case.E * case.N, case.K)
