"""CPU: the predicate of the token-major MoE down projection (pure host logic of the library) and the premise under which
tests/test_gpu_moe_combine.py compares bit for bit (tests/moe_combine_cases.py)."""
import pytest
import torch

import moe_combine_cases as C

MAX_K = 65536   # csrc/gemm4_experts_combine.hip: kMaxSegs * kSegChunks * kChunkK
MAX_S = 16      # kMaxSlots


def test_predicate():
    from bitsandbytes_amd.backends.hip import gemm_4bit_experts_combine_supported as _supported

    for c in C.CASES:
        for S in sorted({s for _, s in C.TS}):
            assert _supported(c.dtype, c.E, c.N, c.K, c.blocksize, S), (c.name, S)
    bf = torch.bfloat16
    assert _supported(bf, 256, 7168, 2048, 64, 8) and _supported(bf, 8, 4096, 14336, 64, 2) and _supported(bf, 2, 32, MAX_K, 4096, MAX_S)
    for E, N, K, bs, S in ((8, 64, 768, 64, 0), (8, 64, 768, 64, MAX_S + 1), (8, 64, 800, 64, 2), (8, 64, 768, 16, 2),
                           (8, 64, 768, 48, 2), (8, 64, MAX_K + 4096, 4096, 2), (1 << 16, 1 << 15, 768, 64, 2)):
        assert not _supported(bf, E, N, K, bs, S), (E, N, K, bs, S)
    assert not _supported(torch.float64, 8, 64, 768, 64, 2)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_exactness_premise(case):
    ex = C.build_case(case)
    used = C.ts_of(case, ex)
    assert (1, 1) in used and (3, 2) in used, used   # (S = 2 everywhere: at K = 18432 ten units, more than wavefronts)
    assert all(S <= 2 for _, S in used) or case.K != C.LONG_K
    for T, S in used:
        w = C.weights(T, S)
        assert bool(torch.isin(w, torch.tensor([0.5, 1.0, 2.0])).all()) and T * S <= ex.x.shape[0]
        assert C.premise(ex, S)
        out = [int(((i < 0) | (i >= case.E)).sum()) for i in (C.make_ids(p, T, S, case.E) for p in C.ID_PATTERNS)]
        assert out == [0, 0, T, S], out   # distinct, same, one_out, token_out
    print(f"{case.name}: (T, S) used {used}")
