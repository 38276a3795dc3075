"""Cases shared by tests/test_experts_mfma_host.py (CPU) and tests/test_gpu_experts_mfma.py (GPU): the expert-indexed MFMA kernel
(``bitsandbytes_amd::gemm_4bit_experts_mfma``, csrc/gemm4_experts_mfma.hip) on the operands of tests/exact_inputs.py.

Shapes ``E x N x K``, blocksize - the smallest at which each mechanism can go wrong:
  3 x 40 x 64     64   a row shorter than one 256-k chunk; N no multiple of 16; gated I = 20
  4 x 96 x 320    64   one whole chunk and a quarter chunk; seven idle wavefronts
  3 x 48 x 2304   128  nine chunks, so wavefront 0 owns two; a block spans two MFMA sub-blocks
  2 x 34 x 4352   64   seventeen chunks; with nested statistics the groups of 256 blocks straddle the expert boundary
each in bf16 and fp16 with plain and nested statistics (fp16: ``exps=(-2, 1)``, as tests/experts_cases.py)."""
import torch

from experts_cases import ExpertCase

SHAPES = ((3, 40, 64, 64), (4, 96, 320, 64), (3, 48, 2304, 128), (2, 34, 4352, 64))
CASES = tuple(ExpertCase(E, N, K, bs, dtype, nested, exps=(-2, 1) if dtype == torch.float16 else (-2, 3))
              for (E, N, K, bs) in SHAPES for dtype in (torch.bfloat16, torch.float16) for nested in (False, True))
TS_OF_P = {1: (1, 1), 15: (5, 3), 16: (8, 2), 17: (17, 1), 33: (11, 3)}   # pairs per expert around the 16-pair pass
ID_SETS = tuple(("one", P) for P in TS_OF_P) + (("random", 33), ("masked", 33))
