"""gemm_int8_tall_kernel (csrc/gemm_int8_tall.hip), forced with tuning knob cfg 61 / 62 / 63 or reached through the route: exact int32 at
every tile edge, the dequant epilogue's bits, nothing stored outside [M, N], and Linear8bitLt on a prefill-sized batch."""
import contextlib
import ctypes as ct

import pytest
import torch

import bitsandbytes_amd as bnb
import bitsandbytes_amd.functional as F
from bitsandbytes_amd.cextension import INT8_OK, GemmInt8Args

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPS = torch.ops.bitsandbytes
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
INT8, TALL = 13, 14                 # bnb_mi355x_last_gemm_kernel
BN, K_TILE, STAGES = 128, 64, 4     # gemm_int8_tall.hip: kBN, kBK, kStages
TILES = {6200: 128, 6300: 64}       # knob -> BM
K_PARTIAL_TILE = K_TILE + 16        # the second tile holds one 16-byte piece
K_RING_WRAPS = (STAGES + 1) * K_TILE + 48   # the ring's first stage is filled twice; the last tile is three pieces


def rand_i8(*shape):
    return torch.randint(-128, 128, shape, dtype=torch.int8)


def bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def dequant_ref(C, rs, cs, bias, dtype):
    out = C.float() * (rs[:, None] * cs[None, :]) * torch.tensor(6.200124e-05, dtype=torch.float32)
    return (out if bias is None else out + bias.float()).to(dtype)


def quant_ref(A):
    stats = A.float().abs().amax(dim=1)
    return torch.round(A.float() * (torch.tensor(127.0) / stats)[:, None]).to(torch.int8), stats


@contextlib.contextmanager
def knob(value):
    try:
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, value)
        yield
    finally:
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, 0)
        bnb.lib.bnb_mi355x_set_cu_count(0)


@pytest.mark.parametrize("K", [16, 48, K_TILE, K_PARTIAL_TILE, K_RING_WRAPS])
@pytest.mark.parametrize("tile", TILES)
def test_tall_matmul_is_exact_at_every_tile_edge_and_cu_count(tile, K):
    BM = TILES[tile]
    A, B = rand_i8(2 * BM + 2, K), rand_i8(2 * BN + 16, K)
    A[0, :], B[0, :] = -128, -128
    want = (A.double() @ B.double().T).int()   # exact: the sums are far below 2^53
    Ad, Bd = A.to(DEV), B.to(DEV)
    bad = []
    with knob(tile):
        for cus in (32, 256):
            bnb.lib.bnb_mi355x_set_cu_count(cus)
            for M in (1, BM - 1, BM, BM + 1, 2 * BM + 2):
                for N in (1, BN - 1, BN, BN + 1, 2 * BN + 16):
                    got = F.int8_linear_matmul(Ad[:M], Bd[:N])
                    out = torch.full((M, N), 7, dtype=torch.int32, device=DEV)
                    F.int8_linear_matmul(Ad[:M], Bd[:N], out=out)
                    ran = bnb.lib.bnb_mi355x_last_gemm_kernel()
                    if not (ran == TALL and torch.equal(got.cpu(), want[:M, :N]) and torch.equal(out.cpu(), want[:M, :N])):
                        bad.append((cus, M, N, ran))
    assert not bad, bad


@pytest.mark.parametrize("K", [4096, 131056])   # 128 * 128 * 131056 = 2^31 - 262144: the longest row, the largest sum
@pytest.mark.parametrize("b", [-128, 127])
def test_tall_matmul_extreme_values_and_the_longest_row(b, K):
    A = torch.full((65, K), -128, dtype=torch.int8, device=DEV)
    B = torch.full((17, K), b, dtype=torch.int8, device=DEV)
    with knob(6100):
        got = F.int8_linear_matmul(A, B)
        assert bnb.lib.bnb_mi355x_last_gemm_kernel() == TALL
    assert torch.equal(got.cpu(), torch.full((65, 17), -128 * b * K, dtype=torch.int32))


@pytest.mark.parametrize("bias_dtype", [None, *DTYPES], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_tall_scaled_mm_has_the_bits_of_the_cpu_formula_and_of_the_other_kernel(dtype, bias_dtype):
    M, N, K = 128 + 1, BN + 17, 80
    A, B = rand_i8(M, K), rand_i8(N, K)
    rs, cs = torch.rand(M) * 4, torch.rand(N) * 4
    rs[:3], cs[:3] = torch.tensor([0.0, 1e-40, 65504.0]), torch.tensor([65504.0, 0.0, 1e-40])
    bias = None if bias_dtype is None else torch.randn(N).to(bias_dtype)
    want = dequant_ref(A.double() @ B.double().T, rs, cs, bias, dtype)
    dev = [t if t is None else t.to(DEV) for t in (A, B, rs, cs, bias)]
    with knob(6100):
        got = OPS.int8_scaled_mm.default(*dev, dtype=dtype)
        assert bnb.lib.bnb_mi355x_last_gemm_kernel() == TALL
    with knob(6000):
        other = OPS.int8_scaled_mm.default(*dev, dtype=dtype)
        assert bnb.lib.bnb_mi355x_last_gemm_kernel() == INT8
    assert got.dtype == dtype and torch.equal(bits(got), bits(want)) and torch.equal(bits(other), bits(got))


@pytest.mark.parametrize("epilogue,dtype", [(0, torch.int32), (1, torch.bfloat16)], ids=str)
def test_tall_guard_band(epilogue, dtype):
    M, N, K, pad = 128 + 1, BN + 1, 80, 4096   # pad: 1024 words, in bytes
    A, B = rand_i8(M, K), rand_i8(N, K)
    rs, cs = torch.rand(M) * 4, torch.rand(N) * 4
    C = A.double() @ B.double().T
    want = C.int() if epilogue == 0 else dequant_ref(C, rs, cs, None, dtype)
    size = M * N * want.element_size()
    buf = torch.full((pad + size + pad,), 0x5A, dtype=torch.uint8, device=DEV)
    dev = [t.to(DEV) for t in (A, B, rs, cs)]
    args = GemmInt8Args(ct.sizeof(GemmInt8Args), epilogue, 2, 0, M, N, K, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                        None, buf.data_ptr() + pad, torch.cuda.current_stream().cuda_stream)
    with knob(6100):
        assert bnb.lib.bnb_mi355x_gemm_int8(ct.byref(args)) == INT8_OK and bnb.lib.bnb_mi355x_last_gemm_kernel() == TALL
    buf = buf.cpu()
    assert torch.equal(buf[pad:pad + size].view(dtype).view(M, N).view(torch.uint8), want.view(torch.uint8))
    assert (buf[:pad] == 0x5A).all() and (buf[pad + size:] == 0x5A).all()


@pytest.mark.parametrize("M,kernel", [(2048, TALL), (4, INT8)])
def test_linear8bitlt_takes_the_route(M, kernel):
    layer = bnb.nn.Linear8bitLt(256, 512, bias=True, has_fp16_weights=False)
    W, b = layer.weight.data.clone().half(), layer.bias.detach().clone()
    x = torch.randn(M, 256).half()
    (qx, sx), (qw, sw) = quant_ref(x), quant_ref(W)
    want = dequant_ref(qx.double() @ qw.double().T, sx, sw, b, torch.float16)
    got = layer.to(DEV)(x.to(DEV))
    assert bnb.lib.bnb_mi355x_last_gemm_kernel() == kernel
    assert torch.equal(bits(got), bits(want))
