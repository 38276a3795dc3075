"""GPU: LLM.int8() inference - csrc/int8_quant.hip, csrc/gemm_int8.hip and nn.Linear8bitLt against the formulas of the reference's
default backend evaluated with torch on the CPU. Everything is compared bit for bit except the 16-bit outlier matmul of the mixed path."""
import ctypes as ct

import pytest
import torch

import bitsandbytes_amd as bnb
import bitsandbytes_amd.functional as F
from bitsandbytes_amd.cextension import INT8_OK, INT8_REFUSED_K, GemmInt8Args

pytestmark = pytest.mark.gpu

DEV = "cuda"
OPS = torch.ops.bitsandbytes
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
# gemm_int8.hip: 8 wavefronts split K in chunks of 256
K_IDLE_WAVES = 3 * 256          # wavefronts 3 ... 7 own no chunk
K_UNEVEN_TAIL = 9 * 256 + 48    # ten chunks (wavefronts 0 and 1 own two), the last one 48 k: a partial MFMA step
REG_COLS = 8192                 # int8_quant.hip: the longest row that stays in registers


def rand_i8(*shape):
    return torch.randint(-128, 128, shape, dtype=torch.int8)


def quant_ref(A, threshold=0.0):
    """backends/default/ops.py:142-177 in fp32 on the CPU; a row without a maximum gives zeros."""
    a = A.float().clone()
    outliers = a.abs() >= threshold if threshold > 0 else torch.zeros_like(a, dtype=torch.bool)
    a[outliers] = 0
    stats = a.abs().amax(dim=1)
    q = torch.round(a * (torch.tensor(127.0) / stats)[:, None])
    q = torch.where(stats[:, None] == 0, torch.zeros_like(q), q).to(torch.int8)
    cols = torch.argwhere(outliers.any(dim=0)).view(-1)
    if A.shape[0] > 1:
        q[:, cols] = 0
    return q, stats, cols


def dequant_ref(C, rs, cs, bias, dtype, rounded=True):
    out = C.float() * (rs[:, None] * cs[None, :])
    out = out * torch.tensor(6.200124e-05, dtype=torch.float32)
    if bias is not None:
        out = out + bias.float()
    return out.to(dtype) if rounded else out


def bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("K", [16, 64, 80, K_IDLE_WAVES, K_UNEVEN_TAIL])
def test_matmul_is_exact_at_every_tile_edge_and_cu_count(K):
    A, B = rand_i8(130, K), rand_i8(1040, K)   # 1040 rows: three 16-row tiles per workgroup on 32 CUs, the last workgroup short
    A[0, :], B[0, :] = -128, -128
    want = (A.long() @ B.long().T).int()
    Ad, Bd = A.to(DEV), B.to(DEV)
    bad = []
    try:
        for cus in (32, 256):
            bnb.lib.bnb_mi355x_set_cu_count(cus)
            for M in (1, 15, 16, 17, 64, 65, 130):
                for N in (1, 15, 16, 17, 1040):
                    got = F.int8_linear_matmul(Ad[:M], Bd[:N])
                    out = torch.full((M, N), 7, dtype=torch.int32, device=DEV)
                    F.int8_linear_matmul(Ad[:M], Bd[:N], out=out)
                    if not (torch.equal(got.cpu(), want[:M, :N]) and torch.equal(out.cpu(), want[:M, :N])):
                        bad.append((cus, M, N))
    finally:
        bnb.lib.bnb_mi355x_set_cu_count(0)
    assert not bad, bad


@pytest.mark.parametrize("b", [-128, 127])
def test_matmul_extreme_values(b):
    A = torch.full((65, 4096), -128, dtype=torch.int8, device=DEV)
    B = torch.full((17, 4096), b, dtype=torch.int8, device=DEV)
    assert torch.equal(F.int8_linear_matmul(A, B).cpu(), torch.full((65, 17), -128 * b * 4096, dtype=torch.int32))


@pytest.mark.parametrize("bias_dtype", [None, *DTYPES], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_scaled_mm_has_the_bits_of_the_cpu_formula_and_of_the_two_step_api(dtype, bias_dtype):
    M, N, K = 17, 33, 80
    A, B = rand_i8(M, K), rand_i8(N, K)
    rs, cs = torch.rand(M) * 4, torch.rand(N) * 4
    rs[:3], cs[:3] = torch.tensor([0.0, 1e-40, 65504.0]), torch.tensor([65504.0, 0.0, 1e-40])
    bias = None if bias_dtype is None else torch.randn(N).to(bias_dtype)
    want = dequant_ref(A.long() @ B.long().T, rs, cs, bias, dtype)
    dev = [t if t is None else t.to(DEV) for t in (A, B, rs, cs, bias)]
    got = OPS.int8_scaled_mm.default(*dev, dtype=dtype)
    two = OPS.int8_mm_dequant.default(F.int8_linear_matmul(dev[0], dev[1]), dev[2], dev[3], dtype=dtype, bias=dev[4])
    assert got.dtype == dtype and torch.equal(bits(got), bits(want)) and torch.equal(bits(two), bits(got))


@pytest.mark.parametrize("cols", [1, 7, 8, 63, 64, 65, 4104, 4112, REG_COLS + 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_vectorwise_quant_has_the_bits_of_the_cpu_formula(dtype, cols):
    A = (torch.randn(3, cols) * 3).to(dtype)
    for rows in (1, 3):
        q, stats, outliers = F.int8_vectorwise_quant(A[:rows].to(DEV))
        want_q, want_stats, _ = quant_ref(A[:rows])
        assert outliers is None and torch.equal(q.cpu(), want_q) and torch.equal(stats.cpu(), want_stats), rows


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_vectorwise_quant_ties_and_zero_row(dtype):
    A = torch.tensor([[127, 0.5, 1.5, 2.5, -0.5, -1.5], [0, 0, 0, 0, 0, 0]]).to(dtype)
    q, stats, _ = F.int8_vectorwise_quant(A.to(DEV))
    assert q.cpu().tolist() == [[127, 0, 2, 2, 0, -2], [0] * 6] and stats.cpu().tolist() == [127.0, 0.0]


@pytest.mark.parametrize("cols", [7, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_vectorwise_quant_threshold(dtype, cols):
    A = (torch.rand(3, cols) * 6 - 3).to(dtype)
    A[1, 5] = 8.0
    for rows in (A, A[1:2], torch.cat([torch.full((1, cols), 7.0, dtype=dtype), A[:1]])):   # three rows; one row; an all-outlier row
        q, stats, outliers = F.int8_vectorwise_quant(rows.to(DEV), threshold=6.0)
        want_q, want_stats, want_cols = quant_ref(rows, 6.0)
        assert outliers.dtype == torch.int64 and torch.equal(outliers.cpu(), want_cols)
        assert torch.equal(q.cpu(), want_q) and torch.equal(stats.cpu(), want_stats)
    assert want_stats[0] == 0 and not q.any()                                  # (the all-outlier row, every column with it)
    q, stats, outliers = F.int8_vectorwise_quant(A.to(DEV), threshold=6.0)
    assert outliers.tolist() == [5] and not q[:, 5].any() and stats[1] == A[1].float().abs()[torch.arange(cols) != 5].max()
    q1 = F.int8_vectorwise_quant(A[1:2].to(DEV), threshold=6.0)[0]
    assert q1[0, 5] == 0 and q1[0, :5].any()


def make_layer(K, N, bias, threshold=0.0):
    layer = bnb.nn.Linear8bitLt(K, N, bias=bias, has_fp16_weights=False, threshold=threshold)
    W = layer.weight.data.clone().half()
    return layer.to(DEV), W


def layer_ref(x, W, bias, dtype, threshold=0.0, rounded=True):
    qx, sx, cols = quant_ref(x, threshold)
    qw, sw, _ = quant_ref(W)
    return dequant_ref(qx.long() @ qw.long().T, sx, sw, bias, dtype, rounded), cols, (qw, sw)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,K,N", [(3, 80, 33), (16, 256, 64)])
def test_linear8bitlt_forward_graph_and_state_dict(M, K, N, bias):
    layer, W = make_layer(K, N, bias)
    b = layer.bias.detach().cpu() if bias else None
    xs = [torch.randn(M, K).half() for _ in range(3)]
    want = [layer_ref(x, W, b, torch.float16) for x in xs]
    qw, sw = want[0][2]
    assert torch.equal(layer.weight.CB.cpu(), qw) and torch.equal(layer.weight.SCB.cpu(), sw)
    eager = [layer(x.to(DEV)) for x in xs]
    assert all(torch.equal(bits(y), bits(w[0])) for y, w in zip(eager, want))

    static = xs[0].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = layer(static)
    for x, e in zip(xs[::-1], eager[::-1]):
        static.copy_(x)
        graph.replay()
        assert torch.equal(bits(y), bits(e))

    sd = layer.state_dict()
    assert {"weight", "SCB", "weight_format"} <= set(sd) and sd["weight"].dtype == torch.int8
    fresh = bnb.nn.Linear8bitLt(K, N, bias=bias)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()})
    assert torch.equal(bits(fresh.to(DEV)(xs[1].to(DEV))), bits(eager[1]))


@pytest.mark.parametrize("dtype,p", [(torch.float16, 11), (torch.bfloat16, 8)], ids=str)
def test_linear8bitlt_mixed_decomposition(dtype, p):
    M, K, N = 16, 256, 64
    layer, W = make_layer(K, N, True, threshold=6.0)
    x = torch.randn(M, K).clamp(-5, 5)
    x[0, 3], x[2, 10] = 8.0, -9.0
    x = x.to(dtype)
    b = layer.bias.detach().cpu()
    part32, cols, (qw, sw) = layer_ref(x, W, b, dtype, 6.0, rounded=False)
    assert cols.tolist() == [3, 10]
    xd = x.to(DEV)
    q, stats, outliers = F.int8_vectorwise_quant(xd, threshold=6.0)
    int8_part = OPS.int8_scaled_mm.default(q, layer.weight.CB, stats, layer.weight.SCB, layer.bias, dtype)
    assert torch.equal(outliers.cpu(), cols) and torch.equal(bits(int8_part), bits(part32.to(dtype)))
    w_out = (qw[:, cols].float() * sw[:, None] * 7.874015718698502e-3).to(dtype).double()        # [N, n_out]
    terms = x[:, cols].double()[:, None, :] * w_out[None, :, :]                                    # [M, N, n_out]
    want = part32.double() + terms.sum(-1)
    bound = 2.0**-p * (part32.double().abs() + want.abs()) + len(cols) * 2.0**-24 * terms.abs().sum(-1)
    err = (layer(xd).cpu().double() - want).abs()
    print(f"max err / bound: {(err / bound).max():.3f}")
    assert (err <= bound).all()


def gemm_int8_c(A, B, out_ptr):
    args = GemmInt8Args(ct.sizeof(GemmInt8Args), 0, 0, 0, A.shape[0], B.shape[0], A.shape[1], A.data_ptr(), B.data_ptr(), None, None, None,
                        out_ptr, torch.cuda.current_stream().cuda_stream)
    return bnb.lib.bnb_mi355x_gemm_int8(ct.byref(args))


def test_refused_k_and_guard_band():
    out = torch.zeros(1, dtype=torch.int32, device=DEV)
    for K in (24, 131072):
        assert gemm_int8_c(torch.ones(1, K, dtype=torch.int8, device=DEV), torch.ones(1, K, dtype=torch.int8, device=DEV), out.data_ptr()) == INT8_REFUSED_K
    A, B = rand_i8(5, 24), rand_i8(9, 24)
    want = (A.long() @ B.long().T).int()   # (sums far below 2^24: the fp32 fallback is exact here)
    assert torch.equal(F.int8_linear_matmul(A.to(DEV), B.to(DEV)).cpu(), want)
    M, N, K, pad = 17, 33, 80, 1024
    A, B = rand_i8(M, K), rand_i8(N, K)
    buf = torch.full((pad + M * N + pad,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    assert gemm_int8_c(A.to(DEV), B.to(DEV), buf.data_ptr() + 4 * pad) == INT8_OK
    buf = buf.cpu()
    assert torch.equal(buf[pad:pad + M * N].view(M, N), (A.long() @ B.long().T).int())
    assert (buf[:pad] == 0x5A5A5A5A).all() and (buf[pad + M * N:] == 0x5A5A5A5A).all()
