"""GPU: the sync-free LLM.int8() mixed decomposition - the quantize with a device column mask (csrc/int8_quant.hip), the outlier
accumulate (csrc/int8_outlier.hip) and nn.Linear8bitLt(threshold > 0) on top of them. The quantize is compared bit for bit with the
CPU formula of tests/test_gpu_int8.py; the outlier term against float64 on the CPU under one rounding of the result plus the fp32
accumulation of exact products."""
import ctypes as ct

import pytest
import torch

import bitsandbytes_amd as bnb
import bitsandbytes_amd.functional as F
from bitsandbytes_amd.cextension import INT8_OK, Int8OutlierAddmmArgs
from test_gpu_int8 import bits, layer_ref, make_layer, quant_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
STRIP = 64     # int8_outlier.hip: columns of out per workgroup
CHUNK = 8192   # int8_outlier.hip: mask bits per chunk of the walk (K = 8208 crosses it)


def mask_of(cols, K):
    flags = torch.zeros(-(K // -32) * 32, dtype=torch.int64)
    flags[cols] = 1
    words = (flags.view(-1, 32) << torch.arange(32)).sum(1)
    return torch.where(words >= 2**31, words - 2**32, words).int()


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("cols", [7, 64, 80, 330, 8208])   # narrow; wide; a partial last mask word; narrow over two steps; past kRegCols
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_quant_mask_has_the_bits_of_the_cpu_formula(dtype, cols, rows):
    A = (torch.rand(rows, cols) * 6 - 3).to(dtype)
    A[0, 0], A[rows - 1, cols - 1], A[rows // 2, 3] = 6.0, -6.0, 8.0                 # +-threshold exactly: outliers (the test is >=)
    A[0, 1] = (bits(torch.tensor([6.0], dtype=dtype)) - 1).view(dtype)[0]            # the largest value below 6: no outlier
    if cols > 32:
        A[0, 31], A[rows - 1, 32] = -7.0, 7.0
    all_out = torch.cat([torch.full((1, cols), 7.0, dtype=dtype), A[:1]])            # an all-outlier row: every column is flagged
    for x in (A, all_out):
        q, stats, mask = F.int8_vectorwise_quant_mask(x.to(DEV), 6.0)
        want_q, want_stats, want_cols = quant_ref(x, 6.0)
        assert mask.dtype == torch.int32 and torch.equal(mask.cpu(), mask_of(want_cols, cols))
        assert torch.equal(q.cpu(), want_q) and torch.equal(stats.cpu(), want_stats)
    assert len(want_cols) == cols and want_stats[0] == 0 and not q.any()
    assert 1 not in quant_ref(A, 6.0)[2] and {0, 3, cols - 1} <= set(quant_ref(A, 6.0)[2].tolist())
    q, stats, mask = F.int8_vectorwise_quant_mask(A.to(DEV), 1e30)                    # no element reaches it: the plain quantization
    want_q, want_stats, _ = quant_ref(A)
    assert not mask.any() and torch.equal(q.cpu(), want_q) and torch.equal(stats.cpu(), want_stats)


@pytest.mark.parametrize("count", [0, 1, 31, 32, 33, "K"])
@pytest.mark.parametrize("K", [80, CHUNK + 16])
@pytest.mark.parametrize("dtype,p", [(torch.float16, 11), (torch.bfloat16, 8)], ids=str)
def test_outlier_addmm_against_float64(dtype, p, K, count):
    Mmax, Nmax = 17, STRIP + 1
    count = K if count == "K" else count
    # K = 80: a random set; K = 8208: the last columns - the second chunk of the mask walk, from 31 on both chunks
    cols = torch.randperm(K)[:count].sort().values if K == 80 else torch.arange(K - count, K)
    x = (torch.randn(Mmax, K) * 4).to(dtype)
    CB, SCB = torch.randint(-128, 128, (Nmax, K), dtype=torch.int8), torch.rand(Nmax) * 2 + 0.5
    old = torch.randn(Mmax, Nmax).to(dtype)
    Wd = (CB.float() * SCB[:, None] * 7.874015718698502e-3).to(dtype).double()
    want = old.double() + x[:, cols].double() @ Wd[:, cols].T
    bound = 2.0**-p * want.abs() + count * 2.0**-24 * (x[:, cols].double().abs() @ Wd[:, cols].abs().T)
    xd, CBd, SCBd, maskd = x.to(DEV), CB.to(DEV), SCB.to(DEV), mask_of(cols, K).to(DEV)
    for M in (1, 16, 17):
        for N in (1, 17, Nmax):
            out = old[:M, :N].contiguous().to(DEV)
            assert F.int8_outlier_addmm_(out, xd[:M], CBd[:N].contiguous(), SCBd[:N].contiguous(), maskd) is out
            if count == 0:
                assert torch.equal(bits(out), bits(old[:M, :N])), (M, N)
            else:
                err = (out.cpu().double() - want[:M, :N]).abs()
                print(f"M={M} N={N}: max err / bound {(err / bound[:M, :N]).max():.3f}")
                assert (err <= bound[:M, :N]).all(), (M, N)


def test_outlier_addmm_guard_bands():
    M, N, K, pad = 17, STRIP + 1, 80, 1024
    x, CB, SCB = torch.randn(M, K).half(), torch.randint(-128, 128, (N, K), dtype=torch.int8), torch.ones(N)
    buf = torch.full((pad + M * N + pad,), 0x5A5A, dtype=torch.int16)
    buf[pad:pad + M * N] = 0                                                          # out = +0.0
    mask = mask_of(torch.tensor([3, 79]), K)
    dev = [t.to(DEV) for t in (x, CB, SCB, mask, buf)]
    args = Int8OutlierAddmmArgs(ct.sizeof(Int8OutlierAddmmArgs), 1, M, N, K, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                dev[3].data_ptr(), dev[4].data_ptr() + 2 * pad, torch.cuda.current_stream().cuda_stream)
    assert bnb.lib.bnb_mi355x_int8_outlier_addmm(ct.byref(args)) == INT8_OK
    got = dev[4].cpu()
    assert (got[:pad] == 0x5A5A).all() and (got[pad + M * N:] == 0x5A5A).all()
    Wd = (CB.float() * 7.874015718698502e-3).half().double()
    want, mag = x[:, [3, 79]].double() @ Wd[:, [3, 79]].T, x[:, [3, 79]].double().abs() @ Wd[:, [3, 79]].abs().T
    err = (got[pad:pad + M * N].view(torch.float16).view(M, N).double() - want).abs()
    assert (err <= 2.0**-11 * want.abs() + 2 * 2.0**-24 * mag).all()


def outlier_inputs(dtype, M=16, K=256):
    """Three inputs whose outlier sets differ: none, columns {3, 10}, 40 columns."""
    xs = [torch.randn(M, K).clamp(-5, 5) for _ in range(3)]
    xs[1][0, 3], xs[1][2, 10] = 8.0, -9.0
    xs[2][torch.arange(40) % M, torch.arange(40) * 6 + 1] = 7.0
    return [x.to(dtype) for x in xs]


@pytest.mark.parametrize("dtype,p", [(torch.float16, 11), (torch.bfloat16, 8)], ids=str)
def test_linear8bitlt_mixed_is_within_the_bound_and_graph_capturable(dtype, p):
    M, K, N = 16, 256, 64
    layer, W = make_layer(K, N, True, threshold=6.0)
    b = layer.bias.detach().cpu()
    xs = outlier_inputs(dtype, M, K)
    eager = [layer(x.to(DEV)) for x in xs]
    for x, y, n_out in zip(xs, eager, (0, 2, 40)):
        part32, cols, (qw, sw) = layer_ref(x, W, b, dtype, 6.0, rounded=False)
        assert len(cols) == n_out
        w_out = (qw[:, cols].float() * sw[:, None] * 7.874015718698502e-3).to(dtype).double()
        want = part32.double() + x[:, cols].double() @ w_out.T
        bound = 2.0**-p * (part32.double().abs() + want.abs()) + n_out * 2.0**-24 * (x[:, cols].double().abs() @ w_out.abs().T)
        err = (y.cpu().double() - want).abs()
        print(f"{n_out} outlier columns: max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()

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


def test_linear8bitlt_mixed_fp32_input_keeps_the_composed_path():
    M, K, N = 16, 256, 64
    layer, W = make_layer(K, N, True, threshold=6.0)
    x = outlier_inputs(torch.float32, M, K)[1]
    part32, cols, (qw, sw) = layer_ref(x, W, layer.bias.detach().cpu(), torch.float32, 6.0)
    assert cols.tolist() == [3, 10]
    w_out = (qw[:, cols].float() * sw[:, None] * 7.874015718698502e-3).double()
    want = part32.double() + x[:, cols].double() @ w_out.T
    # an fp32 addmm over two columns: a rounding per partial sum (each at most |part32| + sum |terms|, the last one |want|) and, without
    # FMAs, one per product
    bound = 2.0**-24 * (part32.double().abs() + want.abs()) + 2 * 2.0**-24 * (x[:, cols].double().abs() @ w_out.abs().T)
    y = layer(x.to(DEV))
    assert y.dtype == torch.float32 and ((y.cpu().double() - want).abs() <= bound).all()
