"""Child process of tests/test_cu_count_host.py: every plan query of the library over the whole grid at ONE CU count, in a process of
its own - a query that kills its process (a division by zero in a plan function would) is then a failed CU count, not a dead pytest.

    python cu_count_sweep.py <library> <cus> <out.npz>        cus = 0: no override (a host without a device answers for 256)

Needs ctypes and numpy only: no torch, no GPU, nothing preloaded. Writes int64 arrays (grid order = the tuples below):

    plan    [dtypes, Ms, shapes, blocksizes, nested, 19]   (answer, out16[0 .. 15], bnb_mi355x_gemm_4bit_route, _workspace_bytes)
    forms   [3, dtypes16, Ms <= 16, shapes, blocksizes >= 64, nested, 17]   bnb_mi355x_gemm_4bit_sm_form_plan, forms 1, 2, 3
    grouped [groups, Ms, 18]                                (answer, out16, bnb_mi355x_gemm_4bit_grouped_route) at bf16, blocksize 64
    grad    [dtypes16, Ms, shapes, blocksizes >= 64, 19]    bnb_mi355x_gemm_4bit_grad_input_plan, (_supported, _workspace_bytes)
    preds   [...]                                           the *_supported predicates and bnb_mi355x_gemv_4bit_peer_serves: they returned
    exact   [3]                                             bnb_mi355x_gemv_4bit_stream_exact(bf16, 1, 4096, 4096, 64, 0) and R, grid_x of its plan
"""
import ctypes as ct
import sys

import numpy as np

CU_COUNTS = (1, 8, 20, 32, 64, 80, 128, 256, 304)
DTYPES = (0, 1, 2)   # fp32, fp16, bf16
MS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 512, 513)
# (N, K): the routed sweep's cases (tests/exact_inputs.py: SWEEP_CASES), then small, ragged and model shapes, one at 2^32 elements
SWEEP_NK = ((4096, 4096), (4096, 10752), (11008, 4096), (8192, 8192), (1376, 4096), (4096, 2752), (1376, 2752), (96, 2752), (4100, 1024),
            (130, 768), (5120, 5120), (3200, 4096))
SHAPES = SWEEP_NK + ((1, 64), (2, 256), (16, 256), (96, 256), (127, 320), (128, 256), (129, 4096), (1088, 256), (1216, 384), (1088, 2752),
                     (4096, 8192), (5120, 8192), (11008, 8192), (14336, 4096), (4096, 14336), (28672, 8192), (32000, 4096), (512, 32768),
                     (152064, 3584), (64, 131072), (65536, 65536))
BLOCKSIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
BLOCKSIZES64 = BLOCKSIZES[1:]
MS16 = tuple(m for m in MS if m <= 16)
GROUPS = ((4096, 4096, 4096, 4096), (5504, 2752), (128, 130, 4100), (1376, 1376), (11008, 11008), (512,) * 8, (129, 4096), (14336, 14336))
GROUP_K = 4096


def load(path):
    lib = ct.CDLL(path)
    I, P = ct.c_int, ct.c_void_p
    for name, args, res in (
        ("bnb_mi355x_set_cu_count", [I], None),
        ("bnb_mi355x_gemm_4bit_plan", [I] * 7 + [P], I),
        ("bnb_mi355x_gemm_4bit_sm_form_plan", [I] * 4 + [P] + [I] * 3 + [P], I),
        ("bnb_mi355x_gemm_4bit_grad_input_plan", [I] * 5 + [P], I),
        ("bnb_mi355x_gemm_4bit_route", [I] * 6, I),
        ("bnb_mi355x_gemm_4bit_workspace_bytes", [I] * 6, ct.c_size_t),
        ("bnb_mi355x_gemm_4bit_grouped_route", [I, I, P, I, I, I], I),
        ("bnb_mi355x_gemm_4bit_grad_input_supported", [I] * 5, I),
        ("bnb_mi355x_gemm_4bit_grad_input_workspace_bytes", [I] * 3, ct.c_size_t),
        ("bnb_mi355x_gemm_4bit_gated_supported", [I] * 5, I),
        ("bnb_mi355x_gemm_4bit_lora_supported", [I] * 7, I),
        ("bnb_mi355x_gemm_4bit_lora_ids_supported", [I] * 8, I),
        ("bnb_mi355x_gemm_4bit_experts_supported", [I] * 5, I),
        ("bnb_mi355x_gemv_4bit_peer_serves", [I] * 5 + [ct.c_long, I], I),
        ("bnb_mi355x_gemv_4bit_stream_exact", [I] * 6, I),
        ("bnb_mi355x_stream_geometry", [I, I, I, ct.c_long, I, I, P], I),
    ):
        f = getattr(lib, name)
        f.argtypes, f.restype = args, res
    return lib


def sweep(lib):
    out16 = np.zeros(16, dtype=np.int32)
    addr = out16.ctypes.data
    plan = np.zeros((len(DTYPES), len(MS), len(SHAPES), len(BLOCKSIZES), 2, 19), dtype=np.int64)
    preds = np.zeros((len(DTYPES), len(MS), len(SHAPES), len(BLOCKSIZES), 2, 4), dtype=np.int64)
    for a, dtype in enumerate(DTYPES):
        for b, M in enumerate(MS):
            for c, (N, K) in enumerate(SHAPES):
                for d, bs in enumerate(BLOCKSIZES):
                    route = lib.bnb_mi355x_gemm_4bit_route(0, dtype, M, N, K, bs)
                    ws = lib.bnb_mi355x_gemm_4bit_workspace_bytes(0, dtype, M, N, K, bs)
                    for e in (0, 1):
                        out16[:] = 0
                        ok = lib.bnb_mi355x_gemm_4bit_plan(0, dtype, M, N, K, bs, e, addr)
                        rec = plan[a, b, c, d, e]
                        rec[0], rec[1:17], rec[17], rec[18] = ok, out16, route, ws
                        preds[a, b, c, d, e] = (lib.bnb_mi355x_gemm_4bit_gated_supported(dtype, M, N, K, bs),
                                                lib.bnb_mi355x_gemm_4bit_lora_supported(dtype, M, N, K, bs, e, 16),
                                                lib.bnb_mi355x_gemm_4bit_lora_ids_supported(dtype, M, N, K, bs, e, 16, 3),
                                                lib.bnb_mi355x_gemm_4bit_experts_supported(dtype, 8, N, K, bs))
    forms = np.zeros((3, 2, len(MS16), len(SHAPES), len(BLOCKSIZES64), 2, 17), dtype=np.int64)
    for f in (1, 2, 3):
        for a, dtype in enumerate(DTYPES[1:]):
            for b, M in enumerate(MS16):
                for c, (N, K) in enumerate(SHAPES):
                    for d, bs in enumerate(BLOCKSIZES64):
                        for e in (0, 1):
                            out16[:] = 0
                            ok = lib.bnb_mi355x_gemm_4bit_sm_form_plan(f, dtype, M, N, None, K, bs, e, addr)
                            forms[f - 1, a, b, c, d, e, 0], forms[f - 1, a, b, c, d, e, 1:] = ok, out16
    grouped = np.zeros((len(GROUPS), len(MS), 18), dtype=np.int64)
    for g, heights in enumerate(GROUPS):
        ns = (ct.c_int * len(heights))(*heights)
        for b, M in enumerate(MS):
            out16[:] = 0
            ok = lib.bnb_mi355x_gemm_4bit_sm_form_plan(4, 2, M, len(heights), ns, GROUP_K, 64, 0, addr)
            grouped[g, b, 0], grouped[g, b, 1:17] = ok, out16
            grouped[g, b, 17] = lib.bnb_mi355x_gemm_4bit_grouped_route(2, len(heights), ns, M, GROUP_K, 64)
    grad = np.zeros((2, len(MS), len(SHAPES), len(BLOCKSIZES64), 19), dtype=np.int64)
    for a, dtype in enumerate(DTYPES[1:]):
        for b, M in enumerate(MS):
            for c, (N, K) in enumerate(SHAPES):
                for d, bs in enumerate(BLOCKSIZES64):
                    out16[:] = 0
                    ok = lib.bnb_mi355x_gemm_4bit_grad_input_plan(dtype, M, N, K, bs, addr)
                    rec = grad[a, b, c, d]
                    rec[0], rec[1:17] = ok, out16
                    rec[17] = lib.bnb_mi355x_gemm_4bit_grad_input_supported(dtype, M, N, K, bs)
                    rec[18] = lib.bnb_mi355x_gemm_4bit_grad_input_workspace_bytes(M, N, K)
    # the peer launcher's shape check reads the CU count as well (it must return; the kernels themselves are not run under an override)
    peer = np.array([[[lib.bnb_mi355x_gemv_4bit_peer_serves(world, ns, K, 64, mode, 16384, wg)
                       for wg in (0, 1, 64, 1024)] for mode in (0, 1, 2)]
                     for world in (1, 2, 8) for ns in (2, 512, 4096, 14336) for K in (64, 4096, 8192)], dtype=np.int64)
    out8 = np.zeros(8, dtype=np.int32)
    assert lib.bnb_mi355x_stream_geometry(0, 2, 1, 4096, 4096, 64, out8.ctypes.data) == 1
    exact = np.array([lib.bnb_mi355x_gemv_4bit_stream_exact(2, 1, 4096, 4096, 64, 0), out8[0], out8[4]], dtype=np.int64)
    return dict(plan=plan, preds=preds, forms=forms, grouped=grouped, grad=grad, peer=peer, exact=exact)


def main(argv):
    lib = load(argv[1])
    cus = int(argv[2])
    if cus:
        lib.bnb_mi355x_set_cu_count(cus)
    np.savez(argv[3], **sweep(lib))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
