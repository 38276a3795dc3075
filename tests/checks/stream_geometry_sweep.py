"""Child process of tests/test_stream_geometry_host.py: one FORM of bnb_mi355x_stream_geometry over the whole grid, in a process of
its own - a query that kills its process (a division by zero in the host geometry did) is then a failed form, not a dead pytest.

    python stream_geometry_sweep.py <library> <form> <out.npz> [<cus> [<tuning indices, comma separated>]]

<cus>: the sweep runs under bnb_mi355x_set_cu_count(cus) (tests/test_cu_count_host.py; absent or 0: the device's count, 256 without
one), over the named subset of TUNINGS (absent: all of them).

Needs ctypes and numpy only: no torch, no GPU, nothing preloaded. Writes, per (tuning, dtype, M) in grid order, the answers as
int32 [tunings, dtypes, Ms, rows, Ks, 9] = (supported, R, SW, G, P, grid_x, lds, mb, waves); the invariants are asserted by the parent.

    python stream_geometry_sweep.py <library> gated-query <dtype> <M> <N> <K> <blocksize>

prints bnb_mi355x_gemm_4bit_gated_supported's answer.
"""
import ctypes as ct
import sys

import numpy as np

FORMS = ("plain", "grouped", "gated", "lora", "lora_ids")
DTYPES = (0, 1, 2)   # fp32, fp16, bf16
MS = (1, 2, 3, 4, 5, 16)
KS = tuple(2048 * s + d for s in range(511) for d in (32, 1024, 2048))
ROWS = (1, 2, 3, 8, 255, 256, 257, 258, 514, 4096, 1764353)
# (ring_depth, segments, rows_per_workgroup, nontemporal, waves): the defaults, then test_stream_kernel_geometry_independent's settings
TUNINGS = ((0, 0, 0, -1, 0), (2, 0, 0, -1, 0), (3, 0, 0, -1, 0), (6, 0, 0, -1, 0), (0, 1, 0, -1, 0), (0, 0, 3, -1, 0), (0, 0, 0, 0, 0),
           (0, 0, 0, -1, 8), (0, 2, 7, 0, 8))
BLOCKSIZE = 64


def load(path):
    lib = ct.CDLL(path)
    lib.bnb_mi355x_stream_geometry.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_long, ct.c_int, ct.c_int, ct.c_void_p]
    lib.bnb_mi355x_stream_geometry.restype = ct.c_int
    lib.bnb_mi355x_set_stream_tuning.argtypes = [ct.c_int] * 5
    lib.bnb_mi355x_set_stream_tuning.restype = None
    lib.bnb_mi355x_gemm_4bit_gated_supported.argtypes = [ct.c_int] * 5
    lib.bnb_mi355x_gemm_4bit_gated_supported.restype = ct.c_int
    return lib


def sweep(lib, form: int, tunings=TUNINGS) -> np.ndarray:
    out = np.zeros((len(tunings), len(DTYPES), len(MS), len(ROWS), len(KS), 9), dtype=np.int32)
    query = lib.bnb_mi355x_stream_geometry
    base = out.ctypes.data
    addr = base + 4   # (entry 0 of a record is the answer, filled in at the end)
    answers = []
    for tune in tunings:
        lib.bnb_mi355x_set_stream_tuning(*tune)
        for dtype in DTYPES:
            for M in MS:
                for rows in ROWS:
                    for K in KS:
                        answers.append(query(form, dtype, M, rows, K, BLOCKSIZE, addr))
                        addr += 36
    lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)
    out[..., 0] = np.array(answers, dtype=np.int32).reshape(out.shape[:-1])
    return out


def main(argv):
    lib = load(argv[1])
    if argv[2] == "gated-query":
        print(lib.bnb_mi355x_gemm_4bit_gated_supported(*[int(a) for a in argv[3:8]]))
        return 0
    tunings = TUNINGS
    if len(argv) > 4 and int(argv[4]) > 0:
        lib.bnb_mi355x_set_cu_count.argtypes = [ct.c_int]
        lib.bnb_mi355x_set_cu_count.restype = None
        lib.bnb_mi355x_set_cu_count(int(argv[4]))
    if len(argv) > 5:
        tunings = tuple(TUNINGS[int(i)] for i in argv[5].split(","))
    np.savez(argv[3], answers=sweep(lib, FORMS.index(argv[2]), tunings))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
