#!/usr/bin/env python3
"""Host census (no GPU): the smallest shapes at which a launch plan under a CU-count override differs from the 256-CU plan - the
cells tests/test_gpu_cu_count.py runs. Asks bnb_mi355x_gemm_4bit_plan / _grad_input_plan (the launch's own plan functions) only.

    python tests/checks/cu_count_census.py            rewrites tests/cu_count_cases.py and the census part of profiles/cu_count_census.txt

Grid: N in {96, 1088, 1216, 4096, 5120, 11008} x K in {256, 384, 2752, 4096, 8192} x blocksize in {32, 64, 128} x plain / nested
statistics (K a multiple of the blocksize), bf16, M from tests/checks/cu_count_sweep.py's list up to fused_max_m + 1. For each override
(32, 64, 128) and each family (stream, sm, rt, pc, kq) two cells, each the one with the smallest N * K (ties: smaller blocksize, plain
first, smaller N):

  plan   the family serves some M at the override AND at 256 CUs, with a different plan tuple
  route  the family serves some M at the override that another family serves at 256 CUs

A cell runs the M at which that holds (all of them, of both kinds and every family - at most the M list). "never" where the grid has no
such cell. The fused backward: per override and row-tile count (M = 8, 32, 64: 1, 2, 4 tiles) the smallest N * K whose plan differs,
plus the smallest with several N slices and the smallest with one where 256 CUs have several.
"""
import ctypes as ct
import os
import pprint
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cu_count_sweep as C  # noqa: E402

sys.path.pop(0)

OVERRIDES = (32, 64, 128)
NS = (96, 1088, 1216, 4096, 5120, 11008)
KS = (256, 384, 2752, 4096, 8192)
BLOCKSIZES = (32, 64, 128)
FAMILY = {1: "stream", 7: "sm", 3: "rt", 4: "pc", 6: "kq"}
GRAD_MS = (8, 32, 64)
DT_BF16 = 2


def load(path):
    return C.load(path)


def fused_max_m(lib, N, K, blocksize, nested):
    return lib.bnb_mi355x_gemm_4bit_fused_max_m(DT_BF16, N, K, blocksize, nested)


def _plan(lib, cus, M, N, K, bs, nested):
    out = np.zeros(16, dtype=np.int32)
    lib.bnb_mi355x_set_cu_count(cus)
    try:
        ok = lib.bnb_mi355x_gemm_4bit_plan(0, DT_BF16, M, N, K, bs, nested, out.ctypes.data)
    finally:
        lib.bnb_mi355x_set_cu_count(0)
    return tuple(int(v) for v in out) if ok == 1 else None


def _grad_plan(lib, cus, M, N, K):
    out = np.zeros(16, dtype=np.int32)
    lib.bnb_mi355x_set_cu_count(cus)
    try:
        ok = lib.bnb_mi355x_gemm_4bit_grad_input_plan(DT_BF16, M, N, K, 64, out.ctypes.data)
    finally:
        lib.bnb_mi355x_set_cu_count(0)
    return tuple(int(v) for v in out) if ok == 1 else None


def pick(lib):
    shapes = sorted(((N, K, bs, nested) for N in NS for K in KS for bs in BLOCKSIZES for nested in (0, 1) if K % bs == 0),
                    key=lambda s: (s[0] * s[1], s[2], s[3], s[0]))
    base = {}
    for s in shapes:
        ms = [m for m in C.MS if m <= fused_max_m(lib, *s) + 1]
        base[s] = (ms, [_plan(lib, 256, m, *s) if m <= fused_max_m(lib, *s) else None for m in ms])
    cells, report = {}, []
    for cus in OVERRIDES:
        here = {s: [_plan(lib, cus, m, *s) if m <= fused_max_m(lib, *s) else None for m in base[s][0]] for s in shapes}
        for fam, name in FAMILY.items():
            for kind in ("plan", "route"):
                found = None
                for s in shapes:
                    hits = [a is not None and b is not None and a[0] == fam and a != b and ((b[0] == fam) == (kind == "plan")) for a, b in zip(here[s], base[s][1])]
                    if any(hits):
                        found = s
                        break
                if found is None:
                    report.append(f"{cus:4d} CUs  {name:6s} {kind:5s}  never (no cell of the grid)")
                    continue
                cells.setdefault((cus,) + found, []).append(f"{name} {kind}")
                i = hits.index(True)
                report.append(f"{cus:4d} CUs  {name:6s} {kind:5s}  N {found[0]} K {found[1]} blocksize {found[2]} {'nested' if found[3] else 'plain'}  "
                              f"first at M {base[found][0][i]}: {here[found][i]}  (256 CUs: {base[found][1][i]})")
    gemm = []
    for (cus, N, K, bs, nested), why in sorted(cells.items()):
        s = (N, K, bs, nested)
        ms, b = base[s]
        a = [_plan(lib, cus, m, *s) if m <= fused_max_m(lib, *s) else None for m in ms]
        keep = [i for i in range(len(ms)) if a[i] is not None and a[i] != b[i]]
        gemm.append(dict(cus=cus, N=N, K=K, blocksize=bs, nested=bool(nested), why=why, Ms=[ms[i] for i in keep], plans=[a[i] for i in keep],
                         plans_256=[b[i] for i in keep]))
    grad, gshapes = [], sorted(((N, K) for N in NS for K in KS if N % 64 == 0 and K % 128 == 0), key=lambda s: (s[0] * s[1], s[0]))
    for cus in OVERRIDES:
        chosen = {}
        for M in GRAD_MS:
            wants = {f"{M} rows": lambda a, b: a != b, f"{M} rows, several slices": lambda a, b: a != b and a[4] > 1,
                     f"{M} rows, one slice (256 CUs: several)": lambda a, b: a[4] == 1 and b[4] > 1}
            for label, want in wants.items():
                for N, K in gshapes:
                    a, b = _grad_plan(lib, cus, M, N, K), _grad_plan(lib, 256, M, N, K)
                    if a is not None and b is not None and want(a, b):
                        chosen.setdefault((M, N, K), []).append(label)
                        report.append(f"{cus:4d} CUs  grad_input {label}:  N {N} K {K}: {a}  (256 CUs: {b})")
                        break
                else:
                    report.append(f"{cus:4d} CUs  grad_input {label}:  never (no cell of the grid)")
        for (M, N, K), why in sorted(chosen.items()):
            grad.append(dict(cus=cus, M=M, N=N, K=K, why=why, plan=_grad_plan(lib, cus, M, N, K), plan_256=_grad_plan(lib, 256, M, N, K)))
    return dict(GEMM_CELLS=gemm, GRAD_CELLS=grad, report=report)


HEADER = '''"""The cells of tests/test_gpu_cu_count.py: literal data, written by tests/checks/cu_count_census.py (do not edit; re-run it).
GEMM_CELLS: (shape, CU count) with the batch sizes whose plan differs from the 256-CU plan, both plan tuples (bnb_mi355x_gemm_4bit_plan's
out16) per batch size. GRAD_CELLS: the same for the fused backward (bnb_mi355x_gemm_4bit_grad_input_plan)."""
'''


def main():
    from bitsandbytes_amd.cextension import LIB_PATH

    picked = pick(load(str(LIB_PATH)))
    with open(os.path.join(ROOT, "tests", "cu_count_cases.py"), "w") as f:
        f.write(HEADER)
        for name in ("GEMM_CELLS", "GRAD_CELLS"):
            f.write(f"\n{name} = " + pprint.pformat(picked[name], width=150, compact=True, sort_dicts=False) + "\n")
    path = os.path.join(ROOT, "profiles", "cu_count_census.txt")
    tail = ""
    if os.path.exists(path):
        text = open(path).read()
        if "\n# ---- measured" in text:
            tail = text[text.index("\n# ---- measured"):]
    with open(path, "w") as f:
        f.write("# CU-count census (tests/checks/cu_count_census.py; host only): per override and family, the cell of the grid with the\n"
                "# smallest N * K whose plan tuple (plan) or whose family (route) differs from the 256-CU one, or never. Plan tuples:\n"
                "# bnb_mi355x_gemm_4bit_plan's out16 (include/bnb_mi355x.h).\n")
        f.write("\n".join(picked["report"]) + "\n")
        f.write(f"# cells run on the GPU: {len(picked['GEMM_CELLS'])} gemm_4bit (cap 40), {len(picked['GRAD_CELLS'])} fused backward\n")
        f.write(tail)
    print("\n".join(picked["report"]))
    print(len(picked["GEMM_CELLS"]), "gemm cells,", len(picked["GRAD_CELLS"]), "grad cells")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
