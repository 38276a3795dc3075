"""CPU (-m "not gpu"): the launch geometry of the streaming kernel, over the whole range its predicates accept.

``bnb_mi355x_stream_geometry`` returns what a launch would use - computed by the launch's own functions (csrc/gemv4_stream.hip:
rows_waves, launch_plan, make_geometry), under the calling thread's stream tuning - without a launch. Here it is swept over every
segment count the kernel accepts (K = 32 ... 511 * 2048), every activation dtype, M on every row-instance, row counts on either side
of the CU count and of the points where the rows per workgroup change, every form, the defaults and the tuning settings of
test_stream_kernel_geometry_independent; and every answer is held against what the KERNEL needs of it:

* argument packing (gemv4_stream.hip, kernel head: ``R = hot_geom & 0xFFFF, SW = (hot_geom >> 16) & 31, G = (hot_geom >> 21) & 31``
  and ``P = (hot_packed >> 23) & 511``; launch_one packs ``ge.R | ge.SW << 16 | ge.G << 21`` and ``... | ge.P << 23``):
  1 <= R <= 0xFFFF, 1 <= SW <= 31, 1 <= G <= 31, 1 <= P <= 511;
* wavefront (sw, g) = (wave % SW, wave / SW) must exist for every segment column and row group: SW * G <= waves;
* the phase loop ``for (ph = 0; ph < P; ++ph)`` with ``seg = ph * SW + sw`` covers segments 0 ... S - 1 exactly when
  P * SW >= S > (P - 1) * SW;
* ``row_begin = blockIdx.x * R`` covers the rows exactly when grid_x * R >= rows > (grid_x - 1) * R;
* the LDS map ``table | nested code(s) (1 KiB per matrix) + 64 | activation image [MB][SW][2048] T | segment partials [R][S][MB]``
  (``part[(rl * S + seg) * MB + m]``): lds = 65536 + (8 if grouped else 1) * 1024 + 64 + MB * SW * 2048 * sizeof(T) +
  align16(R * S * MB * 4), within kLdsBudget = 156 KiB, the largest dynamic allocation that launches;
* gated (``out[m, pair]`` from rows 2 i, 2 i + 1 of ONE workgroup): R even and >= 2, rows even;
* grouped instances have no phase loop: P == 1;
* SW and P are functions of (K, mb, waves, dtype, tuning) alone - not of rows, grouped or pairs: what rows_waves rests on.

Each form runs in a child process (tests/checks/stream_geometry_sweep.py: ctypes + numpy, no GPU, nothing preloaded), all five at
once: a query that kills its process fails that form's test. One did: bnb_mi355x_gemm_4bit_gated_supported(bf16, M = 3, N = 2,
K = 1046528, 64) divided by zero in make_geometry (R = 1 under ``pairs`` with r_cap = 1 became 0).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "checks", "stream_geometry_sweep.py")
sys.path.insert(0, os.path.dirname(CHILD))
import stream_geometry_sweep as G  # noqa: E402

sys.path.pop(0)

LDS_BUDGET = 156 * 1024
SEG_K = 2048


def _library():
    from bitsandbytes_amd.cextension import LIB_PATH

    assert LIB_PATH.exists(), f"{LIB_PATH} is not built"
    return str(LIB_PATH)


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """{form: (returncode, stderr, answers or None)}: the five children, started together."""
    tmp = tmp_path_factory.mktemp("stream_geometry")
    lib = _library()
    procs = {}
    for form in G.FORMS:
        out = str(tmp / f"{form}.npz")
        procs[form] = (subprocess.Popen([sys.executable, CHILD, lib, form, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), out)
    result = {}
    for form, (p, out) in procs.items():
        _, err = p.communicate()
        result[form] = (p.returncode, err, out if p.returncode == 0 else None)
    return result


def _answers(sweeps, form):
    code, err, out = sweeps[form]
    assert code == 0, f"the {form} sweep's process ended with status {code} (negative: killed by that signal; -8 = SIGFPE)\n{err[-2000:]}"
    return np.load(out)["answers"].astype(np.int64)


def _axes():
    """Broadcastable index arrays over [tunings, dtypes, Ms, rows, Ks]."""
    tune_sw = np.array([t[1] for t in G.TUNINGS]).reshape(-1, 1, 1, 1, 1)
    tbytes = np.array([4 if d == 0 else 2 for d in G.DTYPES]).reshape(1, -1, 1, 1, 1)
    M = np.array(G.MS).reshape(1, 1, -1, 1, 1)
    rows = np.array(G.ROWS, dtype=np.int64).reshape(1, 1, 1, -1, 1)
    K = np.array(G.KS, dtype=np.int64).reshape(1, 1, 1, 1, -1)
    return tune_sw, tbytes, M, rows, K


def _where(bad):
    """The first violating grid point, named."""
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return f"{int(bad.sum())} violations, first at tuning {G.TUNINGS[i[0]]} dtype {G.DTYPES[i[1]]} M {G.MS[i[2]]} rows {G.ROWS[i[3]]} K {G.KS[i[4]]}"


def _check(cond, ok, what):
    bad = ok & ~cond
    assert not bad.any(), f"{what}: {_where(bad)}"


@pytest.mark.parametrize("form", G.FORMS)
def test_geometry_invariants(sweeps, form):
    a = _answers(sweeps, form)
    ok = a[..., 0] == 1
    R, SW, Gr, P, grid, lds, mb, waves = (a[..., i] for i in range(1, 9))
    _, tbytes, M, rows, K = _axes()
    S = (K + SEG_K - 1) // SEG_K
    fits = rows * K < 2 ** 32
    grouped, gated, fused = form == "grouped", form == "gated", form in ("gated", "lora", "lora_ids")
    assert set(np.unique(a[..., 0]).tolist()) <= {0, 1}
    # ---- what must be served and what must be refused
    assert not (ok & ~fits).any(), f"served at rows * K >= 2^32: {_where(ok & ~fits)}"
    sixteen_bit = np.broadcast_to(tbytes == 2, ok.shape)
    if form == "plain":
        assert (ok == np.broadcast_to(fits, ok.shape)).all(), f"the plain form serves exactly rows * K < 2^32: {_where(ok != fits)}"
    if form in ("lora", "lora_ids"):
        assert (ok == (fits & sixteen_bit)).all(), f"the LoRA forms serve 16-bit activations at rows * K < 2^32: {_where(ok != (fits & sixteen_bit))}"
    if gated:
        assert not (ok & ~sixteen_bit).any() and not (ok & (rows % 2 == 1)).any(), "gated: 16-bit activations, an even row count"
        # (default tuning) whatever fits two rows of partial sums beside the image is served
        even = [G.ROWS.index(r) for r in (2, 8, 256, 258, 514, 4096)]
        assert (ok[0][1:, :2][:, :, even] == np.broadcast_to(fits, ok.shape)[0][1:, :2][:, :, even]).all(), "gated M = 1, 2 at even rows: served wherever rows * K < 2^32"
    if grouped:
        assert not (ok & (M > 4)).any(), "grouped: M <= 4"
        # (default tuning) one segment at M <= 4 in every dtype; 8 segments - one phase of the one-row instance with the `waves` knob at
        # rest and at 8 (grouped_fits) - in 16 bits
        assert ok[0][:, :4, :-1, G.KS.index(2048)].all() and ok[0][1:, 0, :-1, G.KS.index(8 * 2048)].all(), "grouped one-phase rows are served"
    assert ok.any()
    # ---- the instance
    _check((mb == np.where(M == 1, 1, np.where(M == 2, 2, 4))) & ((waves == 8) | (waves == 16)), ok, "mb follows M; 8 or 16 wavefronts")
    if fused:
        _check(tbytes == 2, ok, "fused forms: 16-bit activations")
        _check((mb != 1) | (waves == 16), ok, "no fused 1 x 8 instance")
    # ---- argument packing and coverage
    _check((R >= 1) & (R <= 0xFFFF), ok, "1 <= R <= 0xFFFF (16 bits of hot_geom)")
    _check((SW >= 1) & (SW <= 31) & (Gr >= 1) & (Gr <= 31), ok, "1 <= SW, G <= 31 (5 bits each of hot_geom)")
    _check(SW * Gr <= waves, ok, "SW * G <= waves")
    _check((P >= 1) & (P <= 511), ok, "1 <= P <= 511 (9 bits of hot_packed)")
    _check((P * SW >= S) & (S > (P - 1) * SW), ok, "P * SW >= S > (P - 1) * SW")
    _check((grid * R >= rows) & (rows > (grid - 1) * R), ok, "grid_x * R >= rows > (grid_x - 1) * R")
    # ---- LDS
    fixed = 65536 + (8 if grouped else 1) * 1024 + 64
    want_lds = fixed + ((R * S * mb * 4 + 15) & ~15) + mb * SW * SEG_K * tbytes
    _check(lds == want_lds, ok, "lds = fixed + align16(R S mb 4) + mb SW 2048 tbytes")
    _check(lds <= LDS_BUDGET, ok, "the LDS request stays within 156 KiB")
    # ---- per form
    if gated:
        _check((R >= 2) & (R % 2 == 0) & (rows % 2 == 0), ok, "gated: R even and >= 2, rows even")
    if grouped:
        _check(P == 1, ok, "grouped: one phase")
    # ---- SW, P, mb, waves do not depend on rows
    for name, v in (("SW", SW), ("P", P), ("mb", mb), ("waves", waves)):
        served = np.where(ok, v, -1)
        top = served.max(axis=3, keepdims=True)
        assert not (ok & (v != top)).any(), f"{name} depends on the row count: {_where(ok & (v != top))}"


def test_segment_columns_do_not_depend_on_the_form(sweeps):
    """SW and P of two forms agree wherever both serve the shape with the same (mb, waves) - `fixed` (grouped) and `pairs` (gated) do
    not feed back into them. (Under the `waves` knob the plain and grouped forms run 8 wavefronts and the fused forms 16: not compared.)"""
    tables = {}
    for form in G.FORMS:
        a = _answers(sweeps, form)
        ok = a[..., 0] == 1
        # one row count is enough (the test above): the served entry with the largest SW over the rows axis
        pick = np.where(ok[..., None], a[..., [2, 4, 7, 8]], -1).max(axis=3)
        tables[form] = pick
    compared = 0
    for form in G.FORMS[1:]:
        both = (tables["plain"][..., 0] > 0) & (tables[form][..., 0] > 0) & (tables["plain"][..., 2:] == tables[form][..., 2:]).all(axis=-1)
        compared += int(both.sum())
        differ = both & (tables["plain"][..., :2] != tables[form][..., :2]).any(axis=-1)
        assert not differ.any(), f"plain and {form} differ in (SW, P) at {[int(v[0]) for v in np.nonzero(differ)]} (tuning, dtype, M, K indices)"
    assert compared > 100000


def test_the_recorded_crash_is_a_refusal():
    """bnb_mi355x_gemm_4bit_gated_supported(bf16, M = 3, N = 2, K = 1046528, 64): S = 511, mb = 4, SW = 5, 80 KiB of image, room for the
    partial sums of ONE row - no (gate, up) pair fits a workgroup. The answer is 0; it was a SIGFPE."""
    p = subprocess.run([sys.executable, CHILD, _library(), "gated-query", "2", "3", "2", "1046528", "64"], capture_output=True, text=True)
    assert p.returncode == 0, f"the query's process ended with status {p.returncode} (-8 = SIGFPE)\n{p.stderr[-2000:]}"
    assert p.stdout.strip() == "0"
    for N in (2, 8):   # (fewer rows than the streaming MFMA kernel takes: the streaming kernel's answer) every M of the 4-row instance
        for M in (3, 4):
            q = subprocess.run([sys.executable, CHILD, _library(), "gated-query", "2", str(M), str(N), "1046528", "64"], capture_output=True, text=True)
            assert (q.returncode, q.stdout.strip()) == (0, "0"), (M, N, q.returncode, q.stdout, q.stderr[-500:])


def test_query_is_declared_and_exported():
    from bitsandbytes_amd import cextension as ce

    assert "bnb_mi355x_stream_geometry" in ce.EXPORTED_SYMBOLS
    assert len(ce.lib.bnb_mi355x_stream_geometry.argtypes) == 7
    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    assert "int bnb_mi355x_stream_geometry(int form, int dtype, int M, long rows, int K, int blocksize, int* out8);" in header
    # out8 stays untouched where the answer is 0
    out = np.full(8, -7, dtype=np.int32)
    assert ce.lib.bnb_mi355x_stream_geometry(0, 2, 1, 8, 33, 64, out.ctypes.data) == 0 and (out == -7).all()
    assert ce.lib.bnb_mi355x_stream_geometry(0, 2, 1, 8, 511 * 2048 + 32, 64, out.ctypes.data) == 0 and (out == -7).all()
    assert ce.lib.bnb_mi355x_stream_geometry(5, 2, 1, 8, 64, 64, out.ctypes.data) == 0 and (out == -7).all()
    assert ce.lib.bnb_mi355x_stream_geometry(0, 2, 1, 4096, 4096, 64, out.ctypes.data) == 1
    assert out.tolist() == [16, 2, 8, 1, 256, 65536 + 1024 + 64 + 16 * 2 * 4 + 2 * 2048 * 2, 1, 16]   # the exact-geometry shape on 256 CUs
