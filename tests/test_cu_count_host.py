"""CPU (-m "not gpu"): every launch plan of the library at CU counts other than the test machine's.

Every plan asks ``device_cu_count_or_default()`` (csrc/bnb_common.h), and every GPU test answers for the 256 CUs of the machine that
ran it. An MI355X in DPX / QPX / CPX partition mode presents 128 / 64 / 32. ``bnb_mi355x_set_cu_count`` (thread-local, 0 = ask the
device) makes the calling thread's plans for another count, and ``bnb_mi355x_gemm_4bit_plan`` / ``_sm_form_plan`` /
``_grad_input_plan`` return a plan without the launch - computed by the launch's own functions. Here they are swept, per CU count in
(1, 8, 20, 32, 64, 80, 128, 256, 304), over three dtypes, M on either side of every row-instance boundary, small / ragged / model
(N, K) including the routed sweep's, blocksizes 32 ... 4096, plain and nested statistics - each count in a child process
(tests/checks/cu_count_sweep.py: a query that kills its process fails that count's tests) - and every answer is held against what
the KERNEL needs of it.

The plan functions that read the CU count, and the invariant that covers each:

* ``make_geometry`` (gemv4_stream.hip; ``R = ceil(rows / cus)``, the exact-geometry instance): the kernel walks ``row_begin =
  blockIdx.x * R`` and unpacks ``R = hot_geom & 0xFFFF``: test_stream_geometry_host.py's own checker, re-run at every count
  (test_stream_geometry_invariants_hold_at_every_cu_count), and grid_x * R >= N > (grid_x - 1) * R here; 4096 x 4096 M = 1 takes the
  exact instance with R = 32 / 64 / 128 at 128 / 64 / 32 CUs (test_exact_geometry_instance_follows_the_cu_count).
* ``sm_plan`` / ``sm_grouped_plan`` (gemm4_mfma_sm.hip; R, tiles, 16- or 32-row passes, the grouped launch's ``limit``): the kernel
  reads ``R = hot_geom & 0xFFFF``, ``row0 = block * R``, ``row_end = min(row0 + R, N)``, ``m_base = blockIdx.y * (16 * RB)``, and its
  TT tiles hold 16 TT rows; sm_launch_tt has instances for 1 ... 4 tiles (``default:`` is 4). So 16 <= R <= 16 tt <= 64, grid_x * R
  >= N > (grid_x - 1) * R (grouped: grid_x = sum ceil(N_i / R)), grid_y * 16 RB >= M > (grid_y - 1) * 16 RB, gated R even, fused forms
  in passes of at most 16 rows, 8 wavefronts from 16-row passes or 3 tiles on.
* ``rt_plan`` (gemm4_mfma_rt.hip; mt, ``ks = cus / (2 wgs)``, 8 or 16 wavefronts): ``col0 = blockIdx.x * 16``, ``m_base = blockIdx.z *
  (16 * MT)``, ``cb = blockIdx.y * hot_cps``, slab ``blockIdx.y * M * N``: ks * cps >= chunks > (ks - 1) * cps, every wavefront keeps a
  chunk (cps >= min(waves, chunks)), 16 wavefronts only at one row tile.
* ``kq_plan`` (gemm4_mfma_kq.hip; ``ks = cus / (gx * gz)``): ``col0 = blockIdx.x * 128``, ``m_base = blockIdx.z * (32 * MT)``, ``cb =
  blockIdx.y * hot_cps``: the same coverage; a slice holds at most 64 chunks (one change of the second-level absmax) and at least two
  where the row has two.
* ``make_plan`` (gemm4_mfma.hip; 64-column workgroups while ``wgs14 <= cus``): ``per_wg = ceil(chunks_total / hot_kslices)``; grid x
  covers N in 64 / 128 / 256 columns, at least two chunks per slice where the row has two.
* ``sm_selected`` (gemm4_mfma.hip; ``N >= 12 * cus``) and ``gemm_4bit_route`` (gemm4_mfma.hip): bnb_mi355x_gemm_4bit_route's answer is 1
  exactly where the plan names an MFMA family; the census (each family reached at 32, 64, 128 and 256 CUs).
* ``gi_plan`` (gemm4_grad_input.hip; ``ns = cus / wgs``): ``k0 = blockIdx.x * 128``, ``m_base = blockIdx.z * (16 * MT)``, ``bb =
  blockIdx.y * hot_bps``, slab ``blockIdx.y * M * K``: ns * bps >= blocks > (ns - 1) * bps, two blocks per wavefront and slice where the
  column has them, workspace = ns * M * K * 4 exactly when ns > 1.
* the quantizers' grid caps (quantize4.hip ``4 * cus``, blockwise8.hip ``2 * cus``): grid-stride loops - no host plan to query; the GPU
  module runs them at 32 CUs (tests/test_gpu_cu_count.py).
* ``gemv_4bit_peer_serves``: returns at every count (the peer-chain kernels are not run under an override: they poll across workgroups).

For every family: every grid dimension >= 1 and within HIP's limits (x < 2^31, y and z <= 65535), dynamic LDS within kLdsBudget =
156 KiB. Workspace: ``bnb_mi355x_gemm_4bit_workspace_bytes`` = slices * M * N * 4 when the plan splits K and 0 when not - for the
K-quarter kernel slices * whole 128 x 32 mt tiles (kq_slab_floats); at 17 rows and more the query cannot know whether the K-quarter
kernel will serve the statistics and answers with the larger of its need and the next family's (gemm_4bit_workspace_bytes), so
there the bound is >=, and equality is asserted up to 16 rows. At 256 the answers equal those without an override.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = os.path.join(ROOT, "tests", "checks")
sys.path.insert(0, CHECKS)
import cu_count_census as Census  # noqa: E402
import cu_count_sweep as C  # noqa: E402
import stream_geometry_sweep as G  # noqa: E402

sys.path.pop(0)
import cu_count_cases as Cases  # noqa: E402
import test_stream_geometry_host as StreamHost  # noqa: E402

LDS_BUDGET = 156 * 1024
K_STREAM, K_RT, K_PC, K_KQ, K_SM = 1, 3, 4, 6, 7
FAMILY = {K_STREAM: "stream", K_RT: "rt", K_PC: "pc", K_KQ: "kq", K_SM: "sm"}
MFMA = (K_RT, K_PC, K_KQ, K_SM)
STREAM_TUNINGS = "0,7"   # defaults and the 8-wavefront instances: the tunings whose R reads the CU count and whose G differs


def _library():
    from bitsandbytes_amd.cextension import LIB_PATH

    assert LIB_PATH.exists(), f"{LIB_PATH} is not built"
    return str(LIB_PATH)


def _pool(commands, jobs=8):
    """Run the commands, at most `jobs` at once: [(returncode, stderr)] in order."""
    results, running, todo = [None] * len(commands), [], list(enumerate(commands))
    while todo or running:
        while todo and len(running) < jobs:
            i, cmd = todo.pop(0)
            running.append((i, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        i, p = running.pop(0)
        _, err = p.communicate()
        results[i] = (p.returncode, err)
    return results


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """{cus: (returncode, stderr, npz path)} for every count and 0 (no override)."""
    tmp = tmp_path_factory.mktemp("cu_count")
    lib, child = _library(), os.path.join(CHECKS, "cu_count_sweep.py")
    counts = (0,) + C.CU_COUNTS
    outs = [str(tmp / f"cus{c}.npz") for c in counts]
    done = _pool([[sys.executable, child, lib, str(c), o] for c, o in zip(counts, outs)])
    return {c: (code, err, o) for c, (code, err), o in zip(counts, done, outs)}


def _load(sweeps, cus):
    code, err, out = sweeps[cus]
    assert code == 0, f"the sweep at {cus} CUs ended with status {code} (negative: killed by that signal; -8 = SIGFPE)\n{err[-2000:]}"
    return np.load(out)


def _first(bad, axes):
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return f"{int(bad.sum())} violations, first at " + ", ".join(f"{name} {values[j]}" for (name, values), j in zip(axes, i))


PLAN_AXES = (("dtype", C.DTYPES), ("M", C.MS), ("(N, K)", C.SHAPES), ("blocksize", C.BLOCKSIZES), ("nested", (0, 1)))


def _grid(Ms, shapes, blocksizes, lead=1, tail=1):
    """Broadcastable M, N, K, blocksize for an array [lead..., Ms, shapes, blocksizes, tail...]."""
    M = np.array(Ms, dtype=np.int64).reshape((1,) * lead + (-1, 1, 1) + (1,) * tail)
    N = np.array([s[0] for s in shapes], dtype=np.int64).reshape((1,) * lead + (1, -1, 1) + (1,) * tail)
    K = np.array([s[1] for s in shapes], dtype=np.int64).reshape((1,) * lead + (1, -1, 1) + (1,) * tail)
    bs = np.array(blocksizes, dtype=np.int64).reshape((1,) * lead + (1, 1, -1) + (1,) * tail)
    return M, N, K, bs


def _ceil(a, b):
    return (a + b - 1) // b


def check_family_plan(p, M, N, K, ok, say):
    """What every family's kernel needs of out16 (module docstring). p[..., i] = out16[i]; `say(cond, what)` asserts cond where ok."""
    fam, gx, gy, gz, slices, per, total, tiles, waves, rows_step, cols, extra, lds, unit, inst, flag = (p[..., i] for i in range(16))
    say((gx >= 1) & (gx < 2 ** 31) & (gy >= 1) & (gy <= 65535) & (gz >= 1) & (gz <= 65535), "grid dimensions within HIP's limits")
    say((lds > 0) & (lds <= LDS_BUDGET), "dynamic LDS within 156 KiB")
    say((waves == 8) | (waves == 12) | (waves == 16), "8, 12 or 16 wavefronts")
    m_steps = np.where((fam == K_STREAM) | (fam == K_SM), gy, gz)
    say((m_steps * rows_step >= M) & (M > (m_steps - 1) * rows_step), "the M axis covers the batch rows exactly once")
    say((gx * cols >= N) & (N > (gx - 1) * cols), "grid x covers the weight rows exactly once")
    st = fam == K_STREAM   # (its [5], [6] are phases and segments: checked below)
    say(st | ((slices >= 1) & (per >= 1) & (slices * per >= total) & (total > (slices - 1) * per)), "slices non-empty and slices x per-slice covers the row")
    say((total * unit >= K) & (K > (total - 1) * unit), "the units cover K")
    split = (fam == K_RT) | (fam == K_PC) | (fam == K_KQ)
    say(~split | ((gy == slices) & (total * unit == K)), "rt / pc / kq: grid y = K slices, whole 256-k chunks")
    say(split | (slices == 1), "stream / sm: one K slice")
    # ---- stream
    say(~st | ((extra >= 1) & (per * extra >= total) & (total > (per - 1) * extra) & (extra * inst <= waves) & (cols <= 0xFFFF)),
        "stream: P * SW >= S > (P - 1) * SW, SW * G <= waves, R in 16 bits")
    # ---- sm
    sm = fam == K_SM
    say(~sm | ((cols >= 16) & (cols <= extra) & (extra <= 64) & (tiles >= 1) & (tiles <= 4) & (extra == 16 * tiles)),
        "sm: 16 <= R <= 16 tt <= 64 (instances exist for 1 ... 4 tiles)")
    want_inst = np.where(M <= 4, 4, np.where(M <= 8, 8, 16))
    say(~sm | (inst == want_inst) | ((M > 16) & (inst == 32)), "sm: the rows instance follows M")
    say(~sm | ((rows_step == np.where(inst == 32, 32, 16)) & (waves == np.where((inst >= 16) | (tiles >= 3), 8, 16))), "sm: row step and wavefronts of the instance")
    # ---- rt
    rt = fam == K_RT
    say(~rt | ((tiles >= 1) & (tiles <= 4) & (rows_step == 16 * tiles) & (cols == 16) & ((waves == 8) | ((waves == 16) & (tiles == 1)))),
        "rt: 1 ... 4 row tiles, 16 wavefronts only at one")
    say(~rt | (per >= np.minimum(waves, total)), "rt: every wavefront keeps a chunk")
    # ---- kq
    kq = fam == K_KQ
    say(~kq | (((tiles == 1) | (tiles == 2)) & (rows_step == 32 * tiles) & (cols == 128) & (waves == 8)), "kq: one or two 32-row tiles, 128 columns")
    say(~kq | ((per <= 64) & (per >= np.minimum(2, total))), "kq: 2 <= chunks per slice <= 64")
    say(~kq | (extra * 1024 == _ceil(N, 128) * _ceil(M, 32 * tiles) * 4096 * tiles), "kq: the slab is whole workgroup tiles")
    # ---- pc
    pc = fam == K_PC
    say(~pc | ((tiles >= 1) & (tiles <= 4) & (rows_step == 16 * tiles) & ((cols == 64) | (cols == 128) | (cols == 256)) & (inst >= 2)),
        "pc: 1 ... 4 row tiles, 64 / 128 / 256 columns, a ring of at least two chunks")
    say(~pc | (per >= np.minimum(2, total)), "pc: two chunks per slice where the row has two")


def _sm_workgroups(rows, cus):
    """grid x of the streaming MFMA kernel's single-matrix plan (sm_plan: whole rounds of cus workgroups of at most 64 rows, 16 at least)."""
    rounds = _ceil(rows, cus * 64)
    return _ceil(rows, max(16, _ceil(rows, cus * rounds)))


def _need_workspace(p, M, N):
    fam, slices, tiles, extra = p[..., 0], p[..., 4], p[..., 7], p[..., 11]
    plain = slices * M * N * 4
    return np.where(slices > 1, np.where(fam == K_KQ, slices * extra * 1024 * 4, plain), 0)


@pytest.mark.parametrize("cus", C.CU_COUNTS)
def test_gemm_4bit_plans_hold_what_the_kernels_need(sweeps, cus):
    a = _load(sweeps, cus)["plan"]
    M, N, K, bs = _grid(C.MS, C.SHAPES, C.BLOCKSIZES)
    whole = np.broadcast_to(K % bs == 0, a.shape[:-1])
    ok = (a[..., 0] == 1) & whole
    assert set(np.unique(a[..., 0]).tolist()) <= {0, 1}
    p, route, ws = a[..., 1:17], a[..., 17], a[..., 18]

    def say(cond, what):
        bad = ok & ~np.broadcast_to(cond, ok.shape)
        assert not bad.any(), f"{cus} CUs: {what}: {_first(bad, PLAN_AXES)}"

    fam = p[..., 0]
    say(np.isin(fam, (K_STREAM,) + MFMA), "a routed family")
    check_family_plan(p, M, N, K, ok, say)
    # ---- every call below 2^32 weights whose K is whole blocks has a plan (the streaming kernel takes what no MFMA kernel does, to 511 segments)
    served = whole & np.broadcast_to((N * K < 2 ** 32) & (K <= 511 * 2048) & (K % 32 == 0), whole.shape)
    assert not (served & (a[..., 0] != 1)).any(), f"{cus} CUs: no plan: {_first(served & (a[..., 0] != 1), PLAN_AXES)}"
    # ---- the route query (plain statistics assumed; blocksize 32 with nested statistics has no MFMA kernel)
    nested = np.arange(2).reshape(1, 1, 1, 1, 2)
    say(np.where((bs == 32) & (nested == 1), fam == K_STREAM, (route == 1) == np.isin(fam, MFMA)), "bnb_mi355x_gemm_4bit_route agrees with the plan's family")
    say((np.array(C.DTYPES).reshape(-1, 1, 1, 1, 1) != 0) | (fam == K_STREAM), "fp32 activations: the streaming kernel")
    # ---- workspace
    need = np.where((bs == 32) & (nested == 1), ws, _need_workspace(p, M, N))   # (the size query assumes plain statistics, like the route query)
    say(np.where(route == 1, ws >= need, ws == 0), "the workspace query covers the plan's slabs; none off the MFMA route")
    say((route == 0) | (M > 16) | (ws == need), "up to 16 rows the workspace is exactly slices x M x N x 4, or 0 without a split")
    say((route == 0) | (ws == need) | ((ws % (M * N * 4) == 0) & (ws // (M * N * 4) >= 2)) | ((M > 16) & (ws % (4096 * 4) == 0)),
        "a larger workspace is the other candidate's: whole M x N slabs, or the K-quarter kernel's whole 4096-float tiles")


@pytest.mark.parametrize("cus", C.CU_COUNTS)
def test_fused_forms_and_grouped_plans(sweeps, cus):
    z = _load(sweeps, cus)
    f = z["forms"]
    M, N, K, bs = _grid(C.MS16, C.SHAPES, C.BLOCKSIZES64, lead=2)
    ok = (f[..., 0] == 1) & np.broadcast_to(K % bs == 0, f.shape[:-1])
    axes = (("form", (1, 2, 3)), ("dtype", C.DTYPES[1:]), ("M", C.MS16), ("(N, K)", C.SHAPES), ("blocksize", C.BLOCKSIZES64), ("nested", (0, 1)))

    def say(cond, what):
        bad = ok & ~np.broadcast_to(cond, ok.shape)
        assert not bad.any(), f"{cus} CUs: {what}: {_first(bad, axes)}"

    p = f[..., 1:17]
    say(p[..., 0] == K_SM, "the streaming MFMA kernel")
    check_family_plan(p, M, N, K, ok, say)
    form = np.arange(1, 4).reshape(-1, 1, 1, 1, 1, 1)
    say(p[..., 14] <= 16, "fused forms: row passes of at most 16")
    say((form != 1) | ((p[..., 10] % 2 == 0) & (N % 2 == 0)), "gated: R even (a workgroup starts on a gate row)")
    assert not (ok[0] & (np.arange(2).reshape(1, 1, 1, 1, 2) == 1)).any(), "gated: fp32 absmax only"
    assert ok.any(axis=(1, 2, 3, 4, 5)).all(), f"{cus} CUs: a fused form never ran the streaming MFMA kernel"
    # ---- the grouped launch: R raised until the members' own shares need no more workgroups than the plan's whole rounds
    g = z["grouped"]
    for i, heights in enumerate(C.GROUPS):
        for j, m in enumerate(C.MS):
            rec = g[i, j]
            assert (rec[0] == 1) == (rec[17] == 2), (cus, heights, m, "a plan exactly where the grouped route is one streaming MFMA launch")
            if rec[0] != 1:
                continue
            q = rec[1:17]
            R, tt = int(q[10]), int(q[7])
            assert q[0] == K_SM and 16 <= R <= 16 * tt <= 64 and q[11] == 16 * tt, (cus, heights, m, q.tolist())
            assert q[1] == sum(-(-n // R) for n in heights) and 1 <= q[1] < 2 ** 31, (cus, heights, m, "grid x = the members' own workgroups")
            assert q[2] * q[9] >= m > (q[2] - 1) * q[9] and q[2] <= 65535 and 0 < q[12] <= LDS_BUDGET, (cus, heights, m, q.tolist())
            limit = max(cus, _sm_workgroups(sum(heights), cus))
            assert q[1] <= limit or R == 64, (cus, heights, m, "the limit loop ends within the plan's rounds, or at four tiles", q.tolist())
    assert (g[:, :, 0] == 1).any(), "no grouped plan at all"


@pytest.mark.parametrize("cus", C.CU_COUNTS)
def test_grad_input_plans(sweeps, cus):
    a = _load(sweeps, cus)["grad"]
    M, N, K, bs = _grid(C.MS, C.SHAPES, C.BLOCKSIZES64, tail=0)
    assert (a[..., 0] == a[..., 17]).all(), "a plan exactly where bnb_mi355x_gemm_4bit_grad_input_supported"
    ok = a[..., 0] == 1
    axes = (("dtype", C.DTYPES[1:]), ("M", C.MS), ("(N, K)", C.SHAPES), ("blocksize", C.BLOCKSIZES64))

    def say(cond, what):
        bad = ok & ~np.broadcast_to(cond, ok.shape)
        assert not bad.any(), f"{cus} CUs: {what}: {_first(bad, axes)}"

    p = a[..., 1:17]
    gx, ns, gz, slices, bps, blocks, mt, waves, rows_step, lds = (p[..., i] for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12))
    say((gx == K // 128) & (gx >= 1) & (ns >= 1) & (ns <= 65535) & (gz >= 1) & (gz <= 65535) & (ns == slices), "grid: K / 128 x N slices x row passes")
    say((mt == np.where(M <= 16, 1, np.where(M <= 32, 2, 4))) & (rows_step == 16 * mt) & (gz * rows_step >= M) & (M > (gz - 1) * rows_step), "row tiles follow M; grid z covers M")
    say((blocks == N // 32) & (ns * bps >= blocks) & (blocks > (ns - 1) * bps), "ns * bps >= blocks > (ns - 1) * bps")
    say(bps >= np.minimum(2 * waves, blocks), "two blocks per wavefront and slice where the column has them")
    say((lds > 0) & (lds <= LDS_BUDGET) & (waves == 8), "LDS within 156 KiB, 8 wavefronts")
    say(a[..., 18] == np.where(ns > 1, ns * M * K * 4, 0), "workspace = ns x M x K x 4 exactly when ns > 1")
    assert ok.any() and (ok & (ns > 1)).any() == (cus >= 8)


def test_answers_at_256_equal_those_without_an_override(sweeps):
    base, forced = _load(sweeps, 0), _load(sweeps, 256)
    for name in base.files:
        assert np.array_equal(base[name], forced[name]), f"{name}: the override at 256 changes an answer of a host without a device"


def test_every_count_returns_from_the_predicates(sweeps):
    for cus in C.CU_COUNTS:
        z = _load(sweeps, cus)
        assert set(np.unique(z["preds"]).tolist()) <= {0, 1} and set(np.unique(z["peer"]).tolist()) <= {0, 1}
        assert z["preds"].any() and z["peer"].any()


def test_census_every_family_is_routed_at_every_partition_size(sweeps):
    """Each of stream, sm, rt, pc, kq is selected somewhere at 32, 64, 128 and 256 CUs - through the route, nothing forced."""
    for cus in (32, 64, 128, 256):
        a = _load(sweeps, cus)["plan"]
        reached = set(np.unique(a[..., 1][a[..., 0] == 1]).tolist())
        assert reached == {K_STREAM, K_RT, K_PC, K_KQ, K_SM}, f"{cus} CUs: the router never selects {[FAMILY[f] for f in FAMILY if f not in reached]}"


def test_exact_geometry_instance_follows_the_cu_count(sweeps):
    """4096 x 4096, M = 1: the exact-geometry instance (gemv4_stream.hip: exact_geometry - rows % R == 0, R % G == 0, R >= 2 G) with
    R = 4096 / cus at every partition size."""
    for cus, R in ((256, 16), (128, 32), (64, 64), (32, 128)):
        assert _load(sweeps, cus)["exact"].tolist() == [1, R, cus]


def test_stream_geometry_invariants_hold_at_every_cu_count(tmp_path_factory):
    """test_stream_geometry_host.py's checker, unchanged, on its own grid under each CU count (the tunings whose rows per workgroup
    come from the CU count: the defaults and the 8-wavefront instances)."""
    tmp = tmp_path_factory.mktemp("stream_geometry_cus")
    lib, child = _library(), os.path.join(CHECKS, "stream_geometry_sweep.py")
    jobs = [(cus, form, str(tmp / f"{form}{cus}.npz")) for cus in C.CU_COUNTS for form in G.FORMS]
    done = _pool([[sys.executable, child, lib, form, out, str(cus), STREAM_TUNINGS] for cus, form, out in jobs])
    for cus in C.CU_COUNTS:
        result = {form: (code, err, out if code == 0 else None) for (c, form, out), (code, err) in zip(jobs, done) if c == cus}
        for form in G.FORMS:
            try:
                StreamHost.test_geometry_invariants(result, form)
            except AssertionError as exc:
                raise AssertionError(f"{cus} CUs, {form}: {exc}") from None


def test_override_is_declared_exported_and_thread_local():
    import threading

    from bitsandbytes_amd import cextension as ce

    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    for decl in ("void bnb_mi355x_set_cu_count(int cus);",
                 "int bnb_mi355x_gemm_4bit_plan(int kernel, int dtype, int M, int N, int K, int blocksize, int nested, int* out16);",
                 "int bnb_mi355x_gemm_4bit_grad_input_plan(int dtype, int M, int N, int K, int blocksize, int* out16);"):
        assert decl in header
    for name in ("bnb_mi355x_set_cu_count", "bnb_mi355x_gemm_4bit_plan", "bnb_mi355x_gemm_4bit_sm_form_plan", "bnb_mi355x_gemm_4bit_grad_input_plan"):
        assert name in ce.EXPORTED_SYMBOLS
    out = np.full(16, -7, dtype=np.int32)
    lib = ce.lib
    assert lib.bnb_mi355x_gemm_4bit_plan(0, 2, 1, 8, 33, 64, 0, out.ctypes.data) == 0 and (out == -7).all()   # out16 untouched at 0
    seen = {}

    def other():
        lib.bnb_mi355x_gemm_4bit_plan(0, 2, 1, 4096, 4096, 64, 0, out.ctypes.data)
        seen["other"] = int(out[10])

    try:
        lib.bnb_mi355x_set_cu_count(32)
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert lib.bnb_mi355x_gemm_4bit_plan(0, 2, 1, 4096, 4096, 64, 0, out.ctypes.data) == 1 and out[10] == 128
        lib.bnb_mi355x_set_cu_count(-5)   # (negative: 0)
        assert lib.bnb_mi355x_gemm_4bit_plan(0, 2, 1, 4096, 4096, 64, 0, out.ctypes.data) == 1 and out[10] == seen["other"]
    finally:
        lib.bnb_mi355x_set_cu_count(0)


def test_committed_gpu_cases_still_differ_from_the_256_cu_plan():
    """tests/cu_count_cases.py is what tests/checks/cu_count_census.py picks today - so no committed cell has become a shape whose plan
    at its CU count equals the 256-CU plan (the GPU module would pass without exercising anything), and the cap holds."""
    picked = Census.pick(Census.load(_library()))
    assert Cases.GEMM_CELLS == picked["GEMM_CELLS"] and Cases.GRAD_CELLS == picked["GRAD_CELLS"], "re-run tests/checks/cu_count_census.py"
    assert len(Cases.GEMM_CELLS) <= 40
    for cell in Cases.GEMM_CELLS:
        assert any(a != b for a, b in zip(cell["plans"], cell["plans_256"])), cell
    for cell in Cases.GRAD_CELLS:
        assert cell["plan"] != cell["plan_256"], cell
