"""CPU (-m "not gpu"): what tests/test_gpu_guard_fused.py relies on, proven without a device - the carving helper
(tests/guard_bands.py on device="cpu"), the draws of tests/checks/guard_fused.py for the seed and draw count that ship (every draw
inside the header's preconditions, every listed shape, the id mixes, the family shares), and a ledger of the launching entry
points of include/bnb_mi355x.h: each one runs between guard bands in guard_stress.py or guard_fused.py, or is exempt with a reason."""
import importlib.util
import os
import random
import re

import pytest
import torch

import experts_cases as EC
import guard_bands as GB
from conftest import ROOT

DRAWS, SEED = 24, 11  # (tests/test_gpu_guard_fused.py's arguments)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "checks", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GF = _load("guard_fused")


def _lib():
    import bitsandbytes_amd as bnb

    return bnb.lib


def _all(section):
    return GF.draws(section, DRAWS, SEED)


# ------------------------------------------------------------------------------------------ the helper
def test_a_write_next_to_the_region_is_seen_and_one_inside_is_not():
    for fill in (GB.PAT, GB.NAN_PAT):
        for off in (0, 16, 2, 498):
            c = GB.Carved(100, off, device="cpu", fill=fill)
            assert c.ptr() % 256 == off % 256 and c.guards_ok()
            c.view[:] = 0x11
            c.view[0], c.view[99] = 0x22, 0x33
            assert c.guards_ok()
            for where in (c.start - 1, c.start + c.nbytes, 0, c.buf.numel() - 1):
                old = int(c.buf[where])
                c.buf[where] = old ^ 0x01
                assert not c.guards_ok(), (fill, off, where)
                c.buf[where] = old
            assert c.guards_ok()
    empty = GB.Carved(0, 4, device="cpu")
    assert empty.guards_ok() and GB.read(empty, torch.float32, 0).numel() == 0


def test_put_read_and_the_old_entry_points_of_guard_stress():
    rng = random.Random(3)
    t = torch.arange(24, dtype=torch.float32).view(4, 6)
    c = GB.carve_in(t, rng, device="cpu")
    assert c.ptr() % 4 == 0 and c.fill == GB.PAT and torch.equal(GB.read(c, torch.float32, 24).view(4, 6), t) and c.guards_ok()
    assert torch.equal(c.as_tensor(torch.float32, (4, 6)), t)
    o = GB.carve_out(64, rng, 2, device="cpu")
    assert o.ptr() % 2 == 0 and o.after >= GB.G and bool((o.bytes() == GB.PAT).all())
    # the same draws from the same generator state: guard_stress.py's placements do not move
    a, b = random.Random(5), random.Random(5)
    assert GB.carve_in(t, a, device="cpu").ptr() % 256 == (4 * b.randint(0, 31)) % 256


def test_offset_for_gives_exactly_the_alignment_asked_for():
    rng = random.Random(1)
    seen = set()
    for _ in range(200):
        c = GB.Carved(64, GB.offset_for(16, rng), device="cpu")
        assert c.ptr() % 16 == 0 and c.ptr() % 32 == 16
        seen.add(c.ptr() % 512)
        for align in (1, 2, 4, 8):
            off = GB.offset_for(align, rng)
            assert off % align == 0 and off % (2 * align) == align and off <= GB.MAX_OFF
        assert (GB.offset_for(2, rng) // 2) % 2 == 1  # (an odd element offset)
        p = GB.place(16, rng)
        assert p % 16 == 0 and 0 <= p <= GB.MAX_OFF
    assert len(seen) == 16
    kinds = [GB.place(16, random.Random(s)) % 32 for s in range(64)]
    assert 0 in kinds and 16 in kinds  # (both halves: exactly 16, and multiples that may be more aligned)


def test_the_band_behind_an_output_reaches_the_largest_row_count():
    assert GB.after_band(100) == GB.G and GB.after_band(16 * 4352 * 2) == 16 * 4352 * 2
    for M, N in ((3, 4352), (1, 7), (16, 2001)):
        c = GB.carve_out(M * N * 2, None, 16, device="cpu", after=GB.after_band(16 * N * 2), off=48)
        assert c.after >= max(8192, 16 * N * 2)
        hi = c.bands()[1]
        assert hi.numel() == c.after and c.start + M * N * 2 + (16 - M) * N * 2 <= c.buf.numel()  # (rows M ... 15 land in the band)
        hi[(16 - M) * N * 2 - 1] = 0
        assert not c.guards_ok()
    # guard_fused.py's sizes: 16 rows (decode ops), P + 4 pairs (experts), 16 R elements (shrink)
    src = open(os.path.join(ROOT, "tests", "checks", "guard_fused.py")).read()
    assert "pl.out(M * width * es, 16 * width * es)" in src and "pl.out(P * width * es, (P + 4) * width * es)" in src
    assert "pl.out(M * R * 2, 16 * R * 2)" in src


def test_input_bands_read_as_nan_and_as_no_adapter():
    c = GB.carve_in(torch.zeros(8, dtype=torch.float32), None, device="cpu", fill=GB.NAN_PAT, off=16)
    lo, hi = c.bands()
    for band in (lo[-64:], hi[:64]):
        band = band.clone()
        for dtype in (torch.float16, torch.bfloat16, torch.float32):
            assert bool(torch.isnan(band.view(dtype)).all())
        for dtype in (torch.int32, torch.int64):
            assert bool((band.view(dtype) == -1).all())
    assert c.guards_ok() and bool((c.bytes() == 0).all())


# ------------------------------------------------------------------------------------------ the generator
def test_draws_are_a_function_of_their_arguments():
    for section in GF.SECTIONS:
        assert GF.draws(section, DRAWS, SEED) == GF.draws(section, DRAWS, SEED)
        assert len(GF.draws(section, DRAWS, SEED)) == (len(GF.GUARD_SHAPES) if section == "python_guards" else DRAWS)
    assert GF.draws("lora", DRAWS, SEED) != GF.draws("lora", DRAWS, SEED + 1)
    with pytest.raises(ValueError):
        GF.draws("nothing", 1, 1)


def _id_kinds(ids, A_n):
    return {("in" if 0 <= i < A_n else "minus" if i == -1 else "A_n" if i == A_n else "alias" if i == GF.ALIAS else "other") for i in ids}


@pytest.mark.parametrize("section", ("gated", "lora", "lora_ids"))
def test_decode_draws_are_inside_the_preconditions_and_cover_the_lists(section):
    ds = _all(section)
    lib = _lib()
    fams = {GF.K_STREAM: 0, GF.K_SM: 0}
    for d in ds:
        M, N, K, bs = d["M"], d["N"], d["K"], d["bs"]
        assert d["dtype"] in ("bf16", "fp16") and 1 <= M <= 16 and N >= 1 and bs in (64, 128) and K % bs == 0 and d["qt"] in ("nf4", "fp4")
        fam = GF.predicted_family(M, N, K)
        if section == "gated":
            assert N % 2 == 0 and not d["nested"]
            sup = lib.bnb_mi355x_gemm_4bit_gated_supported(GF.DT_CODE[d["dtype"]], M, N, K, bs) if lib else 1
        else:
            assert d["r"] in GF.RANKS
            sup = lib.bnb_mi355x_gemm_4bit_lora_supported(GF.DT_CODE[d["dtype"]], M, N, K, bs, int(d["nested"]), d["r"]) if lib else 1
        assert sup == 1, d
        if lib:  # (family 7 exactly where the route answers "MFMA": the library's own logic on its 256-CU assumption)
            assert (lib.bnb_mi355x_gemm_4bit_route(0, GF.DT_CODE[d["dtype"]], M, N, K, bs) == 1) == (fam == GF.K_SM), d
        assert fam == (GF.K_STREAM if d["kind"] == "stream" else GF.K_SM), d
        fams[fam] += 1
        if d["kind"] == "stream":
            assert M == 1 or (2 <= M <= 4 and N < 128)
    assert 3 * fams[GF.K_STREAM] >= len(ds) and 3 * fams[GF.K_SM] >= len(ds), fams
    stream, sm = [d for d in ds if d["kind"] == "stream"], [d for d in ds if d["kind"] == "sm"]
    assert {d["N"] for d in stream} == set(GF.STREAM_N_GATED if section == "gated" else GF.STREAM_N)
    assert {d["K"] for d in stream} == set(GF.STREAM_K) and {d["K"] for d in sm} == set(GF.SM_K)
    assert {d["M"] for d in sm} == set(GF.SM_M) and {d["N"] for d in sm} == set(GF.SM_N)
    assert 1 in {d["M"] for d in stream} and {d["M"] for d in stream} & {2, 3, 4}
    assert {d["bs"] for d in ds} == {64, 128} and {d["dtype"] for d in ds} == {"bf16", "fp16"} and {d["qt"] for d in ds} == {"nf4", "fp4"}
    assert {d["bias"] for d in ds} == {True, False}
    for kind in (stream, sm):
        assert {d["dtype"] for d in kind} == {"bf16", "fp16"} and {d["qt"] for d in kind} == {"nf4", "fp4"}
    if section != "gated":
        assert {d["r"] for d in ds} == set(GF.RANKS) and {d["nested"] for d in ds} == {True, False}
    if section == "lora_ids":
        assert {d["A_n"] for d in ds} == set(GF.ADAPTERS) and {d["index_bytes"] for d in ds} == {4, 8}
        kinds = set()
        for d in ds:
            assert len(d["ids"]) == d["M"] and 1 <= d["A_n"] <= 64
            k = _id_kinds(d["ids"], d["A_n"])
            assert "other" not in k and (d["index_bytes"] == 8 or "alias" not in k)
            assert d["none"] == ("in" not in k)
            kinds |= k
            if lib:
                assert lib.bnb_mi355x_gemm_4bit_lora_ids_supported(GF.DT_CODE[d["dtype"]], d["M"], d["N"], d["K"], d["bs"], int(d["nested"]), d["r"], d["A_n"]) == 1
        assert kinds == {"in", "minus", "A_n", "alias"}
        none = [d for d in ds if d["none"]]
        assert 3 * len(none) >= len(ds) and {d["kind"] for d in none} == {"stream", "sm"}
        assert any(len(_id_kinds(d["ids"], d["A_n"])) >= 3 for d in ds)  # (a mix inside one batch)


@pytest.mark.parametrize("section", ("shrink", "shrink_ids"))
def test_shrink_draws_are_inside_the_preconditions_and_cover_the_lists(section):
    ds = _all(section)
    lib = _lib()
    for d in ds:
        M, K, R, splits = d["M"], d["K"], d["R"], d["splits"]
        assert d["dtype"] in ("bf16", "fp16") and 1 <= M <= 16 and K % 64 == 0 and R % 8 == 0 and 8 <= R <= 1024
        assert R != 1024 or K == 64
        if splits is not None:
            assert 1 <= len(splits) <= 8 and sum(splits) == R and all(s % 8 == 0 and 8 <= s <= 128 for s in splits)
        if lib and section == "shrink":
            assert lib.bnb_mi355x_lora_shrink_supported(GF.DT_CODE[d["dtype"]], M, R, K) == 1, d
        if lib and section == "shrink_ids":
            assert lib.bnb_mi355x_lora_shrink_ids_supported(GF.DT_CODE[d["dtype"]], M, d["A_n"], R, K) == 1, d
    assert {d["M"] for d in ds} == set(GF.SHRINK_M) and {d["K"] for d in ds} == set(GF.SHRINK_K) and {d["R"] for d in ds} == set(GF.SHRINK_R)
    tables = {d["splits"] for d in ds}
    assert None in tables and (8, 128) in tables and any(t is not None and set(t) == {8} for t in tables)
    assert any(t is not None and len(t) == 8 for t in tables)  # (the 8-part maximum)
    if section == "shrink_ids":
        assert {d["A_n"] for d in ds} == set(GF.ADAPTERS) and {d["index_bytes"] for d in ds} == {4, 8}
        kinds = set()
        for d in ds:
            k = _id_kinds(d["ids"], d["A_n"])
            assert len(d["ids"]) == d["M"] and "other" not in k and d["none"] == ("in" not in k)
            kinds |= k
        assert kinds == {"in", "minus", "A_n", "alias"} and sum(d["none"] for d in ds) >= 1


@pytest.mark.parametrize("section", ("experts", "experts_ffn"))
def test_experts_draws_are_inside_the_preconditions_and_cover_the_lists(section):
    ds = _all(section)
    lib = _lib()
    masked_pairs = 0
    for d in ds:
        E, N, K, bs, P = d["E"], d["N"], d["K"], d["bs"], d["P"]
        assert (E, N, K, bs) in GF.EXPERT_SHAPES and K % bs == 0 and bs >= 32 and P in EC.TS_OF_P and d["pattern"] in EC.ID_PATTERNS
        T, S = EC.TS_OF_P[P]
        assert T * S == P
        gated = {"chunked": 1, "interleaved": 2}.get(d["mode"], 0)
        assert not gated or N % 2 == 0
        assert (d["mode"] == "plain") == (section == "experts")
        ids = GF.expert_ids(d)
        assert ids.shape == (P,) and torch.equal(ids, GF.expert_ids(d))
        if d["pattern"] == "masked":
            masked_pairs += int(((ids < 0) | (ids >= E)).sum())
        else:
            assert bool(((ids >= 0) & (ids < E)).all())
        if lib:
            c = GF.DT_CODE[d["dtype"]]
            assert lib.bnb_mi355x_gemm_4bit_experts_supported(c, E, N, K, bs) == 1
            assert lib.bnb_mi355x_gemm_4bit_experts_ffn_supported(c, E, N, K, bs, gated) == 1
    assert {(d["E"], d["N"], d["K"], d["bs"]) for d in ds} == set(GF.EXPERT_SHAPES) and {d["P"] for d in ds} == set(GF.EXPERT_P)
    assert {d["dtype"] for d in ds} == {"bf16", "fp16", "fp32"} and {d["nested"] for d in ds} == {True, False}
    assert {d["shared_rows"] for d in ds} == {True, False} and {d["index_bytes"] for d in ds} == {4, 8}
    assert 3 * sum(d["pattern"] == "masked" for d in ds) >= len(ds) and masked_pairs >= 8
    assert {d["pattern"] for d in ds} == set(EC.ID_PATTERNS)
    if section == "experts_ffn":
        assert {d["mode"] for d in ds} == set(GF.FFN_MODES)
        assert any(d["pattern"] == "masked" and d["mode"].startswith("scale") for d in ds)  # (a NaN scale on a masked pair)
        assert any(d["pattern"] == "masked" and not d["mode"].startswith("scale") for d in ds)


def test_grouped_and_rows_draws_are_inside_the_preconditions_and_cover_the_lists():
    ds = _all("grouped")
    lib = _lib()
    routes = set()
    for d in ds:
        assert d["count"] == len(d["Ns"]) == len(d["bias"]) and d["count"] in GF.GROUP_COUNT and d["K"] % d["bs"] == 0 and d["M"] >= 1
        assert set(d["Ns"]) <= set(GF.GROUP_N)
        if lib:
            import ctypes as ct

            routes.add(lib.bnb_mi355x_gemm_4bit_grouped_route(GF.DT_CODE[d["dtype"]], d["count"], (ct.c_int * d["count"])(*d["Ns"]), d["M"], d["K"], d["bs"]))
    assert {d["count"] for d in ds} == set(GF.GROUP_COUNT) and {d["M"] for d in ds} == set(GF.GROUP_M) and {d["K"] for d in ds} == set(GF.GROUP_K)
    assert {n for d in ds for n in d["Ns"]} == set(GF.GROUP_N) and {d["nested"] for d in ds} == {True, False}
    if lib:
        assert routes <= {0, 1, 2} and len(routes) >= 2, routes
    ds = _all("rows")
    for d in ds:
        assert d["dim"] % 8 == 0 and d["dim"] % d["bs"] == 0 and d["bs"] in GF.ROWS_BS
        idx = GF.rows_indices(d)
        assert len(idx) == d["count"] and all(0 <= i < d["num_rows"] for i in idx) and idx[-1] == d["num_rows"] - 1
        assert d["count"] < 5 or len(set(idx)) < len(idx)  # (repeated indices)
    assert {d["dim"] for d in ds} == set(GF.ROWS_DIM) and {d["bs"] for d in ds} == set(GF.ROWS_BS) and {d["count"] for d in ds} == set(GF.ROWS_COUNT)
    assert {d["dtype"] for d in ds} == {"fp16", "bf16", "fp32"} and {d["index_bytes"] for d in ds} == {4, 8}
    assert all(72 % bs for bs in GF.ROWS_BS)  # (why a row length of 72 is not among the draws: no listed blocksize divides it)


def test_legacy_draws_name_every_entry_point_of_the_reference_abi_that_guard_stress_leaves():
    ds = _all("legacy")
    names = set()
    for d in ds:
        assert d["kind"] in GF.LEGACY_KINDS and d["bs"] in (32, 64, 128, 256, 512, 1024, 2048, 4096)
        if d["kind"] == "quant4":
            names.add(f"cquantize_blockwise_{d['dtype']}_{d['qt']}")
            assert d["n"] >= 1
        elif d["kind"] == "quant8":
            names.add(f"cquantize_blockwise_{d['dtype']}")
        else:
            names.add(("cgemm_4bit_" if d["kind"] == "gemm" else "cgemm_4bit_inference_naive_") + d["dtype"])
            assert d["K"] % d["bs"] == 0 and d["M"] >= 1 and (d["kind"] == "gemm" or (d["M"] == 1 and not d["nested"] and not d["bias"]))
    assert len(names) == 15, sorted(names)
    assert {d["nested"] for d in ds if d["kind"] == "gemm"} == {True, False}


def test_python_guard_shapes_are_one_of_each_family():
    (s, m) = GF.draws("python_guards", DRAWS, SEED)
    assert GF.predicted_family(s["M"], s["N"], s["K"]) == GF.K_STREAM and GF.predicted_family(m["M"], m["N"], m["K"]) == GF.K_SM
    assert s["N"] in GF.STREAM_N and s["K"] in GF.STREAM_K and m["M"] in GF.SM_M and m["N"] in GF.SM_N and m["K"] in GF.SM_K
    lib = _lib()
    for d in (s, m):
        assert d["N"] % 2 == 0 and d["r"] in GF.RANKS
        if lib:
            assert lib.bnb_mi355x_gemm_4bit_lora_supported(GF.DT_CODE[d["dtype"]], d["M"], d["N"], d["K"], 64, 0, d["r"]) == 1
            assert lib.bnb_mi355x_gemm_4bit_gated_supported(GF.DT_CODE[d["dtype"]], d["M"], d["N"], d["K"], 64) == 1
            assert lib.bnb_mi355x_lora_shrink_supported(GF.DT_CODE[d["dtype"]], d["M"], 24, d["K"]) == 1


def test_sm_selected_is_the_librarys_rule():
    """guard_fused.sm_selected against the route query over a grid around the draws' shapes (256 CUs without a device)."""
    lib = _lib()
    assert lib, "libbitsandbytes_mi355x.so is not built"
    for M in range(1, 17):
        for N in (1, 7, 127, 128, 130, 1000, 2001, 3071, 3072, 4352):
            for K in (64, 128, 256, 320, 768, 2112, 2560, 2752, 4096):
                sup = lib.bnb_mi355x_gemm_4bit_lora_supported(2, M, N, K, 64, 0, 8)
                route = lib.bnb_mi355x_gemm_4bit_route(0, 2, M, N, K, 64)
                if GF.sm_selected(M, N, K):
                    assert (sup, route) == (1, 1), (M, N, K)
                else:
                    assert sup == 0 or route == 0, (M, N, K)


# ------------------------------------------------------------------------------------------ the ledger
# launching exports that run between guard bands in neither check, each with its reason
EXEMPT = {
    "bnb_mi355x_peer_allgather": "peer exchange: needs several ranks; tests/checks/peer_ranks.py",
    "bnb_mi355x_gemv_4bit_peer": "peer chain: needs several ranks; tests/checks/peer_ranks.py",
    "bnb_mi355x_peer_chain_read": "peer chain: needs several ranks; tests/checks/peer_ranks.py",
    "cget_managed_ptr": "takes no device pointer (an allocation)",
}


def _launching_exports():
    header = open(os.path.join(ROOT, "include", "bnb_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = []
    for m in re.finditer(r"^[\w\s\*]*?\b(\w+)\s*\(([^;{]*)\)\s*;", code, flags=re.M):
        name, args = m.group(1), m.group(2)
        if (name.startswith("bnb_mi355x_") and "bnb_stream_t" in args) or re.match(r"c[a-z]", name):
            names.append(name)
    return names


def _called_names(path, exports):
    """Exports that `path` calls: `lib.NAME(` literally, or getattr(lib, f"...{x}...") with the braces as wildcards."""
    src = open(path).read()
    called = set(re.findall(r"\blib\.(\w+)\(", src))
    for pat in re.findall(r"getattr\(lib, f\"([^\"]+)\"\)", src):
        rx = re.compile("^" + re.sub(r"\\\{[^}]*\\\}", r"[a-z0-9]+", re.escape(pat)) + "$")
        called |= {n for n in exports if rx.match(n)}
    return called


def test_every_launching_entry_point_runs_between_guard_bands_or_is_exempt():
    exports = _launching_exports()
    assert len(exports) == len(set(exports)) >= 40 and "bnb_mi355x_gemm_4bit_lora_ids" in exports and "cdequantize_blockwise_bf16_nf4" in exports
    assert "bnb_mi355x_gemm_4bit_route" not in exports and "bnb_mi355x_version" not in exports
    called = set()
    for name in ("guard_stress.py", "guard_fused.py"):
        called |= _called_names(os.path.join(ROOT, "tests", "checks", name), exports)
    for name in exports:
        assert (name in called) != (name in EXEMPT), f"{name}: " + ("covered AND exempt" if name in called else "launches work but runs in neither "
                                                                    "tests/checks/guard_stress.py nor guard_fused.py, and EXEMPT has no reason")
    assert set(EXEMPT) <= set(exports), sorted(set(EXEMPT) - set(exports))
    assert all(len(reason) > 10 and "\n" not in reason for reason in EXEMPT.values())
    fused = _called_names(os.path.join(ROOT, "tests", "checks", "guard_fused.py"), exports)
    assert fused >= {"bnb_mi355x_gemm_4bit_experts", "bnb_mi355x_gemm_4bit_experts_ffn", "bnb_mi355x_gemm_4bit_gated", "bnb_mi355x_gemm_4bit_lora",
                     "bnb_mi355x_gemm_4bit_lora_ids", "bnb_mi355x_lora_shrink", "bnb_mi355x_lora_shrink_ids", "bnb_mi355x_gemm_4bit_grouped",
                     "bnb_mi355x_dequantize_4bit_rows"}
