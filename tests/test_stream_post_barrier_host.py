"""CPU: the in-lane row sum of the M = 1 streaming gemv (csrc/gemv4_stream.hip), as far as a host can check it.

  * The row sum finished in the vector unit (wave_sum_n_lane63, csrc/bnb_common.h) adds in the association of wave_sum_n,
    (r0 + r1) + (r2 + r3) with commuted operands: a float32 replay of both spellings, lane by lane, gives the same bits - and a
    differently ordered sum does NOT on most inputs, so the GPU identity test (tests/test_gpu_stream_post_barrier.py) would see a
    wrong order.
  * ISA: no v_readlane_b32 is left in a one-row instance; the sweep twins still carry the form they are named after.
  * The host's exact-instance query follows the two new values of the `nt` knob."""
import numpy as np

N_SUMS = 4096
F32 = np.float32


def _row_steps(v):
    """The four DPP steps both spellings share, on [n, 64] float32: lane ^ 1, lane ^ 2, row_half_mirror, row_mirror."""
    lane = np.arange(64)
    for src in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        v = (v[:, src] + v).astype(F32)  # v_add_f32_dpp: src0 = the moved value
    return v


def _readlane_sum(v):
    v = _row_steps(v)
    r0, r1, r2, r3 = v[:, 0], v[:, 16], v[:, 32], v[:, 48]
    return ((r0 + r1).astype(F32) + (r2 + r3).astype(F32)).astype(F32)


def _lane63_sum(v):
    v = _row_steps(v).copy()
    lane = np.arange(64)
    row = lane >> 4
    on = (row == 1) | (row == 3)  # row_bcast:15, row mask 0xA: lane 15 of the row below into every lane of rows 1 and 3
    v[:, on] = (v[:, (row[on] - 1) * 16 + 15] + v[:, on]).astype(F32)
    on = row >= 2                 # row_bcast:31, row mask 0xC: lane 31 into every lane of rows 2 and 3
    v[:, on] = (v[:, np.full(on.sum(), 31)] + v[:, on]).astype(F32)
    return v[:, 63]


def _other_row_tree_sum(v):
    v = _row_steps(v)
    r0, r1, r2, r3 = v[:, 0], v[:, 16], v[:, 32], v[:, 48]
    return ((r0 + r2).astype(F32) + (r1 + r3).astype(F32)).astype(F32)


def _sequential_sum(v):
    acc = v[:, 0].copy()
    for lane in range(1, 64):
        acc = (acc + v[:, lane]).astype(F32)
    return acc


def test_both_spellings_of_the_row_sum_give_the_same_bits_and_another_tree_does_not():
    rng = np.random.RandomState(20260421)
    v = (rng.standard_normal((N_SUMS, 64)) * np.exp2(rng.randint(-3, 4, (N_SUMS, 64)))).astype(F32)
    a, b = _readlane_sum(v), _lane63_sum(v)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rows = _row_steps(v)
    for r in range(4):  # every lane of a row holds the row's sum after the shared steps: lane 15 / 31 serve as well as 0 / 16 / 32 / 48
        assert (rows[:, 16 * r:16 * r + 16].view(np.uint32) == rows[:, 16 * r:16 * r + 1].view(np.uint32)).all()
    # a wrong order shows: the lanes added one after the other change most sums (asserted: at least half, seed fixed); the four row
    # sums alone in another association, (r0 + r2) + (r1 + r3), change fewer - one rounding of three differs (printed, 38 %)
    changed = int((a.view(np.uint32) != _sequential_sum(v).view(np.uint32)).sum())
    rows_only = int((a.view(np.uint32) != _other_row_tree_sum(v).view(np.uint32)).sum())
    print(f"of {N_SUMS} sums: sequential order changes {changed}, (r0 + r2) + (r1 + r3) changes {rows_only}")
    assert 2 * changed >= N_SUMS, changed
    assert rows_only > N_SUMS // 4, rows_only


def test_exact_instance_query_follows_the_twin_knob_values():
    """nt = 4: the readlane twin of the instance the launch selects (4096 x 4096: the exact one); nt = 5: of the general instance."""
    from bitsandbytes_amd import cextension as ce

    assert ce.lib
    q = ce.lib.bnb_mi355x_gemv_4bit_stream_exact
    try:
        for nt, want in ((4, 1), (5, 0), (2, 0), (3, 0), (-1, 1)):
            ce.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, nt, 0)
            assert q(2, 1, 4096, 4096, 64, 0) == want, nt
    finally:
        ce.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)
    assert q(2, 1, 4096, 4096, 64, 0) == 1


def test_isa_no_readlane_in_one_row_instances_and_the_twins_are_what_they_say():
    """<T, MB, WAVES, NS, FLAGS>: every MB = 1 instance without kReadlaneSum (4096) carries the two row_bcast adds per item copy and
    - wherever the compiler spills no SGPR into VGPR lanes - no v_readlane_b32 at all; MB > 1 instances keep the readlane form. The three
    twins (bf16, 16 wavefronts: kNT general, kNT | kExact, kNT | kFp4 | kNested general) exist, with v_readlane_b32 and without row_bcast."""
    from test_stream_fixed_cost_isa import STREAM, _device_disassembly

    stream = _device_disassembly("gemv4_stream_kernel")
    K_NESTED, K_FP4, K_NT, K_EXACT, K_READLANE = 1, 4, 8, 128, 4096
    by_key, one_row = {}, 0
    for name, lines in stream.items():
        m = STREAM.search(name)
        assert m, name
        key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
        by_key[key] = lines
        ops = [ln.split()[0] for ln in lines]
        bcast = sum("row_bcast" in ln for ln in lines)
        if key[1] == 1 and not key[4] & K_READLANE:
            # (a few multi-phase and 8-wavefront instances spill SGPRs into VGPR lanes: the compiler's v_writelane_b32 / v_readlane_b32
            # pairs are not the reduction's - every single-phase 16-wavefront instance is free of both)
            assert bcast >= 2 and bcast % 2 == 0, (name, bcast)
            if ops.count("v_writelane_b32") == 0 or (key[2] == 16 and not key[4] & 32):
                one_row += 1
                assert ops.count("v_readlane_b32") == 0, (name, ops.count("v_readlane_b32"))
        else:
            assert bcast == 0 and ops.count("v_readlane_b32") >= 4, (name, bcast)
    assert one_row >= 60, one_row
    twins = sorted(k for k in by_key if k[4] & K_READLANE)
    assert twins == sorted(("DF16b", 1, 16, 2, fl | K_READLANE) for fl in (K_NT, K_NT | K_EXACT, K_NT | K_FP4 | K_NESTED)), twins
