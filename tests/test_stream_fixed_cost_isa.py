"""CPU: the fixed cost of the M = 1 streaming gemv, read from the ISA of the built library (no GPU needed).

Two properties of csrc/gemv4_stream.hip and csrc/gemm4_mfma_sm.hip that no test of values can see:
  * no kernarg load behind the last barrier. The epilogue's out / bias pointers live beyond the preloaded dwords; loaded where they
    are used, their cold miss sits on the tail of the kernel, where every other wavefront has ended and nothing hides it;
  * the exact-geometry instance of the streaming kernel reaches its first weight request in at most half the instructions of
    the general instance - on the path of wavefronts 8 - 15 (no activation copy) and on the path of the builder wavefronts 0 - 7.
And one of the host: which shapes select the exact instance."""
import re

import pytest

STREAM = re.compile(r"stream_kernelI(\w+?)Li(\d)ELi(\d+)ELi(\d)ELi(\d+)E")  # <T, MB, WAVES, NS, FLAGS>
K_NESTED, K_FP4, K_NT, K_GROUPED, K_MULTI, K_PEER, K_EXACT, K_LATE = 1, 4, 8, 16, 32, 64, 128, 256


def _device_disassembly(symbol_substring: str):
    """{kernel symbol: [instruction lines]} for the kernels of the library's gfx950 code objects whose name contains
    `symbol_substring` (llvm-objdump; the helper of tests/test_cabi.py)."""
    import subprocess
    import tempfile
    from pathlib import Path

    llvm = Path("/opt/rocm/lib/llvm/bin")
    tools = [llvm / "llvm-objcopy", llvm / "clang-offload-bundler", llvm / "llvm-objdump"]
    if not all(t.exists() for t in tools):
        pytest.skip("ROCm LLVM binutils not available")
    from bitsandbytes_amd.cextension import LIB_PATH

    kernels = {}
    with tempfile.TemporaryDirectory() as td:
        fat = Path(td) / "fat.bin"
        subprocess.check_call([str(tools[0]), "-O", "binary", "--only-section=.hip_fatbin", str(LIB_PATH), str(fat)])
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
        for i, s0 in enumerate(starts):
            piece = Path(td) / f"bundle{i}.bin"
            piece.write_bytes(blob[s0 : starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = Path(td) / f"dev{i}.co"
            subprocess.check_call([str(tools[1]), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--input={piece}", f"--output={co}"], stderr=subprocess.DEVNULL)
            syms = subprocess.run([str(tools[2]), "-t", str(co)], capture_output=True, text=True).stdout
            if symbol_substring not in syms:
                continue
            text = subprocess.run([str(tools[2]), "-d", "--no-show-raw-insn", str(co)], capture_output=True, text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = m.group(1) if symbol_substring in m.group(1) and not m.group(1).endswith(".kd") else None
                    if cur:
                        kernels[cur] = []
                elif cur and line.strip():
                    kernels[cur].append(line.strip())
    return kernels


def _scalar_loads_behind_last_barrier(lines):
    """s_load_dword* instructions from the KERNARG segment behind the last s_barrier of the kernel's text. The kernarg pointer
    arrives in s[0:1]; in text order, a register pair holds it from the entry (or from an s_mov_b64 copy of a pair that holds it) until
    an instruction writes one of its registers. Scalar loads through other pointers (the nested statistics' second-level absmax, read per
    item through the matrix's own pointer) are data, not arguments."""
    ops = [ln.split()[0] for ln in lines]
    last = max(i for i, op in enumerate(ops) if op == "s_barrier")
    holds = {(0, 1)}  # register pairs that hold the kernarg pointer at this point of the text
    found = []
    for i, ln in enumerate(lines):
        text = ln.split("//")[0].strip()
        args = [a.strip() for a in text[len(ops[i]):].split(",")]
        if ops[i].startswith("s_load_dword"):
            m = re.fullmatch(r"s\[(\d+):(\d+)\]", args[1])
            if i > last and m and (int(m.group(1)), int(m.group(2))) in holds:
                found.append(text)
        copy = re.fullmatch(r"s_mov_b64 s\[(\d+):(\d+)\], s\[(\d+):(\d+)\]", text)
        copied = copy is not None and (int(copy.group(3)), int(copy.group(4))) in holds
        # the destination of an instruction is its first operand (VALU compares and v_readfirstlane write SGPRs too): that register (pair, range) no longer holds the pointer
        if not ops[i].startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_waitcnt")) and args and args[0]:
            m = re.fullmatch(r"s(\d+)|s\[(\d+):(\d+)\]", args[0])
            if m:
                lo, hi = (int(m.group(1)),) * 2 if m.group(1) else (int(m.group(2)), int(m.group(3)))
                holds = {h for h in holds if h[1] < lo or h[0] > hi}
        if copied:
            holds.add((int(copy.group(1)), int(copy.group(2))))
    return found


def test_no_kernarg_load_behind_the_last_barrier():
    """Every single-matrix, non-peer instance of gemv4_stream_kernel and EVERY instance of gemm4_mfma_sm_kernel: no s_load_dword*
    behind the last s_barrier. Deliberately left:
      * grouped stream instances (FLAGS & 16): out / bias / N belong to the matrix of each ROW (mat[mi], mi found per row in the
        epilogue) - there is no one pointer to request early;
      * peer-chain stream instances (FLAGS & 64): their epilogue reads the exchange's descriptors (ranks' buffers, mode, epoch
        offset), a different and larger set - not part of this change;
      * the two sweep-only kLateArgs instances (FLAGS & 256): they ARE the old form, kept so that tools/stream_fixed_cost_ab.py can
        measure the lever in one process - asserted below to still show the late load (the A/B compares what it claims to).
    gemm4_mfma_rt_kernel and gemm4_experts_kernel never had such a load (checked here so that it stays so)."""
    stream = _device_disassembly("gemv4_stream_kernel")
    assert len(stream) >= 150, len(stream)
    checked = late = 0
    for name, lines in stream.items():
        m = STREAM.search(name)
        assert m, name
        flags = int(m.group(5))
        if flags & (K_GROUPED | K_PEER):
            continue
        behind = _scalar_loads_behind_last_barrier(lines)
        if flags & K_LATE:
            late += 1
            assert behind, f"{name}: the kLateArgs instance no longer loads its epilogue pointers late - the A/B has no 'off' side"
            continue
        checked += 1
        assert not behind, f"{name}: kernarg load(s) behind the last barrier: {behind}"
    assert checked >= 80 and late == 2, (checked, late)
    for family, least in (("gemm4_mfma_sm_kernel", 40), ("gemm4_mfma_rt_kernel", 28), ("gemm4_experts_kernel", 4)):
        kernels = _device_disassembly(family)
        assert len(kernels) >= least, (family, len(kernels))
        for name, lines in kernels.items():
            if "s_barrier" not in [ln.split()[0] for ln in lines]:
                continue
            behind = _scalar_loads_behind_last_barrier(lines)
            assert not behind, f"{name}: kernarg load(s) behind the last barrier: {behind}"


def _path_lengths(lines):
    """Instructions executed from the kernel's post-preload entry up to (not including) its first weight request
    (buffer_load_dwordx4), on two paths: (wavefronts 8 - 15, builder wavefronts 0 - 7).

    A kernel with preloaded arguments starts with a 256-byte compatibility header (the loads of the preloaded dwords, a wait, a
    branch over s_nop padding) that the hardware skips when the firmware preloads: the entry is the header branch's target. The
    builder path falls through every conditional branch in front of the first request (one trip of the activation-copy loop, no early
    exit). The path of wavefronts 8 - 15 differs in ONE place: it takes the forward branch around the activation copy - the only
    conditional branch whose target still lies in front of the first request."""
    lines = [ln for ln in lines if "//" in ln]  # (llvm-objdump elides runs of zero padding as "...")
    addr = []
    for ln in lines:
        m = re.search(r"//\s*([0-9A-Fa-f]+):", ln)
        assert m, ln
        addr.append(int(m.group(1), 16))
    ops = [ln.split()[0] for ln in lines]

    def target(i):
        m = re.search(r"<[^>]*\+0x([0-9a-f]+)>", lines[i])
        assert m, lines[i]
        return addr[0] + int(m.group(1), 16)

    assert ops[0].startswith("s_load_dword"), "expected the kernarg-preload header"
    header_branch = ops.index("s_branch")
    entry = addr.index(target(header_branch))
    first_request = next(i for i, op in enumerate(ops) if op == "buffer_load_dwordx4")
    assert entry < first_request
    builder = first_request - entry
    late, i, taken = 0, entry, 0
    while i < first_request:
        late += 1
        if ops[i].startswith("s_cbranch") and addr[i] < target(i) <= addr[first_request]:
            i = addr.index(target(i))
            taken += 1
        else:
            i += 1
    assert taken == 1, f"expected one branch around the activation copy, found {taken}"
    return late, builder


def test_exact_instance_reaches_its_first_weight_request_in_half_the_instructions():
    """The headline instance <bf16, 1, 16, 2, kNT | kExact> against the general <bf16, 1, 16, 2, kNT> of the same library (the
    parent's prologue): both paths at most half as long. Every exact instance (bf16 / f16 x NF4 / FP4, fp32 absmax) exists; the
    nested-statistics ones were measured behind the general instance and are not built."""
    stream = _device_disassembly("gemv4_stream_kernel")
    by_key = {}
    for name in stream:
        m = STREAM.search(name)
        by_key[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))] = name
    for t in ("DF16b", "DF16_"):
        for fl in (0, K_FP4):
            assert (t, 1, 16, 2, K_NT | K_EXACT | fl) in by_key, (t, fl)
            assert (t, 1, 16, 2, K_NT | fl) in by_key, (t, fl)
        for fl in (K_NESTED, K_FP4 | K_NESTED):
            assert (t, 1, 16, 2, K_NT | K_EXACT | fl) not in by_key and (t, 1, 16, 2, K_NT | fl) in by_key, (t, fl)
    exact = _path_lengths(stream[by_key[("DF16b", 1, 16, 2, K_NT | K_EXACT)]])
    general = _path_lengths(stream[by_key[("DF16b", 1, 16, 2, K_NT)]])
    print(f"instructions in front of the first weight request (wavefronts 8-15, builders): exact {exact}, general {general}")
    assert 2 * exact[0] <= general[0], (exact, general)
    assert 2 * exact[1] <= general[1], (exact, general)


def test_host_selects_the_exact_instance_only_for_exact_geometries():
    """bnb_mi355x_gemv_4bit_stream_exact runs the launcher's geometry and rule on the host (256 CUs assumed without a device, the
    MI355X's count): 4096 x 4096 (16 rows per workgroup) and 14336 x 4096 (56) are exact; 11008 x 4096 (43 rows: not a multiple of
    the 8 row groups), 1376 x 4096 (6 rows: fewer than a ring per row group), K = 11008 (not 2 x 2048), any K % 2048 != 0, fp32
    activations, nested statistics and M > 1 are not. The tuning knob's value 2 forces the general instance."""
    from bitsandbytes_amd import cextension as ce

    assert ce.lib
    q = ce.lib.bnb_mi355x_gemv_4bit_stream_exact
    BF16, F16, F32 = 2, 1, 0
    for dt in (BF16, F16):
        for bs in (64, 128):
            assert q(dt, 1, 4096, 4096, bs, 0) == 1
            assert q(dt, 1, 14336, 4096, bs, 0) == 1
            assert q(dt, 1, 4096, 4096, bs, 1) == 0
            for N, K in ((11008, 4096), (1376, 4096), (4096, 11008), (512, 11008), (4096, 4096 + 64), (4096, 2048 + 32), (4096, 8192),
                         (4096, 2048), (4096 + 8, 4096)):
                assert q(dt, 1, N, K, bs, 0) == 0, (N, K)
    assert q(F32, 1, 4096, 4096, 64, 0) == 0 and q(BF16, 2, 4096, 4096, 64, 0) == 0
    try:
        ce.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, 2, 0)
        assert q(BF16, 1, 4096, 4096, 64, 0) == 0
    finally:
        ce.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, -1, 0)
    assert q(BF16, 1, 4096, 4096, 64, 0) == 1
