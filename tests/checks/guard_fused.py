#!/usr/bin/env python3
"""Guard bands and placement sweep for the fused decode entry points of the C ABI - gemm_4bit_gated, gemm_4bit_lora,
gemm_4bit_lora_ids, lora_shrink, lora_shrink_ids, gemm_4bit_experts, gemm_4bit_experts_ffn, gemm_4bit_grouped and
dequantize_4bit_rows, the names of the reference ABI that tests/checks/guard_stress.py does not call (section `legacy`: the
NULL-stream quantize, cgemm_4bit_<T>, the legacy gemv; guard_stress.py has the rest of the base path) - and the misaligned-view sweep
of the Python layer in front of the fused ops (section `python_guards`: no C ABI, no bands).

Per draw (``draws(section, n, seed)``: a pure generator, no device and no library), through ``bnb.lib``:
  1. the matching ``_supported`` predicate answers 1 (a 0 is a failure, not a skip);
  2. the WANT: the entry point on fresh, aligned, stand-alone tensors; the kernel family of both calls is the same;
  3. the CARVED call (tests/guard_bands.py): every 16-byte operand at an odd multiple of 16 (or a random one), every other operand
     at exactly its element's alignment, absmax at exactly 4 bytes, ids at exactly index_bytes; inputs between bands of 0xFF (NaN /
     id -1), outputs between bands of 0xA5 that reach as far as the output would at the entry point's largest row count; ``splits``
     and the grouped call's pointer arrays are host arrays;
  4. the bands of every output are untouched;
  5. the output bytes equal the want's, bit for bit (the legacy matmuls: see Legacy.bit_exact);
  6. the want agrees with a plain high-precision reference of the operation (the tolerances the project already has: each section's
     ``ref``).
Values are random normal data. One line per failure, a summary line per section.
    python tests/checks/guard_fused.py [--draws 24] [--seed 11] [--only SECTION]"""
import argparse
import ctypes as ct
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import guard_bands as GB  # noqa: E402

SECTIONS = ("gated", "lora", "lora_ids", "shrink", "shrink_ids", "experts", "experts_ffn", "grouped", "rows", "legacy", "python_guards")
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
DT_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}
QT_CODE = {"fp4": 1, "nf4": 2}
IDX = {4: torch.int32, 8: torch.int64}
K_STREAM, K_SM = 1, 7
CUS = 256  # (the CU count the generator's family prediction assumes: an MI355X, and the library's default without a device)

# ---------------------------------------------------------------------------------------------- shapes (the issue's lists)
STREAM_N, STREAM_N_GATED, STREAM_K = (1, 2, 7, 130, 2001), (2, 6, 130, 2002), (64, 128, 768, 2112)
SM_M, SM_N, SM_K = (2, 3, 5, 8, 15, 16), (128, 130, 1000, 4352), (64, 256, 320, 2752)
RANKS = (8, 24, 128)
ADAPTERS = (1, 3, 64)
ALIAS = 2 ** 32 + 1
SHRINK_M, SHRINK_K, SHRINK_R = (1, 2, 3, 7, 8, 9, 16), (64, 128, 2752, 4096), (8, 24, 136, 1024)
EXPERT_SHAPES = ((4, 96, 96, 32), (5, 130, 768, 64), (5, 144, 768, 64), (8, 512, 1024, 128))
EXPERT_P = (1, 2, 5, 16, 65)
EXPERT_PATTERNS = ("one", "distinct", "ends", "random")  # and "masked" in every third draw
FFN_MODES = ("chunked", "interleaved", "scale_fp32", "scale_T")
GROUP_COUNT, GROUP_N, GROUP_M, GROUP_K = (2, 3, 8), (1, 7, 130, 1000, 3200), (1, 2, 4, 8, 16, 17, 33), (64, 256, 2048)
# (the issue also lists dim 72: no listed blocksize divides it, so it is outside the entry point's preconditions - a refused launch;
# 96 takes its place as the row length that is a multiple of the smallest blocksize only)
ROWS_DIM, ROWS_BS, ROWS_COUNT = (64, 96, 192, 2560), (32, 64, 128), (1, 5, 1000)
ROWS_TABLE = 37
# the reference ABI's names that guard_stress.py does not call (NULL-stream quantize, cgemm_4bit_<T>, the legacy gemv): four kinds in turn
LEGACY_KINDS = ("quant4", "quant8", "gemm", "naive")
LEGACY_N = (1, 63, 1000, 4097, 64 * 255 + 7, 70000)
# the Python-layer sweep: one stream-kernel shape and one streaming-MFMA shape (M, N, K, r) from the lists above
GUARD_SHAPES = ((1, 130, 768, 8), (3, 1000, 320, 24))


def sm_selected(M, N, K, cus=CUS):
    """csrc/gemm4_mfma.hip: sm_selected without tuning knobs - which 16-bit problems the built-in route gives the streaming MFMA
    kernel (tests/test_guard_bands_host.py holds it against bnb_mi355x_gemm_4bit_lora_supported / _route for every draw)."""
    if M < 2 or N < 128 or K % 64:
        return False
    if K % 256:
        return M <= 128
    if N >= 12 * cus:
        return M <= 16 and not (M > 8 and K > 2 * N)
    if M == 2:
        return K <= 5120
    if M <= 4:
        return True
    if M <= 8:
        return K >= 2560 and (N >= 1024 or K <= 4096)
    return M <= 16 and (K <= 4096 or K <= 2 * N)


def predicted_family(M, N, K):
    """The kernel family of a decode draw: the streaming MFMA kernel where sm_selected, else the streaming kernel (the draws stay
    below the sizes at which the other MFMA kernels take over: M <= 4 and N K < 12 M off the streaming MFMA kernel's reach)."""
    return K_SM if sm_selected(M, N, K) else K_STREAM


def _cycle(values, n, rng):
    out = []
    while len(out) < n:
        part = list(values)
        rng.shuffle(part)
        out += part
    return out[:n]


def _ids(M, A_n, idx64, none, rng):
    bad = [-1, A_n] + ([ALIAS] if idx64 else [])
    if none:
        shift = rng.randrange(len(bad))
        return [bad[(k + shift) % len(bad)] for k in range(M)]
    ids = [rng.choice(bad) if rng.random() < 0.35 else rng.randrange(A_n) for _ in range(M)]
    ids[rng.randrange(M)] = rng.randrange(A_n)  # (at least one row with an adapter)
    return ids


def _split_tables(R):
    """The split tables of the issue for this R: None, (8,) * k and an (8, 128, ...) table, where they exist (parts in [8, 128])."""
    out = [None]
    if R // 8 <= 8:
        out.append((8,) * (R // 8))
    if R == 136:
        out.append((8, 128))
    if R == 1024:
        out.append((128,) * 8)  # (the 8-part maximum)
    return out


def _decode_draws(section, n, rng):
    gated = section == "gated"
    ns, nm = (n + 1) // 2, n // 2
    sN, sK = _cycle(STREAM_N_GATED if gated else STREAM_N, ns, rng), _cycle(STREAM_K, ns, rng)
    mM, mN, mK = _cycle(SM_M, nm, rng), _cycle(SM_N, nm, rng), _cycle(SM_K, nm, rng)
    ranks, adapters = _cycle(RANKS, n, rng), _cycle(ADAPTERS, n, rng)
    for i in range(n):
        j = i // 2
        if i % 2 == 0:
            N, K = sN[j], sK[j]
            M = rng.choice((2, 3, 4)) if N < 128 and j % 2 else 1  # (2 ... 4 rows stay on the streaming kernel below 128 rows)
        else:
            M, N, K = mM[j], mN[j], mK[j]
            if not sm_selected(M, N, K):  # (5 ... 8 rows on K = 256 below 3072 rows run the register-transposed kernel: no epilogue)
                N = 4352
        d = dict(section=section, i=i, kind="stream" if i % 2 == 0 else "sm", M=M, N=N, K=K,
                 bs=128 if K % 128 == 0 and rng.random() < 0.5 else 64, dtype=("bf16", "fp16")[(i // 2 + i) % 2], qt=("nf4", "fp4")[(i // 3) % 2],
                 bias=rng.random() < 0.5, nested=False, seed=rng.randrange(1 << 30))
        if not gated:
            d.update(nested=rng.random() < 0.5, r=ranks[i], scaling=rng.choice((0.25, 0.5, 2.0)))
        if section == "lora_ids":
            A_n, ib = adapters[i], (4, 8)[(i // 2) % 2]
            none = i % 3 == 0
            if A_n * N * d["r"] > 1 << 24:
                d["r"] = 8
            d.update(A_n=A_n, index_bytes=ib, none=none, ids=_ids(M, A_n, ib == 8, none, rng))
        yield d


def _shrink_draws(section, n, rng):
    ms, ks, rs, adapters = _cycle(SHRINK_M, n, rng), _cycle(SHRINK_K, n, rng), _cycle(SHRINK_R, n, rng), _cycle(ADAPTERS, n, rng)
    used = {}
    for i in range(n):
        M, K, R = ms[i], ks[i], rs[i]
        if R == 1024:
            K = 64
        tables = _split_tables(R)
        splits = tables[used.get(R, 0) % len(tables)]
        used[R] = used.get(R, 0) + 1
        d = dict(section=section, i=i, M=M, K=K, R=R, splits=splits, dtype=("bf16", "fp16")[i % 2], seed=rng.randrange(1 << 30))
        if section == "shrink_ids":
            A_n, ib = adapters[i], (4, 8)[(i // 2) % 2]
            if A_n * R * K > 1 << 24:
                A_n = 3
            none = i == 5
            d.update(A_n=A_n, index_bytes=ib, none=none, ids=_ids(M, A_n, ib == 8, none, rng))
        yield d


def _experts_draws(section, n, rng):
    shapes, ps, pats, modes = _cycle(EXPERT_SHAPES, n, rng), _cycle(EXPERT_P, n, rng), _cycle(EXPERT_PATTERNS, n, rng), _cycle(FFN_MODES, n, rng)
    for i in range(n):
        E, N, K, bs = shapes[i]
        d = dict(section=section, i=i, E=E, N=N, K=K, bs=bs, P=ps[i], dtype=("bf16", "fp16", "fp32")[i % 3], qt=("nf4", "fp4")[(i // 2) % 2],
                 nested=(i // 3) % 2 == 1, bias=rng.random() < 0.5, shared_rows=rng.random() < 0.5, index_bytes=(4, 8)[(i // 2) % 2],
                 pattern="masked" if i % 3 == 0 else pats[i], mode="plain", seed=rng.randrange(1 << 30))
        if section == "experts_ffn":
            d["mode"] = modes[i]
        yield d


def _grouped_draws(section, n, rng):
    counts, ms, ks = _cycle(GROUP_COUNT, n, rng), _cycle(GROUP_M, n, rng), _cycle(GROUP_K, n, rng)
    ns = _cycle(GROUP_N, sum(counts), rng)
    for i in range(n):
        Ns, ns = tuple(ns[:counts[i]]), ns[counts[i]:]
        K = ks[i]
        yield dict(section=section, i=i, count=counts[i], Ns=Ns, M=ms[i], K=K, bs=128 if K % 128 == 0 and rng.random() < 0.5 else 64,
                   dtype=("bf16", "fp16")[i % 2], qt=("nf4", "fp4")[(i // 2) % 2], nested=(i // 3) % 2 == 1,
                   bias=tuple(rng.random() < 0.5 for _ in Ns), seed=rng.randrange(1 << 30))


def _rows_draws(section, n, rng):
    dims, counts = _cycle(ROWS_DIM, n, rng), _cycle(ROWS_COUNT, n, rng)
    for i in range(n):
        dim = dims[i]
        bss = [b for b in ROWS_BS if dim % b == 0]
        yield dict(section=section, i=i, dim=dim, bs=bss[(i // len(ROWS_DIM)) % len(bss)], count=counts[i], num_rows=ROWS_TABLE,
                   dtype=("fp16", "bf16", "fp32")[i % 3], qt=("nf4", "fp4")[(i // 2) % 2], index_bytes=(4, 8)[(i // 3) % 2],
                   seed=rng.randrange(1 << 30))


def _legacy_draws(section, n, rng):
    for i in range(n):
        kind, j = LEGACY_KINDS[i % 4], i // 4
        d = dict(section=section, i=i, kind=kind, dtype=("bf16", "fp16", "fp32")[j % 3], qt=("nf4", "fp4")[(j // 3) % 2], seed=rng.randrange(1 << 30))
        if kind == "quant4":
            d.update(n=LEGACY_N[j % 6], bs=(32, 64, 4096)[(j + 1) % 3])
        elif kind == "quant8":
            d.update(n=LEGACY_N[(j + 2) % 6], bs=(256, 4096, 64)[(j + 1) % 3])
        elif kind == "gemm":
            d.update(M=(1, 3, 17)[(j + 1) % 3], N=(7, 130)[j % 2], K=(64, 256, 768)[(j + 2) % 3], bs=64, nested=j % 2 == 1, bias=rng.random() < 0.5)
        else:
            d.update(M=1, N=(7, 130, 2001)[(j + 1) % 3], K=(64, 768)[j % 2], bs=64, nested=False, bias=False)
        yield d


def draws(section, n, seed):
    """The draws of a section as plain dicts (ints, strings, tuples): a function of (section, n, seed) alone."""
    rng = random.Random(f"{section}/{seed}")
    if section in ("gated", "lora", "lora_ids"):
        return list(_decode_draws(section, n, rng))
    if section in ("shrink", "shrink_ids"):
        return list(_shrink_draws(section, n, rng))
    if section in ("experts", "experts_ffn"):
        return list(_experts_draws(section, n, rng))
    if section == "grouped":
        return list(_grouped_draws(section, n, rng))
    if section == "rows":
        return list(_rows_draws(section, n, rng))
    if section == "legacy":
        return list(_legacy_draws(section, n, rng))
    if section == "python_guards":
        return [dict(section=section, i=i, M=M, N=N, K=K, r=r, dtype=("bf16", "fp16")[i % 2]) for i, (M, N, K, r) in enumerate(GUARD_SHAPES)]
    raise ValueError(section)


def rows_indices(d):
    """The index list of a `rows` draw: repeats, and the table's last row."""
    rng = random.Random(d["seed"])
    idx = [rng.randrange(d["num_rows"]) for _ in range(d["count"])]
    idx[-1] = d["num_rows"] - 1
    if d["count"] >= 5:
        idx[1] = idx[0]
    return idx


def expert_ids(d):
    """[P] int64 expert ids (CPU) of an experts draw: tests/experts_cases.py's patterns."""
    import experts_cases as EC

    return EC.make_ids(d["pattern"], d["P"], d["E"], torch.Generator().manual_seed(d["seed"]))


# ---------------------------------------------------------------------------------------------- placement
DEV = "cuda"


class Fresh:
    """The want: every operand a freshly allocated, 256-byte aligned tensor of its own (an output's allocation carries the same
    bands as the carved call's, and they are checked as well: a store outside the output stays inside memory the check owns)."""
    carved = False

    def __init__(self, rng=None):
        self.rng, self.keep, self.outs = rng, [], []

    def a16(self, t):
        return self.elt(t)

    def elt(self, t, align=None):
        if t is None:
            return None
        self.keep.append(t.contiguous().clone())
        return self.keep[-1].data_ptr()

    def out(self, nbytes, largest, align=16):
        self.outs.append(GB.Carved(nbytes, 0, device=DEV, after=GB.after_band(largest)))
        return self.outs[-1].ptr()

    def ok(self):
        return all(c.guards_ok() for c in self.outs)

    def result(self, i=0):
        return self.outs[i].bytes()


class Placed(Fresh):
    """The carved call: 16-byte operands at place(16), the others at exactly their element's alignment; 0xFF around inputs, 0xA5
    around outputs, as far behind as the output reaches at the entry point's largest row count."""
    carved = True

    def a16(self, t):
        if t is None:
            return None
        self.keep.append(GB.carve_in(t, None, device=DEV, fill=GB.NAN_PAT, off=GB.place(16, self.rng)))
        return self.keep[-1].ptr()

    def elt(self, t, align=None):
        if t is None:
            return None
        self.keep.append(GB.carve_in(t, None, device=DEV, fill=GB.NAN_PAT, off=GB.offset_for(align or t.element_size(), self.rng)))
        return self.keep[-1].ptr()

    def out(self, nbytes, largest, align=16):
        off = GB.place(16, self.rng) if align == 16 else GB.offset_for(align, self.rng)
        self.outs.append(GB.carve_out(nbytes, None, align, device=DEV, after=GB.after_band(largest), off=off))
        return self.outs[-1].ptr()



def _stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _quant(W, bs, qt, nested):
    """(packed, (absmax fp32, absmax_8bit, absmax_code, absmax_offset), QuantState)"""
    import bitsandbytes_amd.functional as F

    q, st = F.quantize_4bit(W, blocksize=bs, quant_type=qt, compress_statistics=nested)
    if nested:
        return q.view(-1), (st.state2.absmax, st.absmax, st.state2.code.float().contiguous(), st.offset.float().reshape(1)), st
    return q.view(-1), (st.absmax, None, None, None), st


def _dequant64(q, st):
    import bitsandbytes_amd.functional as F

    return F.dequantize_4bit(q.view(-1, 1), st).double()


def _rel(got, want):
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-30))


def _bound(dt):
    return 1e-5 if dt == "fp32" else 1e-2


PLAIN_PROBLEMS = []  # (what _plain saw beside its result; run_section reports and clears it)


def _plain(lib, d, x, q, stats, bias, M, N):
    """bnb_mi355x_gemm_4bit on fresh tensors: [M, N]."""
    am, a8, code, off = stats
    dt = DTYPES[d["dtype"]]
    out = GB.Carved(M * N * dt.itemsize, 0, device=DEV, after=GB.after_band(64 * N * dt.itemsize))  # (bands: see Fresh)
    ws_bytes = lib.bnb_mi355x_gemm_4bit_workspace_bytes(0, DT_CODE[d["dtype"]], M, N, d["K"], d["bs"])
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    lib.bnb_mi355x_gemm_4bit(0, DT_CODE[d["dtype"]], x.data_ptr(), q.data_ptr(), am.data_ptr(), p(a8), p(code), p(off), None, out.ptr(), p(bias),
                             M, N, d["K"], d["bs"], QT_CODE[d["qt"]], ws.data_ptr() if ws_bytes else None, ws_bytes, _stream())
    torch.cuda.synchronize()
    if not out.guards_ok():
        PLAIN_PROBLEMS.append("the plain gemm_4bit call wrote outside its output")
    return out.bytes().view(dt).view(M, N)


# ---------------------------------------------------------------------------------------------- the sections
# Each: setup(lib, d) -> operands; supported(lib, d); call(lib, d, o, pl) enqueues the entry point with the placer's pointers;
# ref(lib, d, o, outs) -> None or a failure text, on the WANT's outputs (uint8 tensors, one per output).
class Decode:
    """gated / lora / lora_ids: the epilogues of the two decode kernels."""
    families = True

    def setup(self, lib, d):
        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        M, N, K = d["M"], d["N"], d["K"]
        o = dict(x=torch.randn(M, K, device=DEV).to(dt), bias=torch.randn(N, device=DEV).to(dt) if d["bias"] else None)
        o["q"], o["stats"], o["st"] = _quant((torch.randn(N, K, device=DEV) / K ** 0.5).to(dt), d["bs"], d["qt"], d["nested"])
        if d["section"] != "gated":
            r, A_n = d["r"], d.get("A_n", 1)
            o["t"] = torch.randn(M, r, device=DEV).to(dt)  # ([M, r] exactly: what follows it in the carved call is 0xFF)
            o["bl"] = (torch.randn(A_n, N, r, device=DEV) * 0.5).to(dt)
        if d["section"] == "lora_ids":
            o["scalings"] = (torch.rand(d["A_n"], device=DEV) * 2 + 0.25).float()
            o["ids"] = torch.tensor(d["ids"], dtype=IDX[d["index_bytes"]], device=DEV)
        return o

    def supported(self, lib, d):
        c = DT_CODE[d["dtype"]]
        if d["section"] == "gated":
            return lib.bnb_mi355x_gemm_4bit_gated_supported(c, d["M"], d["N"], d["K"], d["bs"])
        if d["section"] == "lora":
            return lib.bnb_mi355x_gemm_4bit_lora_supported(c, d["M"], d["N"], d["K"], d["bs"], int(d["nested"]), d["r"])
        return lib.bnb_mi355x_gemm_4bit_lora_ids_supported(c, d["M"], d["N"], d["K"], d["bs"], int(d["nested"]), d["r"], d["A_n"])

    def call(self, lib, d, o, pl):
        M, N, K = d["M"], d["N"], d["K"]
        am, a8, code, off = o["stats"]
        c, qt, es = DT_CODE[d["dtype"]], QT_CODE[d["qt"]], 2
        width = N // 2 if d["section"] == "gated" else N
        out = pl.out(M * width * es, 16 * width * es)
        if d["section"] == "gated":
            lib.bnb_mi355x_gemm_4bit_gated(c, pl.a16(o["x"]), pl.a16(o["q"]), pl.elt(am, 4), out, pl.elt(o["bias"]), M, N, K, d["bs"], qt, _stream())
            return
        t = o["t"]
        if pl.carved and d.get("none"):  # (no row has an adapter: lora_t is never read - all 0xFF in the carved call)
            t = torch.full((t.numel() * 2,), GB.NAN_PAT, dtype=torch.uint8, device=DEV).view(t.dtype).view(t.shape)
        head = (c, pl.a16(o["x"]), pl.a16(o["q"]), pl.elt(am, 4), pl.elt(a8), pl.elt(code), pl.elt(off), out, pl.elt(o["bias"]), pl.a16(t),
                pl.a16(o["bl"]))
        if d["section"] == "lora":
            lib.bnb_mi355x_gemm_4bit_lora(*head, d["scaling"], d["r"], M, N, K, d["bs"], qt, _stream())
        else:
            lib.bnb_mi355x_gemm_4bit_lora_ids(*head, pl.elt(o["scalings"], 4), pl.elt(o["ids"], d["index_bytes"]), d["index_bytes"], d["A_n"],
                                              d["r"], M, N, K, d["bs"], qt, _stream())

    def ref(self, lib, d, o, outs):
        import lora_cases as LC

        M, N = d["M"], d["N"]
        dt = DTYPES[d["dtype"]]
        y = _plain(lib, d, o["x"], o["q"], o["stats"], o["bias"], M, N)
        if d["section"] == "gated":
            got = outs[0].view(dt).view(M, N // 2)
            want = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
            return None if torch.equal(got, want) else f"not silu(gate) * up of the plain call: {int((got != want).sum())} elements differ"
        got = outs[0].view(dt).view(M, N)
        if not bool(torch.isfinite(got).all()):
            return "non-finite values in the output"
        for m in range(M):
            a = d["ids"][m] if d["section"] == "lora_ids" else 0
            if not 0 <= a < d.get("A_n", 1):
                if not torch.equal(got[m], y[m]):
                    return f"row {m} (no adapter, id {a}) is not the plain call's"
                continue
            s = float(o["scalings"][a]) if d["section"] == "lora_ids" else d["scaling"]
            t, b = o["t"][m:m + 1], o["bl"][a]
            want64 = y[m:m + 1].double() + s * (t.double() @ b.double().t())
            ratio = float(((got[m:m + 1].double() - want64).abs() / LC.tolerance(want64, y[m:m + 1], t, b, s, dt)).max())
            if not ratio <= 1.0:
                return f"row {m}: |out - (y + s t B^T)| is {ratio:.3f} of lora_cases.tolerance"
        return None


class Shrink:
    """shrink / shrink_ids: t = x @ lora_A^T, per-row adapters, the split layout."""
    families = False

    def setup(self, lib, d):
        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        M, K, R, A_n = d["M"], d["K"], d["R"], d.get("A_n", 1)
        o = dict(x=torch.randn(M, K, device=DEV).to(dt), a=(torch.randn(A_n, R, K, device=DEV) / K ** 0.5).to(dt))
        if d["section"] == "shrink_ids":
            o["ids"] = torch.tensor(d["ids"], dtype=IDX[d["index_bytes"]], device=DEV)
        return o

    def supported(self, lib, d):
        c = DT_CODE[d["dtype"]]
        if d["section"] == "shrink":
            return lib.bnb_mi355x_lora_shrink_supported(c, d["M"], d["R"], d["K"])
        return lib.bnb_mi355x_lora_shrink_ids_supported(c, d["M"], d["A_n"], d["R"], d["K"])

    def call(self, lib, d, o, pl):
        M, K, R = d["M"], d["K"], d["R"]
        n = 0 if d["splits"] is None else len(d["splits"])
        table = (ct.c_int * n)(*d["splits"]) if n else None  # (a host array, read during the call)
        out = pl.out(M * R * 2, 16 * R * 2)
        if d["section"] == "shrink":
            lib.bnb_mi355x_lora_shrink(DT_CODE[d["dtype"]], pl.a16(o["x"]), pl.a16(o["a"]), out, M, R, K, table, n, _stream())
        else:
            lib.bnb_mi355x_lora_shrink_ids(DT_CODE[d["dtype"]], pl.a16(o["x"]), pl.a16(o["a"]), pl.elt(o["ids"], d["index_bytes"]), d["index_bytes"],
                                           out, M, d["A_n"], R, K, table, n, _stream())

    def ref(self, lib, d, o, outs):
        import lora_multi_cases as LM
        import lora_shrink_cases as SC

        M, R = d["M"], d["R"]
        flat = outs[0].view(DTYPES[d["dtype"]])
        got = flat.view(M, R) if d["splits"] is None else torch.cat(SC.parts_of(flat, M, d["splits"]), dim=1)
        ids = d["ids"] if d["section"] == "shrink_ids" else [0] * M
        x, stack = o["x"].cpu(), o["a"].cpu()
        want = LM.reference(x, stack, ids) if d["section"] == "shrink_ids" else SC.reference(x, stack[0])
        for m, a in enumerate(ids):
            if not 0 <= a < stack.shape[0]:
                if bool((got[m].view(torch.int16) != 0).any()) or bool((want[m] != 0).any()):
                    return f"row {m} (no adapter, id {a}) is not exactly zero"
                continue
            want64 = x[m:m + 1].double() @ stack[a].double().t()  # (the reference in front of its one rounding: what the bound is about)
            ratio = float(((got[m:m + 1].cpu().double() - want64).abs() / SC.tolerance(want64, x[m:m + 1], stack[a])).max())
            if not ratio <= 1.0:
                return f"row {m}: |t - x A^T| is {ratio:.3f} of lora_shrink_cases.tolerance"
            if not bool(((want[m:m + 1].double() - want64).abs() <= SC.tolerance(want64, x[m:m + 1], stack[a])).all()):
                return f"row {m}: the reference itself is outside the bound"
        return None


class Experts:
    """experts / experts_ffn: one launch for any id pattern; rows of zeros for ids outside [0, E)."""
    families = False

    def setup(self, lib, d):
        import experts_cases as EC

        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        E, N, K, P = d["E"], d["N"], d["K"], d["P"]
        T, S = EC.TS_OF_P[P]
        o = dict(T=T, S=S, x=torch.randn(T if d["shared_rows"] else P, K, device=DEV).to(dt),
                 bias=torch.randn(E, N, device=DEV).to(dt) if d["bias"] else None)
        o["q"], o["stats"], o["st"] = _quant((torch.randn(E, N, K, device=DEV) / K ** 0.5).to(dt), d["bs"], d["qt"], d["nested"])
        ids = expert_ids(d)
        o["ids64"] = ids
        o["valid"] = ((ids >= 0) & (ids < E)).to(DEV)
        o["ids"] = ids.to(IDX[d["index_bytes"]]).to(DEV)
        if d["mode"].startswith("scale"):
            w = torch.rand(P, device=DEV) + 0.25
            w = torch.where(o["valid"], w, torch.full_like(w, float("nan")))  # (a NaN scale on every masked pair)
            o["scale"] = w if d["mode"] == "scale_fp32" else w.to(dt)
        return o

    def gated_code(self, d):
        return {"chunked": 1, "interleaved": 2}.get(d["mode"], 0)

    def supported(self, lib, d):
        c = DT_CODE[d["dtype"]]
        if d["section"] == "experts":
            return lib.bnb_mi355x_gemm_4bit_experts_supported(c, d["E"], d["N"], d["K"], d["bs"])
        return lib.bnb_mi355x_gemm_4bit_experts_ffn_supported(c, d["E"], d["N"], d["K"], d["bs"], self.gated_code(d))

    def width(self, d):
        return d["N"] // 2 if self.gated_code(d) else d["N"]

    def call(self, lib, d, o, pl, plain=False):
        E, N, K, P = d["E"], d["N"], d["K"], d["P"]
        am, a8, code, off = o["stats"]
        es = DTYPES[d["dtype"]].itemsize
        width = N if plain else self.width(d)
        out = pl.out(P * width * es, (P + 4) * width * es)
        head = (DT_CODE[d["dtype"]], pl.a16(o["x"]), 0 if d["shared_rows"] else K, pl.a16(o["q"]), pl.elt(am, 4), pl.elt(a8), pl.elt(code), pl.elt(off),
                pl.elt(o["bias"]), pl.elt(o["ids"], d["index_bytes"]), d["index_bytes"])
        tail = (out, P, o["S"], E, N, K, d["bs"], QT_CODE[d["qt"]], _stream())
        if plain or d["section"] == "experts":
            lib.bnb_mi355x_gemm_4bit_experts(*head, *tail)
        else:
            scale = o.get("scale")
            lib.bnb_mi355x_gemm_4bit_experts_ffn(*head, pl.elt(scale), DT_CODE[d["dtype"]] if d["mode"] == "scale_T" else 0, self.gated_code(d), *tail)

    def ref(self, lib, d, o, outs):
        E, N, K, P = d["E"], d["N"], d["K"], d["P"]
        dt = DTYPES[d["dtype"]]
        got = outs[0].view(dt).view(P, self.width(d))
        if bool((got[~o["valid"]].contiguous().view(torch.uint8) != 0).any()):
            return "a pair whose id is outside [0, E) is not a row of zeros"
        if self.gated_code(d):
            pl = Fresh()
            self.call(lib, d, o, pl, plain=True)
            torch.cuda.synchronize()
            y = pl.result().view(dt).view(P, N)
            g, u = (y[:, :N // 2], y[:, N // 2:]) if d["mode"] == "chunked" else (y[:, 0::2], y[:, 1::2])
            want = torch.nn.functional.silu(g) * u
            return None if torch.equal(got, want) else f"not silu(gate) * up of the plain call: {int((got != want).sum())} elements differ"
        W = _dequant64(o["q"], o["st"]).view(E, N, K)
        safe = torch.where(o["valid"], o["ids64"].to(DEV), torch.zeros(P, dtype=torch.int64, device=DEV))
        rows = o["x"].double()
        rows = rows.repeat_interleave(o["S"], dim=0) if d["shared_rows"] else rows
        want = torch.bmm(W[safe], rows.view(P, K, 1)).view(P, N)
        if o["bias"] is not None:
            want = want + o["bias"].double()[safe]
        if "scale" in o:
            want = want * torch.nan_to_num(o["scale"].double()).view(P, 1)
        want = want * o["valid"].view(P, 1)
        if not bool(torch.isfinite(got).all()):
            return "non-finite values in the output"
        if not bool(o["valid"].any()):
            return None
        err = _rel(got, want)
        return None if err < _bound(d["dtype"]) else f"relative error {err:.2e} against float64 dequantize-and-matmul"


class Grouped:
    """grouped: several matrices on one activation; every out[i] its own carved region."""
    families = False

    def setup(self, lib, d):
        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        M, K = d["M"], d["K"]
        o = dict(x=torch.randn(M, K, device=DEV).to(dt), mats=[])
        for N, has_bias in zip(d["Ns"], d["bias"]):
            q, stats, st = _quant((torch.randn(N, K, device=DEV) / K ** 0.5).to(dt), d["bs"], d["qt"], d["nested"])
            o["mats"].append(dict(q=q, stats=stats, st=st, bias=torch.randn(N, device=DEV).to(dt) if has_bias else None))
        o["route"] = lib.bnb_mi355x_gemm_4bit_grouped_route(DT_CODE[d["dtype"]], d["count"], (ct.c_int * d["count"])(*d["Ns"]), M, K, d["bs"])
        return o

    def supported(self, lib, d):
        return 1 if d["K"] % d["bs"] == 0 and 1 <= d["count"] <= 8 else 0  # (no predicate: any group inside these is served)

    def call(self, lib, d, o, pl):
        M, K, n = d["M"], d["K"], d["count"]
        cols = {k: [] for k in ("q", "am", "a8", "code", "off", "out", "bias")}
        x = pl.a16(o["x"])
        for N, m in zip(d["Ns"], o["mats"]):
            am, a8, code, off = m["stats"]
            for k, v in zip(cols, (pl.a16(m["q"]), pl.elt(am, 4), pl.elt(a8), pl.elt(code), pl.elt(off), pl.out(M * N * 2, 64 * N * 2), pl.elt(m["bias"]))):
                cols[k].append(v)
        arr = lambda vals: (ct.c_void_p * n)(*vals)  # noqa: E731  (host arrays of device pointers)
        nested = d["nested"]
        lib.bnb_mi355x_gemm_4bit_grouped(DT_CODE[d["dtype"]], x, n, arr(cols["q"]), arr(cols["am"]), arr(cols["a8"]) if nested else None,
                                         arr(cols["code"]) if nested else None, arr(cols["off"]) if nested else None, arr(cols["out"]),
                                         arr(cols["bias"]), (ct.c_int32 * n)(*d["Ns"]), M, K, d["bs"], QT_CODE[d["qt"]], _stream())

    def ref(self, lib, d, o, outs):
        M = d["M"]
        dt = DTYPES[d["dtype"]]
        exact = o["route"] in (0, 1) or (o["route"] == 2 and M <= 16)
        for i, (N, m) in enumerate(zip(d["Ns"], o["mats"])):
            got = outs[i].view(dt).view(M, N)
            y = _plain(lib, d, o["x"], m["q"], m["stats"], m["bias"], M, N)
            if exact and not torch.equal(got, y):
                return f"matrix {i} (N {N}, route {o['route']}) is not the separate gemm_4bit call's bits"
            if not exact and not _rel(got, y.double()) < 1e-2:
                return f"matrix {i} (N {N}, route 2 at {M} rows): {_rel(got, y.double()):.2e} from the separate call"
            want = o["x"].double() @ _dequant64(m["q"], m["st"]).view(N, d["K"]).t()
            if m["bias"] is not None:
                want = want + m["bias"].double()
            err = _rel(got, want)
            if not (err < _bound(d["dtype"]) and bool(torch.isfinite(got).all())):
                return f"matrix {i} (N {N}): relative error {err:.2e} against float64 dequantize-and-matmul"
        return None


class Rows:
    """rows: gathered dequantize. The launcher wants 4-byte aligned packed rows and a 16-byte aligned output."""
    families = False

    def setup(self, lib, d):
        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        o = dict(idx=torch.tensor(rows_indices(d), dtype=IDX[d["index_bytes"]], device=DEV))
        o["q"], o["stats"], o["st"] = _quant((torch.randn(d["num_rows"], d["dim"], device=DEV) * 0.1).to(dt), d["bs"], d["qt"], False)
        return o

    def supported(self, lib, d):
        return 1 if d["dim"] % 8 == 0 and d["dim"] % d["bs"] == 0 else 0

    def call(self, lib, d, o, pl):
        es = DTYPES[d["dtype"]].itemsize
        out = pl.out(d["count"] * d["dim"] * es, (d["count"] + 16) * d["dim"] * es)
        lib.bnb_mi355x_dequantize_4bit_rows(DT_CODE[d["dtype"]], pl.elt(o["q"], 4), pl.elt(o["stats"][0], 4), pl.elt(o["idx"], d["index_bytes"]),
                                            d["index_bytes"], out, d["count"], d["num_rows"], d["dim"], d["bs"], QT_CODE[d["qt"]], _stream())

    def ref(self, lib, d, o, outs):
        import bitsandbytes_amd.functional as F

        dt = DTYPES[d["dtype"]]
        full = F.dequantize_4bit(o["q"].view(-1, 1), o["st"]).view(d["num_rows"], d["dim"])
        want = full[o["idx"].long()]
        got = outs[0].view(dt).view(d["count"], d["dim"])
        return None if full.dtype == dt and torch.equal(got, want) else "not the rows of the full dequantize_4bit result"


class Legacy:
    """legacy: cquantize_blockwise_* (NULL stream), cgemm_4bit_<T>, cgemm_4bit_inference_naive_<T> - the reference ABI's names; no
    operand of theirs needs more than its element's alignment."""
    families = False

    def setup(self, lib, d):
        import bitsandbytes_amd.functional as F

        torch.manual_seed(d["seed"])
        dt = DTYPES[d["dtype"]]
        if d["kind"] in ("quant4", "quant8"):
            o = dict(x=(torch.randn(d["n"], device=DEV) * (0.1 if d["kind"] == "quant4" else 1.0)).to(dt))
            if d["kind"] == "quant8":
                o["code8"] = F._dynamic_map(torch.device(DEV, torch.cuda.current_device()))
            return o
        M, N, K = d["M"], d["N"], d["K"]
        o = dict(x=torch.randn(M, K, device=DEV).to(dt), bias=torch.randn(N, device=DEV).to(dt) if d["bias"] else None)
        o["q"], o["stats"], o["st"] = _quant((torch.randn(N, K, device=DEV) / K ** 0.5).to(dt), d["bs"], d["qt"], d["nested"])
        o["code16"] = F.get_4bit_type(d["qt"], device=DEV).float().contiguous()
        return o

    def supported(self, lib, d):
        return 1

    def bit_exact(self, d):
        """The matmuls run the generic kernel - another order of summation - on operands that are not 16-byte aligned (the header's
        "aligned pointers"): guard_stress.py's bound on both placements in place of equal bits."""
        return d["kind"] in ("quant4", "quant8")

    def call(self, lib, d, o, pl):
        es = DTYPES[d["dtype"]].itemsize
        torch.cuda.synchronize()
        if d["kind"] == "quant4":
            n, blocks = d["n"], -(d["n"] // -d["bs"])
            getattr(lib, f"cquantize_blockwise_{d['dtype']}_{d['qt']}")(None, pl.elt(o["x"]), pl.out(blocks * 4, blocks * 4, 4), pl.out((n + 1) // 2, n, 1), d["bs"], n)
        elif d["kind"] == "quant8":
            n, blocks = d["n"], -(d["n"] // -d["bs"])
            getattr(lib, f"cquantize_blockwise_{d['dtype']}")(pl.elt(o["code8"], 4), pl.elt(o["x"]), pl.out(blocks * 4, blocks * 4, 4), pl.out(n, n, 1), d["bs"], n)
        elif d["kind"] == "gemm":
            M, N, K = d["M"], d["N"], d["K"]
            am, a8, code, off = o["stats"]
            getattr(lib, f"cgemm_4bit_{d['dtype']}")(pl.elt(o["x"]), pl.elt(o["q"], 1), pl.elt(am, 4), pl.elt(a8), pl.elt(code), pl.elt(off),
                                                     pl.out(M * N * es, 64 * N * es, es), pl.elt(o["bias"]), M, N, K, d["bs"], QT_CODE[d["qt"]], _stream())
        else:
            N, K = d["N"], d["K"]
            getattr(lib, f"cgemm_4bit_inference_naive_{d['dtype']}")(N, 1, K, pl.elt(o["x"]), pl.elt(o["q"], 1), pl.elt(o["stats"][0], 4), pl.elt(o["code16"], 4),
                                                                     pl.out(N * es, 16 * N * es, es), N, (K + 1) // 2, N, d["bs"], _stream())

    def ref(self, lib, d, o, outs):
        dt = DTYPES[d["dtype"]]
        if d["kind"] == "quant4":
            q, am = torch.ops.bitsandbytes.quantize_4bit.default(o["x"], d["bs"], d["qt"], torch.uint8)
            ok = torch.equal(outs[0].view(torch.int32), am.view(torch.int32).view(-1)) and torch.equal(outs[1], q.view(-1))
            return None if ok else "not quantize_4bit's codes and absmax"
        if d["kind"] == "quant8":
            q, am = torch.ops.bitsandbytes.quantize_blockwise.default(o["x"], o["code8"], d["bs"])
            ok = torch.equal(outs[0].view(torch.int32), am.view(torch.int32).view(-1)) and torch.equal(outs[1], q.view(-1))
            return None if ok else "not quantize_blockwise's codes and absmax"
        M, N, K = d["M"], d["N"], d["K"]
        got = outs[0].view(dt).view(M, N)
        want = o["x"].double() @ _dequant64(o["q"], o["st"]).view(N, K).t()
        if o["bias"] is not None:
            want = want + o["bias"].double()
        err = _rel(got, want)
        ok = err < _bound(d["dtype"]) and bool(torch.isfinite(got).all())
        return None if ok else f"relative error {err:.2e} against float64 dequantize-and-matmul"


RUNNERS = {"legacy": Legacy, "gated": Decode, "lora": Decode, "lora_ids": Decode, "shrink": Shrink, "shrink_ids": Shrink, "experts": Experts,
           "experts_ffn": Experts, "grouped": Grouped, "rows": Rows}


def label(d):
    return ", ".join(f"{k} {v}" for k, v in d.items() if k not in ("section", "seed"))


def run_section(lib, section, n, seed):
    """(draws run, draws passed, {family: draws}, failures)"""
    runner = RUNNERS[section]()
    rng = random.Random(f"place/{section}/{seed}")
    passed, fams, fails = 0, {}, 0

    def fail(d, text):
        print(f"{section}: FAIL draw {d['i']}: {text} [{label(d)}]", flush=True)

    cases = draws(section, n, seed)
    for d in cases:
        if runner.supported(lib, d) != 1:
            fail(d, "the _supported predicate answers 0")
            fails += 1
            continue
        o = runner.setup(lib, d)
        want = Fresh()
        runner.call(lib, d, o, want)
        torch.cuda.synchronize()
        fam_w = lib.bnb_mi355x_last_gemm_kernel() if runner.families else None
        pl = Placed(rng)
        runner.call(lib, d, o, pl)
        torch.cuda.synchronize()
        fam_c = lib.bnb_mi355x_last_gemm_kernel() if runner.families else None
        problems = []
        if runner.families:
            fams[fam_c] = fams.get(fam_c, 0) + 1
            if fam_w != fam_c:
                problems.append(f"kernel family {fam_c} in the carved call, {fam_w} on fresh tensors")
            if fam_w not in (K_STREAM, K_SM):
                problems.append(f"kernel family {fam_w}: neither the streaming nor the streaming MFMA kernel")
        if not pl.ok():
            problems.append("a guard band of an output was written")
        if not want.ok():
            problems.append("a guard band of an output was written (fresh tensors)")
        exact = getattr(runner, "bit_exact", lambda d: True)(d)
        for i in range(len(pl.outs)):
            if exact and not torch.equal(pl.result(i), want.result(i)):
                diff = int((pl.result(i) != want.result(i)).sum())
                problems.append(f"output {i}: {diff} bytes differ between the carved call and fresh tensors")
        for which in (want,) if exact else (want, pl):  # (no promise of equal bits: the reference judges both placements)
            text = runner.ref(lib, d, o, [which.result(i) for i in range(len(which.outs))])
            if text:
                problems.append(text + ("" if which is want else " (carved call)"))
        problems += PLAIN_PROBLEMS
        del PLAIN_PROBLEMS[:]
        for text in problems:
            fail(d, text)
        fails += len(problems)
        passed += not problems
    if runner.families:  # (coverage: both decode kernels, a third of the draws each)
        for fam in (K_STREAM, K_SM):
            if 3 * fams.get(fam, 0) < len(cases):
                print(f"{section}: FAIL coverage: family {fam} in {fams.get(fam, 0)} of {len(cases)} draws (a third wanted)", flush=True)
                fails += 1
    return len(cases), passed, fams, fails


# ---------------------------------------------------------------------------------------------- the Python layer
def misaligned(t, off):
    """A contiguous view with t's values, `off` bytes past a 256-byte-aligned address."""
    nbytes = t.numel() * t.element_size()
    buf = torch.empty(nbytes + 512, dtype=torch.uint8, device=t.device)
    start = (-buf.data_ptr()) % 256 + off
    v = buf[start:start + nbytes].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == off
    return v


def run_python_guards(lib, n, seed):
    """Every 16-byte operand in turn as a contiguous view at a 2-byte offset (packed weights: 1 and 8 bytes): the raw op raises -
    the process lives -, the public function returns the aligned call's values (its docstring's bits or item 6's tolerance)."""
    import bitsandbytes_amd as bnb
    import bitsandbytes_amd.functional as F
    import lora_cases as LC
    import lora_shrink_cases as SC

    ops = torch.ops.bitsandbytes_amd
    checks, passed, fails = 0, 0, 0

    def check(name, cond, text=""):
        nonlocal checks, passed, fails
        checks += 1
        if cond:
            passed += 1
        else:
            fails += 1
            print(f"python_guards: FAIL {name} {text}", flush=True)

    def raises(name, fn):
        try:
            fn()
        except (ValueError, RuntimeError):
            check(name, True)
            return
        torch.cuda.synchronize()
        check(name, False, "the raw op took a misaligned operand")

    def variants(args, which):
        """(name, args with one operand misaligned) for every 16-byte operand; `which`: {key: offsets}"""
        for key, offs in which.items():
            for off in offs:
                yield f"{key}+{off}", dict(args, **{key: misaligned(args[key], off)})

    for d in draws("python_guards", n, seed):
        torch.manual_seed(seed + d["i"])
        M, N, K, r = d["M"], d["N"], d["K"], d["r"]
        dt = DTYPES[d["dtype"]]
        tag = f"M {M} N {N} K {K} r {r} {d['dtype']}"
        x = torch.randn(M, K, device=DEV).to(dt)
        W = (torch.randn(N, K, device=DEV) / K ** 0.5).to(dt)
        q, st = F.quantize_4bit(W, blocksize=64, quant_type="nf4")
        # ---- gated (N even)
        a = dict(x=x, q=q)
        want = bnb.matmul_4bit_gated(x, q, st)
        for name, v in variants(a, {"x": (2,), "q": (1, 8)}):
            raises(f"gemm_4bit_gated {name} {tag}", lambda: ops.gemm_4bit_gated.default(v["x"], v["q"], st.shape, st.absmax, 64, "nf4"))
            check(f"matmul_4bit_gated {name} {tag}", torch.equal(bnb.matmul_4bit_gated(v["x"], v["q"], st), want), "differs from the aligned call")
        # ---- lora, lora_ids
        A_n = 3
        t = torch.randn(M, r, device=DEV).to(dt)
        bl = (torch.randn(A_n, N, r, device=DEV) * 0.5).to(dt)
        sc = torch.tensor([0.5, 2.0, 1.25], device=DEV)
        ids = torch.tensor([(1, -1, 2, A_n, 0)[m % 5] for m in range(M)], dtype=torch.int32, device=DEV)
        y = torch.ops.bitsandbytes.gemm_4bit.default(x, q, st.shape, st.absmax, 64, "nf4")
        a = dict(x=x, q=q, t=t, bl=bl[1])
        want = bnb.matmul_4bit_lora(x, q, st, t, bl[1], 0.5)
        want64 = y.double() + 0.5 * (t.double() @ bl[1].double().t())
        tol = LC.tolerance(want64, y, t, bl[1], 0.5, dt)
        check(f"matmul_4bit_lora aligned {tag}", bool(((want.double() - want64).abs() <= tol).all()), "outside lora_cases.tolerance")
        for name, v in variants(a, {"x": (2,), "q": (1, 8), "t": (2,), "bl": (2,)}):
            raises(f"gemm_4bit_lora {name} {tag}", lambda: ops.gemm_4bit_lora.default(v["x"], v["q"], st.shape, st.absmax, 64, "nf4", v["t"], v["bl"], 0.5))
            got = bnb.matmul_4bit_lora(v["x"], v["q"], st, v["t"], v["bl"], 0.5)
            check(f"matmul_4bit_lora {name} {tag}", bool(((got.double() - want64).abs() <= tol).all()), "outside lora_cases.tolerance")
            check(f"matmul_4bit_lora {name} {tag} bits", torch.equal(got, want), "differs from the aligned call")
        a = dict(x=x, q=q, t=t, bl=bl)
        want = bnb.matmul_4bit_lora_ids(x, q, st, t, bl, sc, ids)

        def ids_ok(got):
            for m in range(M):
                i = int(ids[m])
                if not 0 <= i < A_n:
                    if not torch.equal(got[m], y[m]):
                        return False
                    continue
                w64 = y[m:m + 1].double() + float(sc[i]) * (t[m:m + 1].double() @ bl[i].double().t())
                if not bool(((got[m:m + 1].double() - w64).abs() <= LC.tolerance(w64, y[m:m + 1], t[m:m + 1], bl[i], float(sc[i]), dt)).all()):
                    return False
            return True

        check(f"matmul_4bit_lora_ids aligned {tag}", ids_ok(want), "outside lora_cases.tolerance")
        for name, v in variants(a, {"x": (2,), "q": (1, 8), "t": (2,), "bl": (2,)}):
            raises(f"gemm_4bit_lora_ids {name} {tag}",
                   lambda: ops.gemm_4bit_lora_ids.default(v["x"], v["q"], st.shape, st.absmax, 64, "nf4", v["t"], v["bl"], sc, ids))
            got = bnb.matmul_4bit_lora_ids(v["x"], v["q"], st, v["t"], v["bl"], sc, ids)
            check(f"matmul_4bit_lora_ids {name} {tag}", ids_ok(got), "outside lora_cases.tolerance")
            check(f"matmul_4bit_lora_ids {name} {tag} bits", torch.equal(got, want), "differs from the aligned call")
        # ---- shrink, shrink_ids
        R = 24
        la = (torch.randn(A_n, R, K, device=DEV) / K ** 0.5).to(dt)
        a = dict(x=x, la=la[0])
        want64 = x.double() @ la[0].double().t()
        tol = SC.tolerance(want64, x, la[0])
        want = bnb.lora_shrink(x, la[0])
        check(f"lora_shrink aligned {tag}", bool(((want.double() - want64).abs() <= tol).all()), "outside lora_shrink_cases.tolerance")
        for name, v in variants(a, {"x": (2,), "la": (2,)}):
            raises(f"lora_shrink {name} {tag}", lambda: ops.lora_shrink.default(v["x"], v["la"]))
            got = bnb.lora_shrink(v["x"], v["la"])
            check(f"lora_shrink {name} {tag}", bool(((got.double() - want64).abs() <= tol).all()), "outside lora_shrink_cases.tolerance")
            check(f"lora_shrink {name} {tag} bits", torch.equal(got, want), "differs from the aligned call")

        def shrink_ids_ok(got):
            for m in range(M):
                i = int(ids[m])
                if not 0 <= i < A_n:
                    if bool((got[m] != 0).any()):
                        return False
                    continue
                w64 = x[m:m + 1].double() @ la[i].double().t()
                if not bool(((got[m:m + 1].double() - w64).abs() <= SC.tolerance(w64, x[m:m + 1], la[i])).all()):
                    return False
            return True

        a = dict(x=x, la=la)
        want = bnb.lora_shrink_ids(x, la, ids)
        check(f"lora_shrink_ids aligned {tag}", shrink_ids_ok(want), "outside lora_shrink_cases.tolerance")
        for name, v in variants(a, {"x": (2,), "la": (2,)}):
            raises(f"lora_shrink_ids {name} {tag}", lambda: ops.lora_shrink_ids.default(v["x"], v["la"], ids))
            got = bnb.lora_shrink_ids(v["x"], v["la"], ids)
            check(f"lora_shrink_ids {name} {tag}", shrink_ids_ok(got), "outside lora_shrink_cases.tolerance")
            check(f"lora_shrink_ids {name} {tag} bits", torch.equal(got, want), "differs from the aligned call")
        # ---- experts, experts_ffn, moe_ffn: the expert kernel is one family; (E, N, K, bs) = (8, 512, 1024, 128) of the experts list, whose
        # I = 256 is a whole number of blocks for the down projection; M pairs, one slot
        E, N2, K2, bs2 = EXPERT_SHAPES[3]
        x2 = torch.randn(M, K2, device=DEV).to(dt)
        qg, sg = F.quantize_4bit((torch.randn(E, N2, K2, device=DEV) / K2 ** 0.5).to(dt), blocksize=bs2, quant_type="nf4")
        qd, sd = F.quantize_4bit((torch.randn(E, K2, N2 // 2, device=DEV) / (N2 // 2) ** 0.5).to(dt), blocksize=bs2, quant_type="nf4")
        eids = torch.tensor([[(1, -1, 3, E, 0)[m % 5]] for m in range(M)], dtype=torch.int32, device=DEV)
        w = torch.rand(M, 1, device=DEV) + 0.25
        want = bnb.matmul_4bit_experts(x2, qg, sg, eids)
        want_g = bnb.matmul_4bit_experts(x2, qg, sg, eids, gated="chunked")
        want_s = bnb.matmul_4bit_experts(x2, qg, sg, eids, row_scale=w)
        want_f = bnb.moe_ffn_4bit(x2, qg, sg, qd, sd, eids, w)
        for name, v in variants(dict(x=x2, q=qg), {"x": (2,), "q": (1, 8)}):
            raises(f"gemm_4bit_experts {name} {tag}", lambda: ops.gemm_4bit_experts.default(v["x"], v["q"], sg.shape, sg.absmax, eids, bs2, "nf4"))
            raises(f"gemm_4bit_experts_ffn {name} {tag}",
                   lambda: ops.gemm_4bit_experts_ffn.default(v["x"], v["q"], sg.shape, sg.absmax, eids, bs2, "nf4", gated="chunked"))
            check(f"matmul_4bit_experts {name} {tag}", torch.equal(bnb.matmul_4bit_experts(v["x"], v["q"], sg, eids), want), "differs from the aligned call")
            check(f"matmul_4bit_experts gated {name} {tag}", torch.equal(bnb.matmul_4bit_experts(v["x"], v["q"], sg, eids, gated="chunked"), want_g),
                  "differs from the aligned call")
            check(f"matmul_4bit_experts row_scale {name} {tag}", torch.equal(bnb.matmul_4bit_experts(v["x"], v["q"], sg, eids, row_scale=w), want_s),
                  "differs from the aligned call")
        for name, v in variants(dict(x=x2, q=qg, qd=qd), {"x": (2,), "q": (1, 8), "qd": (1, 8)}):
            check(f"moe_ffn_4bit {name} {tag}", torch.equal(bnb.moe_ffn_4bit(v["x"], v["q"], sg, v["qd"], sd, eids, w), want_f), "differs from the aligned call")
        # ---- dequantize_4bit_rows: the packed table at a 1-byte offset (the launcher wants 4) - the op copies it
        tq, ts = F.quantize_4bit((torch.randn(ROWS_TABLE, K, device=DEV) * 0.1).to(dt), blocksize=64, quant_type="nf4")
        idx = torch.tensor([ROWS_TABLE - 1, 0, 5, 5], device=DEV)
        want = ops.dequantize_4bit_rows.default(tq, ts.absmax, idx, K, 64, "nf4", dt)
        check(f"dequantize_4bit_rows aligned {tag}", torch.equal(want, F.dequantize_4bit(tq, ts)[idx]), "not the rows of the full dequantize")
        for off in (1, 2):
            check(f"dequantize_4bit_rows q+{off} {tag}", torch.equal(ops.dequantize_4bit_rows.default(misaligned(tq, off), ts.absmax, idx, K, 64, "nf4", dt), want),
                  "differs from the aligned call")
    torch.cuda.synchronize()
    return checks, passed, {}, fails


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=24)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--only", choices=SECTIONS, default=None)
    a = ap.parse_args()
    import bitsandbytes_amd as bnb

    total = 0
    for section in SECTIONS if a.only is None else (a.only,):
        run, passed, fams, fails = (run_python_guards if section == "python_guards" else lambda lib, n, s: run_section(lib, section, n, s))(
            bnb.lib, a.draws, a.seed)
        total += fails
        what = "checks" if section == "python_guards" else "draws"
        tail = "" if not fams else ", families " + ", ".join(f"{k}: {v}" for k, v in sorted(fams.items()))
        print(f"{section}: {a.draws if what == 'draws' else run} {what}, seed {a.seed}: {passed}/{run} passed{tail}", flush=True)
    print("GUARD_FUSED " + ("OK" if total == 0 else f"FAILED ({total})"))
    sys.exit(0 if total == 0 else 1)


if __name__ == "__main__":
    main()
