#!/usr/bin/env python3
"""A/B of the fixed-cost levers of the M = 1 streaming kernel (csrc/gemv4_stream.hip), each alone, in one process:
    built-in   the production selection: exact-geometry instance where the geometry allows it, epilogue pointers requested early
    general    stream-tuning knob nt = 2: the general instance everywhere (lever B off)
    late-args  nt = 3: the general instance with the epilogue's kernarg load where it is used (levers A and B off: the form up to round 6)
(The store-policy variants of y - write-through, non-temporal - were measured with this tool and dropped with their code: DESIGN 6b.)
bf16, one activation row; config 2 (NF4, bs 64, fp32 absmax) and config 5 (FP4, bs 128, nested absmax). Per-launch us over an HBM-resident
rotation of distinct layers, hipGraph-replayed (launch-to-launch time in a dependent stream).
    python tools/stream_fixed_cost_ab.py [--quick] [--rounds 5]
Method (tools/stream_prologue_ab.py): every variant's graph is captured once, the timed region is >= 15 ms of replays, the variants are
measured round-robin over several rounds; the table shows the MEDIAN over the rounds and each variant's own spread (max - min over the
rounds) - a lever counts only where it is ahead by more than the spread of the variant without it.
First: every variant's output must equal the production instance's bit for bit on every shape (no variant moves arithmetic)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bitsandbytes_amd as bnb  # noqa: E402
from bitsandbytes_amd.backends import hip  # noqa: E402
from stream_ab import alg_bytes, make_layers  # noqa: E402
from stream_prologue_ab import timed  # noqa: E402

SHAPES = [(4096, 4096), (8192, 8192), (14336, 4096), (11008, 4096), (1376, 4096), (512, 11008)]
QUANT = [("config2 nf4 bs64", 64, "nf4", False), ("config5 fp4 bs128 nested", 128, "fp4", True)]
VARIANTS = [("built-in", -1), ("general", 2), ("late-args", 3)]


def tune(nt=-1):
    bnb.lib.bnb_mi355x_set_stream_tuning(0, 0, 0, nt, 0)


def one(q, st, x, out=None):
    if st.nested:
        return hip._gemm_4bit_fused(x, q, st.shape, st.state2.absmax, st.blocksize, st.quant_type, None, st.absmax, st.state2.code, st.offset,
                                    kernel=3, out=out)
    return hip._gemm_4bit_fused(x, q, st.shape, st.absmax, st.blocksize, st.quant_type, None, None, None, None, kernel=3, out=out)


def capture(layers, x, outs):
    def fn():
        for (q, st), o in zip(layers, outs):
            one(q, st, x, o)

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), bnb.lib.bnb_mi355x_version().decode(), os.environ.get("BNB_MI355X_LIBRARY", "product library"))
    variants = VARIANTS
    shapes = SHAPES[:2] if args.quick else SHAPES
    print("# bit identity of every variant with the production instance; exact = the host's answer (bnb_mi355x_gemv_4bit_stream_exact)")
    for qname, bs, qt, dq in QUANT:
        for (N, K) in shapes:
            layers = make_layers(N, K, bs, qt, dq, cap=2)
            x = torch.randn(1, K, device="cuda").bfloat16()
            tune()
            exact = bnb.lib.bnb_mi355x_gemv_4bit_stream_exact(2, 1, N, K, bs, int(dq))
            ref = [one(q, st, x).clone() for q, st in layers]
            bad = []
            for label, nt in variants[1:]:
                tune(nt)
                got = [one(q, st, x).clone() for q, st in layers]
                torch.cuda.synchronize()
                if not all(torch.equal(a, b) for a, b in zip(ref, got)):
                    bad.append(label)
            tune()
            print(f"   {qname:>26s} {N:6d} x {K:5d} exact={exact}: " + ("identical" if not bad else f"DIFFERENT: {bad}   <-- FAIL"), flush=True)
            del layers
    print(f"# us per launch, M = 1: median of {args.rounds} round-robin rounds, each >= 15 ms of graph replays (spread = max - min of the rounds)")
    for qname, bs, qt, dq in QUANT:
        print(f"## {qname}")
        print(f"{'N x K':>14s} " + " ".join(f"{v[0]:>16s}" for v in variants) + "   built-in: GB/s")
        for (N, K) in shapes:
            layers = make_layers(N, K, bs, qt, dq)
            L = len(layers)
            x = torch.randn(1, K, device="cuda").bfloat16()
            outs = [torch.empty(1, N, device="cuda", dtype=torch.bfloat16) for _ in layers]
            graphs = []
            for label, nt in variants:  # the tuning is read at launch time, i.e. at capture: one graph per variant
                tune(nt)
                graphs.append(capture(layers, x, outs))
            tune()
            t0 = timed(graphs[0], L, 20)
            reps = max(20, int(15000.0 / (t0 * L)) + 1)
            samples = [[] for _ in variants]
            for r in range(args.rounds):
                order = list(range(len(variants)))
                if r % 2:
                    order.reverse()
                for i in order:
                    samples[i].append(timed(graphs[i], L, reps))
            med = [statistics.median(s) for s in samples]
            cells = [f"{m:7.3f} ({max(s) - min(s):5.3f})" for m, s in zip(med, samples)]
            ab = alg_bytes(1, N, K, bs, dq)
            print(f"{N:>7d}x{K:<6d} " + " ".join(f"{c:>16s}" for c in cells) + f"   {ab / med[0] / 1e3:8.1f}", flush=True)
            del layers, graphs


if __name__ == "__main__":
    main()
