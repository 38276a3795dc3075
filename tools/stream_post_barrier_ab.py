#!/usr/bin/env python3
"""A/B of the post-barrier lever of the M = 1 streaming kernel (csrc/gemv4_stream.hip) in one process:
    built-in      the production selection: the row sum of an item finished in-lane (two row_bcast DPP adds), stored by lane 63
    readlane      stream-tuning knob nt = 4: the row sum combined through v_readlane / SGPRs, stored by lane 0 (lever off) on the
                  instance the launch selects - exact geometry where the shape allows it
    general       nt = 2: the built-in form on the general instance everywhere
    gen-readlane  nt = 5: the lever off on the general instance everywhere
(the last two differ from the first two on the exact shapes only: the lever on the general family at 4096 x 4096 and 14336 x 4096).
(A second lever - an fp32 activation image converted once by the builder wavefronts - was measured with this tool and dropped with its
code: DESIGN 6b, profiles/stream_post_barrier_ab.txt.)
bf16, one activation row; config 2 (NF4, bs 64, fp32 absmax) and config 5 (FP4, bs 128, nested absmax: general instance only). Per-launch
us over an HBM-resident rotation of distinct layers, hipGraph-replayed (launch-to-launch time in a dependent stream).
    python tools/stream_post_barrier_ab.py [--quick] [--rounds 5]
Method (tools/stream_fixed_cost_ab.py): every variant's graph is captured once, the timed region is >= 15 ms of replays, the variants
are measured round-robin over several rounds; the table shows the MEDIAN over the rounds and each variant's own spread (max - min over
the rounds) - the lever counts only where it is ahead by more than the spread of the variant without it.
First: every variant's output must equal the production instance's bit for bit on every shape (no variant moves arithmetic)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bitsandbytes_amd as bnb  # noqa: E402
from stream_ab import alg_bytes, make_layers  # noqa: E402
from stream_fixed_cost_ab import QUANT, SHAPES, capture, one, tune  # noqa: E402
from stream_prologue_ab import timed  # noqa: E402

VARIANTS = [("built-in", -1), ("readlane", 4), ("general", 2), ("gen-readlane", 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), bnb.lib.bnb_mi355x_version().decode(), os.environ.get("BNB_MI355X_LIBRARY", "product library"))
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
            for label, nt in VARIANTS[1:]:
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
        print(f"{'N x K':>14s} " + " ".join(f"{v[0]:>16s}" for v in VARIANTS) + "   built-in: GB/s")
        for (N, K) in shapes:
            layers = make_layers(N, K, bs, qt, dq)
            L = len(layers)
            x = torch.randn(1, K, device="cuda").bfloat16()
            outs = [torch.empty(1, N, device="cuda", dtype=torch.bfloat16) for _ in layers]
            graphs = []
            for label, nt in VARIANTS:  # the tuning is read at launch time, i.e. at capture: one graph per variant
                tune(nt)
                graphs.append(capture(layers, x, outs))
            tune()
            t0 = timed(graphs[0], L, 20)
            reps = max(20, int(15000.0 / (t0 * L)) + 1)
            samples = [[] for _ in VARIANTS]
            for r in range(args.rounds):
                order = list(range(len(VARIANTS)))
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
