#!/usr/bin/env python3
"""The dense gated-SiLU FFN block on one GPU (bitsandbytes_amd.nn.FFN4bit / ffn_4bit: gated launch + down) against the same block
from the operations the library offered before it, us per block of a decode step; and the gated launch against the plain launch on
the same interleaved [2F, H] matrix.

Method (tools/bench_moe_ffn.py): every leg is a hipGraph of >= 64 blocks that rotate over enough distinct layers that the weights of
one pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms); the legs alternate
inside one process, order reversed every round; median and min ... max of the rounds. Legs:
  fused    FFN4bit.from_linears(gate, up, down)(x): the gated launch, the down launch                           2 launches
  parent   linear4bit_group_forward([gate, up], x) -> F.silu(g) * u -> down                                     4 launches
  gated    the first launch of `fused` alone, writing [M, F]
  plain    matmul_4bit on the same interleaved matrix, writing [M, 2F]
The table is written to profiles/ffn_bench.txt (--out), replacing the file.
    python tools/bench_ffn.py [--rounds 5] [--quick] [--out profiles/ffn_bench.txt]"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bitsandbytes_amd as bnb  # noqa: E402
from tools.bench_experts import BS, CACHE_BYTES, capture, timed  # noqa: E402

# (label, F, H): gate / up [F, H], down [H, F]
SHAPES = [("Llama-3-8B 14336 x 4096", 14336, 4096), ("Llama-2-7B 11008 x 4096", 11008, 4096), ("4096 x 4096", 4096, 4096)]
MS = (1, 2, 4, 8, 16)


def layer(in_f, out_f, gen):
    l = bnb.nn.Linear4bit(in_f, out_f, bias=False, quant_type="nf4", compress_statistics=False, compute_dtype=torch.bfloat16)
    W = (torch.randn(out_f, in_f, device="cuda", generator=gen) / in_f ** 0.5).bfloat16()
    l.weight = bnb.nn.Params4bit(W.cpu(), requires_grad=False, quant_type="nf4", compress_statistics=False, blocksize=BS, module=l)
    return l.to("cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="M = 1 and 4 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_bench.txt"),
                    help="the table is also written to this file, replacing it ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per block / per launch: median (min ... max) of {args.rounds} rounds; NF4, blocksize {BS}, plain statistics, bf16, no bias; "
        "x is [M, H]")
    say(f"{'shape':>24s} {'M':>2s} {'fused block':>24s} {'parent block':>24s} {'saved':>7s} {'ratio':>6s} "
        f"{'gated launch':>24s} {'plain launch':>24s} {'gated-plain':>11s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    from bitsandbytes_amd.nn import linear4bit_group_forward

    with torch.no_grad():
        for label, F_, H in SHAPES:
            per_block = 3 * F_ * H // 2 + 3 * F_ * H // BS * 4
            L = max(2, min(48, math.ceil(1.25 * CACHE_BYTES / per_block)))
            members = [(layer(H, F_, gen), layer(H, F_, gen), layer(F_, H, gen)) for _ in range(L)]
            blocks = [bnb.nn.FFN4bit.from_linears(g, u, d, keep_members=True) for g, u, d in members]
            calls = L * math.ceil(64 / L)
            for M in ((1, 4) if args.quick else MS):
                x = torch.randn(M, H, device="cuda", generator=gen).bfloat16()

                def fused():
                    for c in range(calls):
                        blocks[c % L](x)

                def parent():
                    for c in range(calls):
                        g, u, d = members[c % L]
                        a, b = linear4bit_group_forward([g, u], x)
                        d(TF.silu(a) * b)

                def gated():
                    for c in range(calls):
                        blk = blocks[c % L]
                        bnb.matmul_4bit_gated(x, blk.gate_up, blk.gate_up_state)

                def plain():
                    for c in range(calls):
                        blk = blocks[c % L]
                        bnb.matmul_4bit(x, blk.gate_up, blk.gate_up_state)

                legs = [fused, parent, gated, plain]
                graphs = [capture(fn) for fn in legs]
                samples = [[] for _ in legs]
                reps = [max(2, int(10000.0 / (timed(g, calls, 1) * calls)) + 1) for g in graphs]
                for r in range(args.rounds):
                    order = range(len(legs)) if r % 2 == 0 else reversed(range(len(legs)))
                    for i in order:
                        samples[i].append(timed(graphs[i], calls, reps[i]))
                cols = [f"{statistics.median(s):8.2f} ({min(s):.2f}...{max(s):.2f})" for s in samples]
                med = [statistics.median(s) for s in samples]
                say(f"{label:>24s} {M:>2d} {cols[0]:>24s} {cols[1]:>24s} {med[1] - med[0]:7.2f} {med[1] / med[0]:5.2f}x "
                    f"{cols[2]:>24s} {cols[3]:>24s} {med[2] - med[3]:+11.2f}")
                del graphs
            del members, blocks
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
