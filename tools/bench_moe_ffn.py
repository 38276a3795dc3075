#!/usr/bin/env python3
"""The fused expert FFN block (bitsandbytes_amd.moe_ffn_4bit: gated launch, row-scaled launch, slot sum) against the same block from
the operations the library offered before it, us per block of a decode step; and the gated launch against the plain launch on the
same [E, 2I, K] stack.

Method (tools/bench_experts.py): every leg is a hipGraph of >= 64 blocks that rotate over enough distinct (gate_up, down) stack pairs
that the weights selected by one pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays
(regions >= 10 ms); the legs alternate inside one process, order reversed every round; median and min ... max of the rounds. Legs:
  fused    moe_ffn_4bit(x, gate_up, ..., down, ..., ids, w)                                                    3 launches (2 at S = 1)
  parent   matmul_4bit_experts -> chunk / F.silu / * -> matmul_4bit_experts -> * w -> sum                       6 launches
  gated    the first launch of `fused` alone, writing [T, S, I]
  plain    the first launch of `parent` alone, writing [T, S, 2I]
The table is written to profiles/moe_ffn_bench.txt (--out), replacing the file.
    python tools/bench_moe_ffn.py [--rounds 5] [--quick] [--out profiles/moe_ffn_bench.txt]"""
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
import bitsandbytes_amd.functional as F  # noqa: E402
from tools.bench_experts import BS, CACHE_BYTES, capture, timed  # noqa: E402

# (label, E, I, H, S, T values): gate_up [E, 2I, H], down [E, H, I]
SHAPES = [
    ("Mixtral 8 x 28672 x 4096 + 8 x 4096 x 14336", 8, 14336, 4096, 2, (1, 4, 16)),
    ("128 x 1536 x 2048 + 128 x 2048 x 768", 128, 768, 2048, 8, (1, 4, 8)),
]


def quantized(E, N, K, gen):
    W = (torch.randn(E, N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
    packed, st = F.quantize_4bit(W, blocksize=BS, quant_type="nf4")
    del W
    return packed, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="first T of every shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_ffn_bench.txt"),
                    help="the table is also written to this file, replacing it ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per block / per launch: median (min ... max) of {args.rounds} rounds; NF4, blocksize {BS}, plain statistics, bf16; "
        "x is [T, H], routing weights fp32")
    say(f"{'shape':>44s} {'T':>2s} {'S':>2s} {'fused block':>24s} {'parent block':>24s} {'saved':>7s} {'ratio':>6s} "
        f"{'gated launch':>24s} {'plain launch':>24s} {'gated-plain':>11s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for label, E, I, H, S, Ts in SHAPES:
        per_block = (2 * I * H + H * I) // 2 + (2 * I * H + H * I) // BS * 4     # one expert's bytes of both stacks
        L = max(2, min(48, math.ceil(1.25 * CACHE_BYTES / (min(S, E) * per_block))))
        stacks = [quantized(E, 2 * I, H, gen) + quantized(E, H, I, gen) for _ in range(L)]
        calls = L * math.ceil(64 / L)
        for T in (Ts[:1] if args.quick else Ts):
            x = torch.randn(T, H, device="cuda", generator=gen).bfloat16()
            ids = torch.stack([torch.randperm(E, device="cuda", generator=gen)[:S] for _ in range(T)]).to(torch.int32)
            w = torch.softmax(torch.randn(T, S, device="cuda", generator=gen), dim=-1)

            def fused():
                for c in range(calls):
                    gu, gs, dn, ds = stacks[c % L]
                    bnb.moe_ffn_4bit(x, gu, gs, dn, ds, ids, w)

            def parent():
                for c in range(calls):
                    gu, gs, dn, ds = stacks[c % L]
                    g, u = bnb.matmul_4bit_experts(x, gu, gs, ids).chunk(2, dim=-1)
                    y = bnb.matmul_4bit_experts(TF.silu(g) * u, dn, ds, ids)
                    (y * w.unsqueeze(-1).to(y.dtype)).sum(dim=1)

            def gated():
                for c in range(calls):
                    gu, gs, _, _ = stacks[c % L]
                    bnb.matmul_4bit_experts(x, gu, gs, ids, gated="chunked")

            def plain():
                for c in range(calls):
                    gu, gs, _, _ = stacks[c % L]
                    bnb.matmul_4bit_experts(x, gu, gs, ids)

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
            say(f"{label:>44s} {T:>2d} {S:>2d} {cols[0]:>24s} {cols[1]:>24s} {med[1] - med[0]:7.2f} {med[1] / med[0]:5.2f}x "
                f"{cols[2]:>24s} {cols[3]:>24s} {med[2] - med[3]:+11.2f}")
            del graphs
        del stacks
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
