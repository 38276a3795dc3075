#!/usr/bin/env python3
"""A 4-bit base layer with a LoRA adapter beside it on one GPU, us per layer of a decode step: the adapter term as the epilogue of the
base layer's launch (bitsandbytes_amd.matmul_4bit_lora) against the same layer from the operations the library offered before it;
and the LoRA launch against the plain launch on the same matrix.

Method (tools/bench_ffn.py): every leg is a hipGraph of >= 64 layers that rotate over enough distinct layers that the weights of one
pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms); the legs alternate
inside one process, order reversed every round; median and min ... max of the rounds. Legs:
  fused    t = F.linear(x, A); matmul_4bit_lora(x, W, t, B_l, s)                                2 launches
  addmm    y = matmul_4bit(x, W); t = F.linear(x, A); torch.addmm(y, t, B_l.t(), alpha=s)       3 launches
  peft     matmul_4bit(x, W) + F.linear(F.linear(x, A), B_l) * s                                5 launches
  plain    matmul_4bit(x, W) alone
  lora     the LoRA launch alone (t computed outside the graph)
`ahead` = addmm - fused; `spread` = the larger min ... max range of the two; the fused launch may serve a class only where `ahead`
exceeds `spread` in every cell of the class. The table is written to profiles/lora_bench.txt (--out), replacing the file.
    python tools/bench_lora.py [--rounds 5] [--quick] [--out profiles/lora_bench.txt]"""
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

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]  # N x K
RANKS = (16, 64, 128)
MS = (1, 2, 4, 8, 16)
SCALING = 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, r = 16, M = 1 and 4 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.txt"),
                    help="the table is also written to this file, replacing it ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per layer / per launch: median (min...max) of {args.rounds} rounds; NF4, blocksize {BS}, bf16, no bias, scaling {SCALING}; x is [M, K]")
    say(f"{'N x K':>13s} {'stats':>6s} {'r':>3s} {'M':>2s} {'served':>6s} {'fused':>21s} {'addmm parent':>21s} {'peft parent':>21s} "
        f"{'plain launch':>21s} {'lora launch':>21s} {'ahead':>6s} {'spread':>6s} {'lora-plain':>10s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    from bitsandbytes_amd.backends import hip

    with torch.no_grad():
        for N, K in (SHAPES[:1] if args.quick else SHAPES):
            for nested in (False, True):
                per_layer = N * K // 2 + N * K // BS * (1 if nested else 4)
                L = max(2, min(48, math.ceil(1.25 * CACHE_BYTES / per_layer)))
                layers = []
                for _ in range(L):
                    W = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
                    layers.append(bnb.functional.quantize_4bit(W, blocksize=BS, quant_type="nf4", compress_statistics=nested))
                    del W
                calls = L * math.ceil(64 / L)
                for r in (RANKS[:1] if args.quick else RANKS):
                    As = [(torch.randn(r, K, device="cuda", generator=gen) / K ** 0.5).bfloat16() for _ in range(L)]
                    Bs = [(torch.randn(N, r, device="cuda", generator=gen) * 0.5).bfloat16() for _ in range(L)]
                    for M in ((1, 4) if args.quick else MS):
                        x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
                        ts = [TF.linear(x, A) for A in As]
                        served = hip.gemm_4bit_lora_supported(torch.bfloat16, M, N, K, BS, nested, r)

                        def fused():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit_lora(x, w, st, TF.linear(x, As[c % L]), Bs[c % L], SCALING)

                        def addmm():
                            for c in range(calls):
                                w, st = layers[c % L]
                                y = bnb.matmul_4bit(x, w, st)
                                torch.addmm(y, TF.linear(x, As[c % L]), Bs[c % L].t(), alpha=SCALING)

                        def peft():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit(x, w, st) + TF.linear(TF.linear(x, As[c % L]), Bs[c % L]) * SCALING

                        def plain():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit(x, w, st)

                        def lora():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit_lora(x, w, st, ts[c % L], Bs[c % L], SCALING)

                        legs = [fused, addmm, peft, plain, lora]
                        graphs = [capture(fn) for fn in legs]
                        samples = [[] for _ in legs]
                        reps = [max(2, int(10000.0 / (timed(g, calls, 1) * calls)) + 1) for g in graphs]
                        for rnd in range(args.rounds):
                            order = range(len(legs)) if rnd % 2 == 0 else reversed(range(len(legs)))
                            for i in order:
                                samples[i].append(timed(graphs[i], calls, reps[i]))
                        cols = [f"{statistics.median(s):7.2f} ({min(s):.2f}...{max(s):.2f})" for s in samples]
                        med = [statistics.median(s) for s in samples]
                        spread = max(max(samples[0]) - min(samples[0]), max(samples[1]) - min(samples[1]))
                        say(f"{f'{N} x {K}':>13s} {'nested' if nested else 'plain':>6s} {r:>3d} {M:>2d} {int(served):>6d} {cols[0]:>21s} {cols[1]:>21s} "
                            f"{cols[2]:>21s} {cols[3]:>21s} {cols[4]:>21s} {med[1] - med[0]:6.2f} {spread:6.2f} {med[4] - med[3]:+10.2f}")
                        del graphs
                    del As, Bs
                del layers
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
