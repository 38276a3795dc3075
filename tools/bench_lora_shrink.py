#!/usr/bin/env python3
"""The LoRA shrink matmul t = x @ lora_A^T as a kernel of this library (bitsandbytes_amd.lora_shrink, csrc/lora_shrink.hip) against the
F.linear it replaces, us per layer of a decode step: in front of the LoRA launch of a 4-bit base layer, alone, and for a stacked group.

Method (tools/bench_lora.py): every leg is a hipGraph of >= 64 layers that rotate over enough distinct layers that the weights of one
pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms); the legs alternate
inside one process, order reversed every round; median and min ... max of the rounds. Legs:
  linear   t = F.linear(x, A); matmul_4bit_lora(x, W, t, B_l, s)          2 launches - the yardstick (bench_lora.py's `fused` leg)
  shrink   t = lora_shrink(x, A); matmul_4bit_lora(x, W, t, B_l, s)       2 launches, both of this library
  F.linear / lora_shrink alone: the same rotation of adapters without the base layer (the adapters stay cache-resident)
`ahead` = linear - shrink; `spread` = the larger min ... max range of the two; bnb_mi355x_lora_shrink_supported may answer 1 for a
class only where `ahead` exceeds `spread` in every measured cell of the class (`win`). The kernel is launched through the C entry
point, which does not consult the predicate, so that excluded classes are measured too; `served` is the predicate's answer.
Group legs (K = 4096, three members of rank r that share x - Q/K/V), us per group, every part contiguous as gemm_4bit_lora wants it:
  3 x linear   three F.linear                                               3 launches
  stacked      one F.linear on the stacked [3 r, K] + three .contiguous()   4 launches
  splits       one lora_shrink(x, stacked, splits=(r, r, r))                1 launch
The table is written to profiles/lora_shrink_bench.txt (--out), replacing the file.
    python tools/bench_lora_shrink.py [--rounds 5] [--quick] [--out profiles/lora_shrink_bench.txt]"""
import argparse
import ctypes as ct
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
from tools.bench_lora import MS, RANKS, SCALING, SHAPES  # noqa: E402

GROUP_K = 4096


def shrink(x, A, splits=None):
    """bnb_mi355x_lora_shrink on the current stream, whatever the predicate says; the flat output buffer."""
    M, K = x.shape
    out = torch.empty(M * A.shape[0], dtype=x.dtype, device=x.device)
    n = 0 if splits is None else len(splits)
    bnb.lib.bnb_mi355x_lora_shrink(2, x.data_ptr(), A.data_ptr(), out.data_ptr(), M, A.shape[0], K, (ct.c_int * n)(*splits) if n else None, n,
                                   torch.cuda.current_stream().cuda_stream)
    return out


def measure(legs, calls, rounds):
    graphs = [capture(fn) for fn in legs]
    samples = [[] for _ in legs]
    reps = [max(2, int(10000.0 / (timed(g, calls, 1) * calls)) + 1) for g in graphs]
    for rnd in range(rounds):
        order = range(len(legs)) if rnd % 2 == 0 else reversed(range(len(legs)))
        for i in order:
            samples[i].append(timed(graphs[i], calls, reps[i]))
    del graphs
    return samples


def col(s):
    return f"{statistics.median(s):7.2f} ({min(s):.2f}...{max(s):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, plain statistics, r = 16, M = 1 and 4 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_shrink_bench.txt"),
                    help="the table is also written to this file, replacing it ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from bitsandbytes_amd.backends import hip

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per layer / per launch: median (min...max) of {args.rounds} rounds; NF4, blocksize {BS}, bf16, no bias, scaling {SCALING}; x is [M, K]")
    say(f"{'N x K':>13s} {'stats':>6s} {'r':>3s} {'M':>2s} {'served':>6s} {'linear':>21s} {'shrink':>21s} {'F.linear alone':>21s} "
        f"{'lora_shrink alone':>21s} {'ahead':>6s} {'spread':>6s} {'win':>3s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    ranks = RANKS[:1] if args.quick else RANKS
    ms = (1, 4) if args.quick else MS
    with torch.no_grad():
        for N, K in (SHAPES[:1] if args.quick else SHAPES):
            for nested in ((False,) if args.quick else (False, True)):
                per_layer = N * K // 2 + N * K // BS * (1 if nested else 4)
                L = max(2, min(48, math.ceil(1.25 * CACHE_BYTES / per_layer)))
                layers = []
                for _ in range(L):
                    W = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
                    layers.append(bnb.functional.quantize_4bit(W, blocksize=BS, quant_type="nf4", compress_statistics=nested))
                    del W
                calls = L * math.ceil(64 / L)
                for r in ranks:
                    As = [(torch.randn(r, K, device="cuda", generator=gen) / K ** 0.5).bfloat16() for _ in range(L)]
                    Bs = [(torch.randn(N, r, device="cuda", generator=gen) * 0.5).bfloat16() for _ in range(L)]
                    for M in ms:
                        x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
                        served = hip.lora_shrink_supported(torch.bfloat16, M, r, K)

                        def linear():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit_lora(x, w, st, TF.linear(x, As[c % L]), Bs[c % L], SCALING)

                        def shrunk():
                            for c in range(calls):
                                w, st = layers[c % L]
                                bnb.matmul_4bit_lora(x, w, st, shrink(x, As[c % L]).view(M, r), Bs[c % L], SCALING)

                        def linear_alone():
                            for c in range(calls):
                                TF.linear(x, As[c % L])

                        def shrink_alone():
                            for c in range(calls):
                                shrink(x, As[c % L])

                        s = measure([linear, shrunk, linear_alone, shrink_alone], calls, args.rounds)
                        ahead = statistics.median(s[0]) - statistics.median(s[1])
                        spread = max(max(s[0]) - min(s[0]), max(s[1]) - min(s[1]))
                        say(f"{f'{N} x {K}':>13s} {'nested' if nested else 'plain':>6s} {r:>3d} {M:>2d} {int(served):>6d} {col(s[0]):>21s} {col(s[1]):>21s} "
                            f"{col(s[2]):>21s} {col(s[3]):>21s} {ahead:6.2f} {spread:6.2f} {int(ahead > spread):>3d}")
                    del As, Bs
                del layers
                torch.cuda.empty_cache()
        say()
        say(f"# group of three rank-r members that share x, K = {GROUP_K}: us per group, median (min...max)")
        say(f"{'r':>3s} {'M':>2s} {'served':>6s} {'3 x linear':>21s} {'stacked + 3 copies':>21s} {'splits':>21s} {'ahead':>6s} {'spread':>6s} {'win':>3s}")
        K, L, calls = GROUP_K, 16, 64
        for r in ranks:
            stacks = [(torch.randn(3 * r, K, device="cuda", generator=gen) / K ** 0.5).bfloat16() for _ in range(L)]
            members = [[a[i * r:(i + 1) * r].contiguous() for i in range(3)] for a in stacks]
            for M in ms:
                x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
                served = hip.lora_shrink_supported(torch.bfloat16, M, 3 * r, K)

                def three():
                    for c in range(calls):
                        for a in members[c % L]:
                            TF.linear(x, a)

                def stacked():
                    for c in range(calls):
                        for p in TF.linear(x, stacks[c % L]).split(r, dim=-1):
                            p.contiguous()

                def splits():
                    for c in range(calls):
                        shrink(x, stacks[c % L], (r, r, r))

                s = measure([three, stacked, splits], calls, args.rounds)
                best = min((0, 1), key=lambda i: statistics.median(s[i]))
                ahead = statistics.median(s[best]) - statistics.median(s[2])
                spread = max(max(s[best]) - min(s[best]), max(s[2]) - min(s[2]))
                say(f"{r:>3d} {M:>2d} {int(served):>6d} {col(s[0]):>21s} {col(s[1]):>21s} {col(s[2]):>21s} {ahead:6.2f} {spread:6.2f} {int(ahead > spread):>3d}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
