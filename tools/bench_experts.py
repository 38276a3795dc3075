#!/usr/bin/env python3
"""The expert-indexed fused matmul (bitsandbytes_amd.matmul_4bit_experts, csrc/gemm4_experts.hip) against what the library offered
before it, us per call of one expert projection of a decode step.

Method (the dense bench's): every leg is a hipGraph of >= 64 calls that rotate over enough distinct expert stacks that the weights
selected by one pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms);
the legs alternate inside one process, order reversed every round; median and min ... max of the rounds. Legs:
  experts   one matmul_4bit_experts call (ids on the device, never read by the host);
  separate  (a) the same pairs as separate gemm_4bit M = 1 calls on the expert slices, the ids known to the host IN ADVANCE (which
            needs a device-to-host synchronisation per layer that is not timed here);
  dequant   (b) the parametrization path: dequantize_4bit of the whole stack, indexed matmul.
bytes per call = (distinct selected experts) x (N K / 2 + absmax bytes); the fraction is of 8.0 TB/s.
    python tools/bench_experts.py [--rounds 5] [--quick] [--out profiles/experts_bench.txt]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bitsandbytes_amd as bnb  # noqa: E402
import bitsandbytes_amd.functional as F  # noqa: E402

HBM_TBS = 8.0
CACHE_BYTES = 256 << 20
BS = 64
# (label, E, N, K, S, T values)
SHAPES = [
    ("Mixtral gate/up 8 x 14336 x 4096", 8, 14336, 4096, 2, (1, 4, 16)),
    ("Mixtral down 8 x 4096 x 14336", 8, 4096, 14336, 2, (1, 4, 16)),
    ("128 x 768 x 2048", 128, 768, 2048, 8, (1, 4, 8)),
    ("128 x 2048 x 768", 128, 2048, 768, 8, (1, 4, 8)),
]


def capture(fn):
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


def timed(g, calls, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * calls) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="first T of every shape only")
    ap.add_argument("--no-dequant", action="store_true", help="skip leg (b)")
    ap.add_argument("--out", default=None, help="also append the table to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per call: median (min ... max) of {args.rounds} rounds; NF4, blocksize {BS}, plain statistics, bf16; x is [T, K]")
    say(f"{'shape':>34s} {'T':>2s} {'S':>2s} {'distinct':>8s} {'MB/call':>8s} {'experts':>22s} {'separate (a)':>22s} {'dequant (b)':>24s} "
        f"{'TB/s':>5s} {'of 8.0':>6s} {'vs (a)':>6s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for label, E, N, K, S, Ts in SHAPES:
        per_expert = N * K // 2 + N * K // BS * 4
        # stacks in the rotation: sized for the call that selects the fewest experts
        L = max(2, min(48, math.ceil(1.25 * CACHE_BYTES / (min(S, E) * per_expert))))
        stacks = []
        for _ in range(L):
            W = (torch.randn(E, N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
            packed, st = F.quantize_4bit(W, blocksize=BS, quant_type="nf4")
            del W
            stacks.append((packed, st))
        calls = L * math.ceil(64 / L)
        for T in (Ts[:1] if args.quick else Ts):
            x = torch.randn(T, K, device="cuda", generator=gen).bfloat16()
            ids = torch.stack([torch.randperm(E, device="cuda", generator=gen)[:S] for _ in range(T)]).to(torch.int32)
            host_ids = ids.flatten().tolist()   # leg (a) only: the synchronisation the fused call does not need
            distinct = len(set(host_ids))
            nbytes = distinct * per_expert

            def fused():
                for c in range(calls):
                    packed, st = stacks[c % L]
                    bnb.matmul_4bit_experts(x, packed, st, ids)

            def separate():
                op = torch.ops.bitsandbytes.gemm_4bit.default
                for c in range(calls):
                    packed, st = stacks[c % L]
                    pk, am = packed.view(E, -1), st.absmax.view(E, -1)
                    for p, e in enumerate(host_ids):
                        op(x[p // S:p // S + 1], pk[e].reshape(-1, 1), [N, K], am[e], BS, "nf4")

            def dequant():
                for c in range(calls):
                    packed, st = stacks[c % L]
                    W = F.dequantize_4bit(packed, st)
                    torch.matmul(W[ids.long()], x[:, None, :, None])

            legs = [("experts", fused), ("separate", separate)] + ([] if args.no_dequant else [("dequant", dequant)])
            graphs = [capture(fn) for _, fn in legs]
            samples = [[] for _ in legs]
            reps = [max(2, int(10000.0 / (timed(g, calls, 1) * calls)) + 1) for g in graphs]
            for r in range(args.rounds):
                order = range(len(legs)) if r % 2 == 0 else reversed(range(len(legs)))
                for i in order:
                    samples[i].append(timed(graphs[i], calls, reps[i]))
            cols = [f"{statistics.median(s):8.2f} ({min(s):.2f}...{max(s):.2f})" for s in samples]
            if args.no_dequant:
                cols.append("-")
            t_new, t_a = statistics.median(samples[0]), statistics.median(samples[1])
            tbs = nbytes / t_new / 1e6
            say(f"{label:>34s} {T:>2d} {S:>2d} {distinct:>8d} {nbytes / 1e6:8.1f} {cols[0]:>22s} {cols[1]:>22s} {cols[2]:>24s} "
                f"{tbs:5.2f} {tbs / HBM_TBS:6.1%} {t_a / t_new:5.2f}x")
            del graphs
        del stacks
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
