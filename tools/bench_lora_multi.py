#!/usr/bin/env python3
"""Mixed-adapter LoRA decode - lora_shrink_ids + matmul_4bit_lora_ids, an adapter id per row (csrc/lora_shrink.hip's ids kernel, the
kLoraIds / IDS epilogues of csrc/gemv4_stream.hip and csrc/gemm4_mfma_sm.hip) - against the gathered torch composition it replaces and
against the uniform two launches with one adapter, us per layer of a decode step.

Method (tools/bench_lora.py, tools/bench_lora_shrink.py): every leg is a hipGraph of >= 64 layers that rotate over enough distinct
layers that the weights of one pass over the rotation exceed the 256 MiB Infinity Cache; HIP events around `reps` replays (regions
>= 10 ms); the legs alternate inside one process, order reversed every round; median and min ... max of the rounds. Every layer of the
rotation has its own stacks of A_N adapters. Legs of a layer:
  fused    t = lora_shrink_ids(x, A, ids); matmul_4bit_lora_ids(x, W, t, B, s, ids)          2 launches, ids on the device
  gather   matmul_4bit + bmm(A[ids], x) + bmm(B[ids], t) * s[ids] + add, rows without an adapter masked, all in the tensors' dtype:
           what a captured graph could do before (the cheapest form of the public functions' composition)
  uniform  t = lora_shrink(x, A[0]); matmul_4bit_lora(x, W, t, B[0], s[0])                   2 launches, ONE adapter: the floor
and the three shrinks alone (no base layer between them: the adapters stay cache-resident): ids / gather / uniform.
Id patterns: `same` (every row names adapter 1), `two` (two adapters interleaved), `distinct` (M different adapters).
`ahead` = gather - fused; `spread` = the larger min ... max range of the two; `over` = fused - uniform (what the ids cost over one
adapter); `s.ahead` / `s.spread`: the same for the shrinks alone. A predicate may exclude a class only where `ahead` does not exceed
`spread`. The shrink kernel is launched through the C entry point, which does not consult the predicate. `served`: the expand
predicate's answer (bnb_mi355x_gemm_4bit_lora_ids_supported = the uniform launch's); where it is 0 the base layer runs a kernel family
without a LoRA epilogue and BOTH the fused and the uniform leg run their public function's composition behind the shrink launch.
The table is written to profiles/lora_multi_bench.txt (--out), replacing the file.
    python tools/bench_lora_multi.py [--rounds 5] [--quick] [--out profiles/lora_multi_bench.txt]"""
import argparse
import ctypes as ct
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bitsandbytes_amd as bnb  # noqa: E402
from tools.bench_experts import BS, CACHE_BYTES  # noqa: E402
from tools.bench_lora import MS, RANKS, SHAPES  # noqa: E402
from tools.bench_lora_shrink import col, measure, shrink  # noqa: E402

A_N = 16  # adapters per stack (>= the largest batch: `distinct` names 16 of them)


def shrink_ids(x, stack, ids):
    """bnb_mi355x_lora_shrink_ids on the current stream, whatever the predicate says; [M, R]."""
    M, K = x.shape
    A_n, R, _ = stack.shape
    out = torch.empty(M, R, dtype=x.dtype, device=x.device)
    bnb.lib.bnb_mi355x_lora_shrink_ids(2, x.data_ptr(), stack.data_ptr(), ids.data_ptr(), ids.element_size(), out.data_ptr(), M, A_n, R, K, None, 0,
                                       torch.cuda.current_stream().cuda_stream)
    return out


def gather_shrink(x, stack, ids):
    """index_select + bmm, rows without an adapter masked; (t, valid, safe ids)."""
    A_n, R, K = stack.shape
    i64 = ids.to(torch.int64)
    valid = (i64 >= 0) & (i64 < A_n)
    safe = torch.where(valid, i64, torch.zeros_like(i64))
    t = torch.bmm(stack.index_select(0, safe), x.view(-1, K, 1)).view(-1, R)
    return torch.where(valid.view(-1, 1), t, torch.zeros_like(t)), valid, safe


def gather_layer(x, w, st, A, B, sc, ids):
    t, valid, safe = gather_shrink(x, A, ids)
    y = bnb.matmul_4bit(x, w, st)
    term = torch.bmm(B.index_select(0, safe), t.unsqueeze(2)).squeeze(2)
    return torch.where(valid.view(-1, 1), y + term * sc.index_select(0, safe).view(-1, 1).to(y.dtype), y)


def patterns(M):
    out = [("same", [1] * M)]
    if M > 1:
        out += [("two", [3 if m % 2 else 12 for m in range(M)]), ("distinct", [(5 * m + 2) % A_N for m in range(M)])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, plain statistics, r = 16, M = 1 and 4 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_multi_bench.txt"),
                    help="the table is also written to this file, replacing it ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from bitsandbytes_amd.backends import hip

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per layer / per launch: median (min...max) of {args.rounds} rounds; NF4, blocksize {BS}, bf16, no bias; x is [M, K]; stacks of "
        f"{A_N} adapters, scalings 0.5 ... 2, int32 ids")
    say(f"{'N x K':>13s} {'stats':>6s} {'r':>3s} {'M':>2s} {'ids':>8s} {'served':>6s} {'fused':>21s} {'gather':>21s} {'uniform':>21s} {'ahead':>6s} {'spread':>6s} {'win':>3s} "
        f"{'over':>6s} {'shrink: ids':>21s} {'shrink: gather':>21s} {'shrink: uniform':>21s} {'s.ahead':>7s} {'s.spread':>8s} {'s.win':>5s}")
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
                    As = [(torch.randn(A_N, r, K, device="cuda", generator=gen) / K ** 0.5).bfloat16() for _ in range(L)]
                    Bs = [(torch.randn(A_N, N, r, device="cuda", generator=gen) * 0.5).bfloat16() for _ in range(L)]
                    sc = torch.rand(A_N, device="cuda", generator=gen) * 1.5 + 0.5
                    s0 = float(sc[0])
                    A0s, B0s = [a[0].contiguous() for a in As], [b[0].contiguous() for b in Bs]
                    for M in ms:
                        x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
                        served = hip.gemm_4bit_lora_ids_supported(torch.bfloat16, M, N, K, BS, nested, r, A_N)
                        for name, vals in patterns(M):
                            ids = torch.tensor(vals, dtype=torch.int32, device="cuda")

                            def fused():
                                for c in range(calls):
                                    w, st = layers[c % L]
                                    bnb.matmul_4bit_lora_ids(x, w, st, shrink_ids(x, As[c % L], ids), Bs[c % L], sc, ids)

                            def gathered():
                                for c in range(calls):
                                    w, st = layers[c % L]
                                    gather_layer(x, w, st, As[c % L], Bs[c % L], sc, ids)

                            def uniform():
                                for c in range(calls):
                                    w, st = layers[c % L]
                                    bnb.matmul_4bit_lora(x, w, st, shrink(x, A0s[c % L]).view(M, r), B0s[c % L], s0)

                            def s_ids():
                                for c in range(calls):
                                    shrink_ids(x, As[c % L], ids)

                            def s_gather():
                                for c in range(calls):
                                    gather_shrink(x, As[c % L], ids)

                            def s_uniform():
                                for c in range(calls):
                                    shrink(x, A0s[c % L])

                            s = measure([fused, gathered, uniform, s_ids, s_gather, s_uniform], calls, args.rounds)
                            md = [statistics.median(v) for v in s]
                            ahead, over = md[1] - md[0], md[0] - md[2]
                            spread = max(max(s[0]) - min(s[0]), max(s[1]) - min(s[1]))
                            s_ahead = md[4] - md[3]
                            s_spread = max(max(s[3]) - min(s[3]), max(s[4]) - min(s[4]))
                            say(f"{f'{N} x {K}':>13s} {'nested' if nested else 'plain':>6s} {r:>3d} {M:>2d} {name:>8s} {int(served):>6d} " + " ".join(f"{col(v):>21s}" for v in s[:3])
                                + f" {ahead:6.2f} {spread:6.2f} {int(ahead > spread):>3d} {over:6.2f} " + " ".join(f"{col(v):>21s}" for v in s[3:])
                                + f" {s_ahead:7.2f} {s_spread:8.2f} {int(s_ahead > s_spread):>5d}")
                    del As, Bs, A0s, B0s
                del layers
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
