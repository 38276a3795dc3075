#!/usr/bin/env python3
"""The fused 8-bit Adam update (csrc/optim8.hip), us per parameter tensor, against the composition available without it.

Method (tools/bench_int8.py): every leg is a hipGraph of calls that rotate over enough distinct parameter sets that one pass over
the rotation exceeds the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms); the legs alternate inside one
process, order reversed every round; median and min ... max of the rounds - read the spread first. Legs, Adam, weight decay 0.01:
  fused     optimizer_update_8bit_blockwise                                                      1 launch
  composed  dequantize_blockwise x 2, the update with torch elementwise ops in fp32, quantize_blockwise x 2, the copies back
%HBM of the fused leg = bytes per element (g, p read; p written; two codes read and written: 10 for bf16, 14 for fp32) * n / time
over bench.HBM_PEAK_GBS.
    python tools/bench_optim8.py [--rounds 5] [--out profiles/optim8_bench.txt]"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bitsandbytes_amd as bnb  # noqa: E402
import bitsandbytes_amd.functional as F  # noqa: E402
from bench import HBM_PEAK_GBS  # noqa: E402
from tools.bench_experts import CACHE_BYTES, capture, timed  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096)]
B1, B2, EPS, LR, WD, STEP = 0.9, 0.999, 1e-8, 1e-3, 0.01, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim8_bench.txt"), help="the table is also written here ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# Adam, us per tensor: median (min ... max) of {args.rounds} rounds; %HBM = 10 (bf16) / 14 (fp32) bytes * n / time / {HBM_PEAK_GBS:.0f} GB/s")
    say(f"{'shape':>13s} {'dtype':>8s} {'fused':>28s} {'composed':>28s} {'%HBM':>6s} {'composed/fused':>14s}")
    q1, q2 = F.create_dynamic_map(True).cuda(), F.create_dynamic_map(False).cuda()
    c1, c2 = 1.0 - B1 ** STEP, math.sqrt(1.0 - B2 ** STEP)
    for rows, cols in SHAPES:
        n = rows * cols
        for dtype, nbytes in ((torch.bfloat16, 10), (torch.float32, 14)):
            per_set = n * (2 * torch.finfo(dtype).bits // 8 + 2)
            L = max(2, math.ceil(1.25 * CACHE_BYTES / per_set))
            calls = L * math.ceil(8 / L)
            sets = []
            for _ in range(L):
                g, p = torch.randn(n, device="cuda").to(dtype), torch.randn(n, device="cuda").to(dtype)
                s1, st1 = F.quantize_blockwise(0.1 * torch.randn(n, device="cuda"), code=q1, blocksize=256)
                s2, st2 = F.quantize_blockwise(0.01 * torch.randn(n, device="cuda") ** 2, code=q2, blocksize=256)
                sets.append((g, p, s1, s2, st1.absmax, st2.absmax))
            torch.cuda.empty_cache()

            def fused():
                for c in range(calls):
                    g, p, s1, s2, a1, a2 = sets[c % L]
                    F.optimizer_update_8bit_blockwise("adam", g, p, s1, s2, B1, B2, 0.0, 0.0, EPS, STEP, LR, q1, q2, a1, a2, WD)

            def composed():
                for c in range(calls):
                    g, p, s1, s2, a1, a2 = sets[c % L]
                    m = F.dequantize_blockwise(s1, absmax=a1, code=q1, blocksize=256)
                    v = F.dequantize_blockwise(s2, absmax=a2, code=q2, blocksize=256)
                    g32, p32 = g.float(), p.float()
                    m.mul_(B1).add_(g32, alpha=1.0 - B1)
                    v.mul_(B2).addcmul_(g32, g32, value=1.0 - B2)
                    p32.mul_(1.0 - LR * WD).addcdiv_(m, (v.sqrt() / c2).add_(EPS), value=-LR / c1)
                    p.copy_(p32)
                    for state, absmax, code, new in ((s1, a1, q1, m), (s2, a2, q2, v)):
                        codes, qs = F.quantize_blockwise(new, code=code, blocksize=256)
                        state.copy_(codes)
                        absmax.copy_(qs.absmax)

            graphs = [capture(fused), capture(composed)]
            reps = [max(2, int(10000.0 / (timed(gr, calls, 1) * calls)) + 1) for gr in graphs]
            samples = [[], []]
            for r in range(args.rounds):
                for i in ((0, 1) if r % 2 == 0 else (1, 0)):
                    samples[i].append(timed(graphs[i], calls, reps[i]))
            med = [statistics.median(s) for s in samples]
            cols_ = [f"{med[i]:9.2f} ({min(samples[i]):.2f}...{max(samples[i]):.2f})" for i in range(2)]
            say(f"{f'{rows} x {cols}':>13s} {str(dtype).replace('torch.', ''):>8s} {cols_[0]:>28s} {cols_[1]:>28s} "
                f"{100.0 * nbytes * n / med[0] / 1e3 / HBM_PEAK_GBS:5.1f}% {med[1] / med[0]:13.2f}x")
            del graphs, sets
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
