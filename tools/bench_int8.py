#!/usr/bin/env python3
"""LLM.int8() inference (csrc/int8_quant.hip, csrc/gemm_int8.hip, nn.Linear8bitLt), us per call, against yardsticks in the same process.

Method (tools/bench_moe_ffn.py): every leg is a hipGraph of >= 64 calls that rotate over enough distinct weights that one pass over the
rotation exceeds the 256 MiB Infinity Cache; HIP events around `reps` replays (regions >= 10 ms); the legs alternate inside one process,
order reversed every round; median and min ... max of the rounds - read the spread first. Legs, x bf16 [M, K]:
  quant      int8_vectorwise_quant(x)                                                         1 launch
  scaled_mm  int8_scaled_mm(q, CB, stats, SCB, dtype=bf16): the matmul with the dequant epilogue 1 launch, by the route as shipped
  mm 6000    the same call under bnb_mi355x_set_tuning(0, 0, 0, 6000): gemm_int8_kernel forced (the parent's only kernel)
  mm 6100    the same call under 6100: gemm_int8_tall_kernel forced, its built-in tile choice
  layer      Linear8bitLt(x), threshold 0                                                     2 launches
  bf16       F.linear(x, W) on the dequantized weight (hipBLASLt)
  4bit       this package's Linear4bit (NF4, bf16) at the same shape
  _int_mm    torch._int_mm(q, CB.t()) and the torch dequantization expression, where this torch build runs it ('raises' otherwise)
For M <= 16 the scaled_mm column also gives the achieved bytes/s over bench.HBM_PEAK_GBS; the bound there is the N * K weight bytes.
For M >= 128 the 'mm 6100' column also gives 2 M N K operations / time over the int8 MFMA peak at the clock the device reports: CUs x 4 SIMDs x
1024 operations a cycle (v_mfma_i32_16x16x64_i8: 32768 operations in 8 passes of 4 cycles) x torch's clock_rate.
--mixed prints the threshold-6 table instead (mixed_table below: the sync-free mixed decomposition against the composed ops).
    python tools/bench_int8.py [--rounds 5] [--quick] [--out profiles/int8_bench.txt]
    python tools/bench_int8.py --mixed [--rounds 5] [--quick] [--out profiles/int8_mixed_bench.txt]"""
import argparse
import copy
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
from bench import HBM_PEAK_GBS  # noqa: E402
from tools.bench_experts import CACHE_BYTES, capture, timed  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]  # (N, K)
MS = (1, 4, 16, 64, 128, 256, 512, 2048)
OPS = torch.ops.bitsandbytes
MIXED_OUTLIER_COLS = 8  # --mixed: columns of x that hold a value above the threshold


class Eager:
    """What `timed` replays for a leg that cannot be captured: the calls themselves, host time included."""

    def __init__(self, fn):
        self.replay = fn


def mixed_table(args, say):
    """--mixed: Linear8bitLt at threshold 6 (the mixed decomposition), x bf16 [M, K] with MIXED_OUTLIER_COLS columns that hold one value
    of 8.0 each (the other values are randn: none reaches 6 in practice) - the handful of outlier feature dimensions of a real model.
      layer t0   Linear8bitLt(x), threshold 0: 2 launches, in the tool's graphs (the yardstick: the same matmul without the outlier term)
      layer t6   Linear8bitLt(x), threshold 6: quantize with the mask (3 launches, 2 at M = 1), int8_scaled_mm, int8_outlier_addmm_ -
                 in the tool's graphs, nothing read on the host
      composed   int8_vectorwise_quant(x, 6.0) then int8_mixed_scaled_mm: the path of the parent commit. It synchronises (the number of
                 outlier columns sizes a tensor) and cannot be captured: timed EAGERLY with events around the same rotation of calls, so
                 its figure INCLUDES the host time of about a dozen launches and one device-to-host round trip per call."""
    say(f"# us per call: median (min ... max) of {args.rounds} rounds; x bf16 with {MIXED_OUTLIER_COLS} outlier columns; 'layer' legs in graphs, "
        "'composed' eager (host time included)")
    names = ["layer t0", "layer t6", "composed t6 (eager)"]
    say(f"{'N x K':>13s} {'M':>5s} " + " ".join(f"{n:>28s}" for n in names) + f" {'t6/t0':>7s} {'composed/t6':>11s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for N, K in SHAPES:
        L = max(2, math.ceil(1.25 * CACHE_BYTES / (N * K)))
        calls = L * math.ceil(64 / L)
        layers, layers6 = [], []
        for _ in range(L):
            l8 = bnb.nn.Linear8bitLt(K, N, bias=False)
            l8.weight = bnb.nn.Int8Params((torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).cpu())
            layers.append(l8.to("cuda"))
            l6 = copy.copy(layers[-1])  # (the same parameters)
            l6.threshold = 6.0
            layers6.append(l6)
        for M in (MS[:1] if args.quick else MS):
            x = torch.randn(M, K, device="cuda", generator=gen).clamp(-5.5, 5.5)
            x[torch.arange(MIXED_OUTLIER_COLS) % M, torch.arange(MIXED_OUTLIER_COLS) * (K // MIXED_OUTLIER_COLS) + 3] = 8.0
            x = x.bfloat16()

            def layer_t0():
                for c in range(calls):
                    layers[c % L](x)

            def layer_t6():
                for c in range(calls):
                    layers6[c % L](x)

            def composed_t6():
                for c in range(calls):
                    w = layers[c % L].weight
                    q, stats, cols = OPS.int8_vectorwise_quant.default(x, 6.0)
                    OPS.int8_mixed_scaled_mm.default(x, q, w.CB, stats, w.SCB, cols, None)

            composed_t6()
            torch.cuda.synchronize()
            legs = [capture(layer_t0), capture(layer_t6), Eager(composed_t6)]
            reps = [max(2, int(10000.0 / (timed(g, calls, 1) * calls)) + 1) for g in legs]
            samples = [[] for _ in legs]
            for r in range(args.rounds):
                for i in (range(len(legs)) if r % 2 == 0 else reversed(range(len(legs)))):
                    samples[i].append(timed(legs[i], calls, reps[i]))
            med = [statistics.median(s) for s in samples]
            cols = [f"{m:9.2f} ({min(s):.2f}...{max(s):.2f})" for m, s in zip(med, samples)]
            say(f"{f'{N} x {K}':>13s} {M:>5d} " + " ".join(f"{c:>28s}" for c in cols) + f" {med[1] / med[0]:6.2f}x {med[2] / med[1]:10.2f}x")
            del legs
        del layers, layers6
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="first M of every shape only")
    ap.add_argument("--mixed", action="store_true", help="the threshold-6 table (mixed_table) instead, to profiles/int8_mixed_bench.txt")
    ap.add_argument("--out", default=None, help="the table is also written here ('' for none; default profiles/int8_bench.txt)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "int8_mixed_bench.txt" if args.mixed else "int8_bench.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    if args.mixed:
        mixed_table(args, say)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    say(f"# us per call: median (min ... max) of {args.rounds} rounds; x bf16; %HBM = N * K bytes / time / {HBM_PEAK_GBS:.0f} GB/s (M <= 16)")
    props = torch.cuda.get_device_properties(0)
    khz = ct.c_int(0)  # hipDeviceAttributeClockRate (5): the peak engine clock the runtime reports, kHz
    if ct.CDLL("libamdhip64.so").hipDeviceGetAttribute(ct.byref(khz), 5, torch.cuda.current_device()) != 0:
        raise RuntimeError("hipDeviceGetAttribute(hipDeviceAttributeClockRate) failed")
    khz = khz.value
    peak_ops = props.multi_processor_count * 4 * 1024 * khz * 1e3  # int8 operations / s
    say(f"# %MFMA = 2 M N K / time of 'mm 6100' / ({props.multi_processor_count} CUs x 4 SIMDs x 1024 ops/cycle x {khz / 1e3:.0f} MHz reported = {peak_ops / 1e15:.3f} Pop/s)")
    names = ["quant", "scaled_mm", "mm 6000", "mm 6100", "layer", "bf16 F.linear", "Linear4bit", "_int_mm+dequant"]
    say(f"{'N x K':>13s} {'M':>5s} " + " ".join(f"{n:>26s}" for n in names) + f" {'%HBM':>6s} {'%MFMA':>6s} {'kernel':>6s} {'bf16/layer':>10s} {'4bit/layer':>10s} {'_int_mm/scaled_mm':>17s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for N, K in SHAPES:
        L = max(2, math.ceil(1.25 * CACHE_BYTES / (N * K)))
        calls = L * math.ceil(64 / L)
        layers, dense, four = [], [], []
        for _ in range(L):
            W = torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5
            l8 = bnb.nn.Linear8bitLt(K, N, bias=False)
            l8.weight = bnb.nn.Int8Params(W.cpu())
            layers.append(l8.to("cuda"))
            dense.append(OPS.int8_vectorwise_dequant.default(layers[-1].weight.CB, layers[-1].weight.SCB).bfloat16())
            l4 = bnb.nn.Linear4bit(K, N, bias=False, quant_type="nf4", compute_dtype=torch.bfloat16)
            l4.weight = bnb.nn.Params4bit(W.bfloat16().cpu(), requires_grad=False, quant_type="nf4", module=l4)
            four.append(l4.to("cuda"))
        for M in (MS[:1] if args.quick else MS):
            x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
            q, stats, _ = OPS.int8_vectorwise_quant.default(x, 0.0)

            def quant():
                for c in range(calls):
                    OPS.int8_vectorwise_quant.default(x, 0.0)

            def scaled_mm(value=0):
                bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, value)  # (the route is host logic: what is captured is what it chose)
                try:
                    for c in range(calls):
                        w = layers[c % L].weight
                        OPS.int8_scaled_mm.default(q, w.CB, stats, w.SCB, None, torch.bfloat16)
                finally:
                    bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, 0)

            def mm_6000():
                scaled_mm(6000)

            def mm_6100():
                scaled_mm(6100)

            def layer():
                for c in range(calls):
                    layers[c % L](x)

            def bf16():
                for c in range(calls):
                    TF.linear(x, dense[c % L])

            def fourbit():
                for c in range(calls):
                    four[c % L](x)

            def int_mm():
                for c in range(calls):
                    w = layers[c % L].weight
                    (torch._int_mm(q, w.CB.t()) * (stats[:, None] * w.SCB[None, :]) * 6.200124e-05).bfloat16()

            legs = [quant, scaled_mm, mm_6000, mm_6100, layer, bf16, fourbit, int_mm]
            graphs = []
            for fn in legs:
                try:
                    graphs.append(capture(fn))
                except Exception as exc:  # (torch._int_mm refuses small M on this build)
                    graphs.append(None)
                    say(f"#   {N} x {K}, M = {M}: {fn.__name__} raises {type(exc).__name__}: {str(exc).splitlines()[0][:120]}")
                    torch.cuda.synchronize()
            live = [i for i, g in enumerate(graphs) if g is not None]
            samples = {i: [] for i in live}
            reps = {i: max(2, int(10000.0 / (timed(graphs[i], calls, 1) * calls)) + 1) for i in live}
            for r in range(args.rounds):
                for i in (live if r % 2 == 0 else live[::-1]):
                    samples[i].append(timed(graphs[i], calls, reps[i]))
            med = {i: statistics.median(s) for i, s in samples.items()}
            cols = [f"{med[i]:9.2f} ({min(samples[i]):.2f}...{max(samples[i]):.2f})" if i in med else "raises" for i in range(len(legs))]
            hbm = f"{100.0 * N * K / med[1] / 1e3 / HBM_PEAK_GBS:5.1f}%" if M <= 16 else ""
            mfma = f"{100.0 * 2.0 * M * N * K / (med[3] * 1e-6) / peak_ops:5.1f}%" if M >= 128 and peak_ops > 0 else ""
            vs = f"{med[7] / med[1]:16.2f}x" if 7 in med else f"{'n/a':>17s}"
            say(f"{f'{N} x {K}':>13s} {M:>5d} " + " ".join(f"{c:>26s}" for c in cols) + f" {hbm:>6s} {mfma:>6s} {bnb.lib.bnb_mi355x_gemm_int8_route(M, N, K):>6d} "
                f"{med[5] / med[4]:9.2f}x {med[6] / med[4]:9.2f}x {vs}")
            del graphs
        del layers, dense, four
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
