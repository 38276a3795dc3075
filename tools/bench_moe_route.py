#!/usr/bin/env python3
"""The MoE router - bitsandbytes_amd.moe_route: logits from lora_shrink, then ONE launch of csrc/moe_route.hip - against the torch
composition a caller writes today, us per router of a decode step, eager and under graph replay.

Legs (x [T, K] bf16, router weight [E, K] bf16, S slots):
  torch    F.linear; softmax(dtype=float) or sigmoid (+ select_bias); topk; (gather;) sum; div; (* scale;) ids to int32   7 ... 10 launches
  route    moe_route(x, W, S, ...)                                                                                      2 launches
  torch top-k / moe_topk alone: the same without the matmul, on logits that are already there
softmax legs renormalize with scale 1 (Mixtral / Qwen); sigmoid legs add a selection bias, renormalize and scale by 2.5 (DeepSeek-V3 /
GLM without group limits).

Method (tools/bench_lora_shrink.py): a graph leg is a hipGraph of 64 routers that rotate over 16 distinct router weights (a router's
weight is small: the rotation stays cache-resident for every leg alike); HIP events around `reps` replays (regions >= 10 ms); the
legs alternate inside one process, order reversed every round; median and min ... max of the rounds. An eager leg is the host clock
around 200 calls that end in a device synchronise, the same alternation. `ahead` = torch - route under graph replay; `spread` = the
larger min ... max range of the two; bnb_mi355x_moe_topk_supported may answer 1 for a class only where the launch did not measure
behind the composition: `ok` = the route leg's median is not above the torch leg's by more than `spread`.
Behind the table: the max relative error of the kernel's weights and of torch's fp32 composition against float64 on the cases of
tests/moe_route_cases.py - the two figures tests/test_gpu_moe_route.py compares. Table and figures go to profiles/moe_route.txt
(--out), replacing the file up to its "# ---- notes" line; what follows that line is kept.
    python tools/bench_moe_route.py [--rounds 5] [--quick] [--out profiles/moe_route.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bitsandbytes_amd as bnb  # noqa: E402
from tools.bench_lora_shrink import col, measure  # noqa: E402

# (E, K, S); K = 2880 is 45 * 64
SHAPES = ((8, 4096, 2), (128, 2048, 8), (128, 2880, 4), (256, 7168, 8))
TS = (1, 4, 16)
SCORINGS = ("softmax", "sigmoid")
SCALE = 2.5
LAYERS, CALLS, EAGER_CALLS = 16, 64, 200
NOTES_MARK = "# ---- notes"


def torch_topk(logits, S, scoring, sb):
    """What a model's router does with its logits today."""
    if scoring == "softmax":
        p = torch.softmax(logits, dim=-1, dtype=torch.float)
        w, ids = torch.topk(p, S, dim=-1)
        w = w / w.sum(dim=-1, keepdim=True)
    else:
        p = logits.float().sigmoid()
        ids = torch.topk(p + sb, S, dim=-1).indices
        w = p.gather(-1, ids)
        w = w / w.sum(dim=-1, keepdim=True) * SCALE
    return ids.to(torch.int32), w


def lib_topk(logits, S, scoring, sb):
    if scoring == "softmax":
        return bnb.moe_topk(logits, S)
    return bnb.moe_topk(logits, S, "sigmoid", True, SCALE, sb)


def lib_route(x, W, S, scoring, sb):
    if scoring == "softmax":
        return bnb.moe_route(x, W, S)
    return bnb.moe_route(x, W, S, scoring="sigmoid", renormalize=True, scale=SCALE, select_bias=sb)


def weight_errors():
    """(kernel, torch fp32 composition, cases): max relative error of the weights against float64 over the test cases."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import moe_route_cases as C
    from bitsandbytes_amd.autograd._functions import _moe_topk_composition

    kernel = composed = 0.0
    for case in C.CASES:
        b = C.build(case)
        logits, bias = b.logits.cuda(), None if b.bias is None else b.bias.cuda()
        w = torch.ops.bitsandbytes_amd.moe_topk.default(logits, case.S, case.scoring, case.renormalize, case.scale, bias)[1]
        cw = _moe_topk_composition(logits, case.S, case.scoring, case.renormalize, case.scale, bias)[1]
        kernel, composed = max(kernel, C.max_rel_err(w, b.weights)), max(composed, C.max_rel_err(cw, b.weights))
    return kernel, composed, len(C.CASES)


def eager(legs, rounds):
    """us per call of every leg: the host clock around EAGER_CALLS calls and a synchronise, legs alternating."""
    samples = [[] for _ in legs]
    for fn in legs:
        fn()
    torch.cuda.synchronize()
    for rnd in range(rounds):
        order = range(len(legs)) if rnd % 2 == 0 else reversed(range(len(legs)))
        for i in order:
            t0 = time.perf_counter()
            for _ in range(EAGER_CALLS // CALLS + 1):
                legs[i]()
            torch.cuda.synchronize()
            samples[i].append((time.perf_counter() - t0) * 1e6 / ((EAGER_CALLS // CALLS + 1) * CALLS))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the first shape, T = 1 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_route.txt"),
                    help="the table is also written to this file, replacing it up to its '# ---- notes' line ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from bitsandbytes_amd.backends import hip

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per router: median (min...max) of {args.rounds} rounds; bf16 x and router weight; graph legs: {CALLS} routers per graph over "
        f"{LAYERS} weights; eager legs: host clock, {EAGER_CALLS}+ calls per sample")
    say(f"{'E x K, S':>16s} {'scoring':>7s} {'T':>2s} {'served':>6s} {'shrink':>6s} {'graph torch':>21s} {'graph route':>21s} {'graph torch top-k':>21s} "
        f"{'graph moe_topk':>21s} {'ahead':>6s} {'spread':>6s} {'ok':>2s} {'eager torch':>21s} {'eager route':>21s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for E, K, S in (SHAPES[:1] if args.quick else SHAPES):
            Ws = [(torch.randn(E, K, device="cuda", generator=gen) / K ** 0.5).bfloat16() for _ in range(LAYERS)]
            sb = (torch.randn(E, device="cuda", generator=gen) * 0.1).float()
            for scoring in SCORINGS:
                for T in (TS[:1] if args.quick else TS):
                    x = torch.randn(T, K, device="cuda", generator=gen).bfloat16()
                    logits = [TF.linear(x, W) for W in Ws]
                    served = hip.moe_topk_supported(torch.bfloat16, T, E, S)
                    shrink = hip.lora_shrink_supported(torch.bfloat16, T, E, K)

                    def torch_leg():
                        for c in range(CALLS):
                            torch_topk(TF.linear(x, Ws[c % LAYERS]), S, scoring, sb)

                    def route_leg():
                        for c in range(CALLS):
                            lib_route(x, Ws[c % LAYERS], S, scoring, sb)

                    def torch_topk_leg():
                        for c in range(CALLS):
                            torch_topk(logits[c % LAYERS], S, scoring, sb)

                    def moe_topk_leg():
                        for c in range(CALLS):
                            lib_topk(logits[c % LAYERS], S, scoring, sb)

                    g = measure([torch_leg, route_leg, torch_topk_leg, moe_topk_leg], CALLS, args.rounds)
                    e = eager([torch_leg, route_leg], args.rounds)
                    ahead = statistics.median(g[0]) - statistics.median(g[1])
                    spread = max(max(g[0]) - min(g[0]), max(g[1]) - min(g[1]))
                    say(f"{f'{E} x {K}, {S}':>16s} {scoring:>7s} {T:>2d} {int(served):>6d} {int(shrink):>6d} {col(g[0]):>21s} {col(g[1]):>21s} "
                        f"{col(g[2]):>21s} {col(g[3]):>21s} {ahead:6.2f} {spread:6.2f} {int(ahead > -spread):>2d} {col(e[0]):>21s} {col(e[1]):>21s}")
            del Ws
        say()
        kernel, composed, count = weight_errors()
        say(f"# weights against float64 on the {count} cases of tests/moe_route_cases.py (what tests/test_gpu_moe_route.py bounds), max relative error:")
        say(f"#   moe_topk kernel {kernel:.3e}   torch fp32 composition on this GPU {composed:.3e}   "
            f"bound max(4 x composition, 2^-20) = {max(4 * composed, 2.0 ** -20):.3e}")
    if args.out:
        notes = []
        if os.path.exists(args.out):   # what follows NOTES_MARK is written by hand (results of other tools) and kept
            old = open(args.out).read().split("\n")
            notes = old[old.index(NOTES_MARK):] if NOTES_MARK in old else []
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines + [""] + notes).rstrip("\n") + "\n")


if __name__ == "__main__":
    main()
