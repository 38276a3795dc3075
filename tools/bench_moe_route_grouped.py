#!/usr/bin/env python3
"""Group-limited MoE routing - bitsandbytes_amd.moe_topk_grouped, ONE launch of csrc/moe_route.hip (moe_topk_grouped_kernel) - against
the torch code it replaces, us per router of a decode step under graph replay, on logits that are already there (the router matmul
in front is the same for every leg: tools/bench_moe_route.py measures it).

Legs (logits [T, E] bf16, S slots, n_group groups of which topk_group stay):
  model    what a model's own router does with its logits today: scores, the group scores (view, max or topk(2) + sum), topk over the
           groups, scatter to a mask, expand, masked_fill with -inf, topk, gather, sum, div, mul, ids to int32       ~15 launches
  compose  the library's own fall-back (_moe_topk_grouped_composition: the kernel's tie and NaN rules from stable sorts)
  kernel   torch.ops.bitsandbytes_amd.moe_topk_grouped                                                               1 launch
Geometries (E, n_group, topk_group, S): (160, 8, 3, 6) DeepSeek-V2 - softmax, "max", no renormalisation, scale 16 -; (256, 8, 4, 8)
DeepSeek-V3 - sigmoid, "top2sum", selection bias, renormalised, scale 2.5 -; (384, 1, 1, 8) one group - sigmoid, bias, renormalised:
the group stage is skipped, the model leg is a plain top-k. Two more rows stand at the limits of the launch: (1024, 16, 4, 16) - 16
register slots per lane, 16 rounds - and (128, 64, 16, 16) - 64 groups.

Method (tools/bench_lora_shrink.py): a graph leg is a hipGraph of 64 routers that rotate over 16 distinct logit tensors; HIP events
around `reps` replays (regions >= 10 ms); the legs alternate inside one process, order reversed every round; median and min ... max
of the rounds. `ahead` = min(model, compose) - kernel; `spread` = the largest min ... max range of the three;
bnb_mi355x_moe_topk_grouped_supported may answer 1 for a class only where the launch did not measure behind the code it replaces:
`ok` = the kernel's median is not above the faster torch leg's by more than `spread`.
Behind the table: the max relative error of the kernel's weights and of the fp32 composition against float64 on the cases of
tests/moe_route_grouped_cases.py - the two figures tests/test_gpu_moe_route_grouped.py compares. Table and figures go to
profiles/moe_route_grouped.txt (--out), replacing the file up to its "# ---- notes" line; what follows that line is kept.
    python tools/bench_moe_route_grouped.py [--rounds 5] [--quick] [--out profiles/moe_route_grouped.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bitsandbytes_amd as bnb  # noqa: E402
from bitsandbytes_amd.autograd._functions import _moe_topk_grouped_composition  # noqa: E402
from tools.bench_lora_shrink import col, measure  # noqa: E402

# (E, n_group, topk_group, S, scoring, group_score, renormalize, scale, select_bias)
GEOMETRIES = ((160, 8, 3, 6, "softmax", "max", False, 16.0, False), (256, 8, 4, 8, "sigmoid", "top2sum", True, 2.5, True),
              (384, 1, 1, 8, "sigmoid", "top2sum", True, 2.5, True),
              # the limits of the launch: 16 slots per lane and 16 rounds; 64 groups
              (1024, 16, 4, 16, "sigmoid", "top2sum", True, 2.5, True), (128, 64, 16, 16, "softmax", "max", True, 1.0, False))
TS = (1, 4, 16, 64)
LAYERS, CALLS = 16, 64
NOTES_MARK = "# ---- notes"


def model_router(logits, S, n_group, topk_group, scoring, group_score, renormalize, scale, sb):
    """The router of the DeepSeek-V2 / -V3 modelling code on its logits (dropped experts filled with -inf, no epsilon)."""
    p = torch.softmax(logits, dim=-1, dtype=torch.float) if scoring == "softmax" else logits.float().sigmoid()
    key = p if sb is None else p + sb
    if n_group > 1:
        T = key.shape[0]
        by_group = key.view(T, n_group, -1)
        group_key = by_group.max(dim=-1).values if group_score == "max" else by_group.topk(2, dim=-1)[0].sum(dim=-1)
        kept = torch.topk(group_key, topk_group, dim=-1, sorted=False)[1]
        mask = torch.zeros_like(group_key).scatter_(1, kept, 1)
        mask = mask.unsqueeze(-1).expand(T, n_group, by_group.shape[-1]).reshape(T, -1)
        key = key.masked_fill(~mask.bool(), float("-inf"))
    ids = torch.topk(key, S, dim=-1, sorted=True)[1]
    w = p.gather(-1, ids)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return ids.to(torch.int32), w * scale


def weight_errors():
    """(kernel, torch fp32 composition, cases): max relative error of the weights against float64 over the test cases."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import moe_route_cases as C
    import moe_route_grouped_cases as GC

    kernel = composed = 0.0
    for case in GC.CASES:
        b = GC.build(case)
        logits, bias = b.logits.cuda(), None if b.bias is None else b.bias.cuda()
        args = (logits, case.S, case.n_group, case.topk_group, case.group_score, case.scoring, case.renormalize, case.scale, bias)
        w = torch.ops.bitsandbytes_amd.moe_topk_grouped.default(*args)[1]
        cw = _moe_topk_grouped_composition(*args)[1]
        kernel, composed = max(kernel, C.max_rel_err(w, b.weights)), max(composed, C.max_rel_err(cw, b.weights))
    return kernel, composed, len(GC.CASES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the first geometry, T = 1 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_route_grouped.txt"),
                    help="the table is also written to this file, replacing it up to its '# ---- notes' line ('' for none)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from bitsandbytes_amd.backends import hip

    say(f"# {torch.cuda.get_device_name(0)}, {bnb.lib.bnb_mi355x_version().decode()}, torch {torch.__version__}")
    say(f"# us per router (scoring + group stage + top-k on logits that are there): median (min...max) of {args.rounds} rounds; bf16 logits; "
        f"graph legs: {CALLS} routers per graph over {LAYERS} logit tensors")
    say(f"{'E, groups, kept, S':>20s} {'scoring':>7s} {'group':>7s} {'T':>2s} {'served':>6s} {'graph model':>21s} {'graph compose':>21s} "
        f"{'graph kernel':>21s} {'ahead':>6s} {'spread':>6s} {'ok':>2s}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    behind = []
    with torch.no_grad():
        for E, n_group, topk_group, S, scoring, group_score, renormalize, scale, biased in (GEOMETRIES[:1] if args.quick else GEOMETRIES):
            sb = (torch.randn(E, device="cuda", generator=gen) * 0.1).float() if biased else None
            for T in (TS[:1] if args.quick else TS):
                logits = [torch.randn(T, E, device="cuda", generator=gen).bfloat16() for _ in range(LAYERS)]
                served = hip.moe_topk_grouped_supported(torch.bfloat16, T, E, S, n_group, topk_group, group_score)
                tail = (S, n_group, topk_group, scoring, group_score, renormalize, scale, sb)

                def model_leg():
                    for c in range(CALLS):
                        model_router(logits[c % LAYERS], *tail)

                def compose_leg():
                    for c in range(CALLS):
                        _moe_topk_grouped_composition(logits[c % LAYERS], S, n_group, topk_group, group_score, scoring, renormalize, scale, sb)

                def kernel_leg():
                    for c in range(CALLS):
                        torch.ops.bitsandbytes_amd.moe_topk_grouped.default(logits[c % LAYERS], S, n_group, topk_group, group_score, scoring,
                                                                            renormalize, scale, sb)

                g = measure([model_leg, compose_leg, kernel_leg], CALLS, args.rounds)
                ahead = min(statistics.median(g[0]), statistics.median(g[1])) - statistics.median(g[2])
                spread = max(max(s) - min(s) for s in g)
                ok = ahead > -spread
                if not ok:
                    behind.append((E, n_group, topk_group, S, T))
                say(f"{f'{E}, {n_group}, {topk_group}, {S}':>20s} {scoring:>7s} {group_score:>7s} {T:>2d} {int(served):>6d} {col(g[0]):>21s} "
                    f"{col(g[1]):>21s} {col(g[2]):>21s} {ahead:6.2f} {spread:6.2f} {int(ok):>2d}")
        say()
        say(f"# classes in which the kernel measured behind: {behind if behind else 'none'}")
        kernel, composed, count = weight_errors()
        say(f"# weights against float64 on the {count} cases of tests/moe_route_grouped_cases.py (what tests/test_gpu_moe_route_grouped.py "
            "bounds), max relative error:")
        say(f"#   moe_topk_grouped kernel {kernel:.3e}   torch fp32 composition on this GPU {composed:.3e}   "
            f"bound max(4 x composition, 2^-20) = {max(4 * composed, 2.0 ** -20):.3e}")
    if args.out:
        notes = []
        if os.path.exists(args.out):   # what follows NOTES_MARK is written by hand and kept
            old = open(args.out).read().split("\n")
            notes = old[old.index(NOTES_MARK):] if NOTES_MARK in old else []
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines + [""] + notes).rstrip("\n") + "\n")


if __name__ == "__main__":
    main()
