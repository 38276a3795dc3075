#!/usr/bin/env python3
"""Census of the built-in gemm_4bit route on this device: for every case of the routed sweep (tests/exact_inputs.py: SWEEP_CASES),
which kernel family served which range of M through the public op, where the fused range ends, and whether each range was bit-equal
to the float64 reference. The same runner as tests/test_gpu_routed_sweep.py (tests/routed_sweep.py); a RECORD of what the route does
on this many CUs, not an assertion - the assertions are in that test.
    python tests/checks/routed_census.py [--out profiles/routed_census.txt] [--cases NAME ...]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_inputs as X  # noqa: E402
import routed_sweep as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = [f"routed census: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs; families: stream = gemv4_stream_kernel, sm / rt / pc / kq = "
             "the streaming / register-transposed / producer-consumer / K-quarter MFMA kernels; all ranges bit-equal to the float64 "
             "reference unless marked",
             ""]
    total, wrong, seconds = 0, 0, 0.0
    for i, case in enumerate(X.SWEEP_CASES):
        if a.cases and case.name not in a.cases:
            continue
        res = S.run_case(case, i)
        total += len(res.records)
        seconds += res.seconds
        bad = [r for r in res.records if r.mismatch is not None]
        wrong += len(bad)
        lines.append(f"{case.name:26s} blocksize {case.blocksize:4d} {str(case.dtype)[6:]:8s} {'nested' if case.nested else 'plain':6s} "
                     f"fused to {res.fused_max:4d} rows, {len(res.records)} calls, {res.seconds:.1f} s")
        lines.append("    " + S.family_ranges(res.records))
        for r in bad[:6]:
            lines.append(f"    WRONG {S.describe(case.name, r)}; largest relative error of a row {r.rel_rows:.3g}")
        print("\n".join(lines[-(2 + min(len(bad), 6)):]), flush=True)
    lines += ["", f"{total} calls, {wrong} not bit-equal, {seconds:.1f} s"]
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
