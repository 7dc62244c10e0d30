#!/usr/bin/env python3
"""k_score_list time by build phase, from one rocprofv3 kernel trace of select-all steps, set against the entry bytes of
each build (the JSON tools/list_shape_run.py prints for the same shape):

  python3 tools/list_phases.py <rocprofv3 output dir> <list_shape_run.json> [label]

The launch order is the iteration order: the first list launch of a step is the iteration of the first build.  Every step
in the trace (warm-up included) runs the same launches; the table gives the mean per step.  Bytes of a phase = launches x
4 x padded entries of its build: an upper bound, since a winner's segments are read no more."""
import csv
import glob
import json
import sys

import numpy as np


def main():
    trace = max(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True), key=lambda f: len(f))
    run = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    log, n_iter = run["list"]["log"], run["rows"]
    rows = []
    for r in csv.DictReader(open(trace)):
        if "k_score_list" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per_step = n_iter - log[0]["iter"]
    steps = len(rows) // per_step
    assert steps >= 1 and steps * per_step == len(rows), (len(rows), per_step)
    us = np.array([x[1] for x in rows], dtype=np.float64).reshape(steps, per_step) / 1e3
    names = [x[2] for x in rows[:per_step]]
    shape = run.get("shape") or [None] * len(log)
    print(f"# {label}: {steps} step(s) of {n_iter} iterations in the trace, per-step means; {len(rows)} k_score_list launches")
    print(f"{'iterations':>12s} {'kernel':>24s} {'lanes':>5s} {'wgs':>6s} {'T':>3s} {'tiles':>5s} {'launches':>8s} {'MB/iter':>8s} {'ms/step':>8s} "
          f"{'us mean':>8s} {'us min':>7s} {'us max':>7s} {'GB/s':>7s}")
    total = 0.0
    for k, b in enumerate(log):
        lo = b["iter"] - log[0]["iter"]
        hi = (log[k + 1]["iter"] if k + 1 < len(log) else n_iter) - log[0]["iter"]
        d = us[:, lo:hi]
        ms = d.sum() / steps / 1e3
        total += ms
        mb = b["padded"] * 4 / 1e6
        kern = names[lo].split("k_score_list")[1].split("(")[0]
        sh = shape[k] or {}
        print(f"{b['iter']:5d}-{(b['iter'] + hi - lo - 1):<6d} {('k_score_list' + kern):>24s} {str(sh.get('lanes', 64)):>5s} {str(sh.get('wgs', '-')):>6s} "
              f"{b['t']:3d} {b['tiles']:5d} {hi - lo:8d} {mb:8.1f} {ms:8.2f} {d.mean():8.1f} {d.min():7.1f} {d.max():7.1f} "
              f"{mb * 1e6 * (hi - lo) / (ms * 1e-3) / 1e9:7.0f}")
    print(f"# all k_score_list launches: {total:.2f} ms per step")


if __name__ == "__main__":
    main()
