#!/usr/bin/env python3
"""The coverage bound on bench.py's default workload (10M x 2,504 synthetic, seed 0; --rows shrinks the variant axis), k = 100,
T = 200, one process, one GPU:

  (a) utm_coverage_bound over every sample: HIP-event time of the whole call and host wall time, warmed up once and
      repeated; on a second context with UTM_FLAG_PROFILE_EVENTS the summed times of k_bound_sums, k_bound_pick and
      k_bound_update, per iteration, and pick + update as a share of the iteration.  (Events around every launch cost
      launch overlap: the per-kernel figures come from that context, the call time from the plain one.)
  (b) utm_stream_calibration of the same process, and k_bound_sums's bytes per second (the candidate columns, once per
      iteration; the multipliers it re-reads per sample group are not counted) as a share of it;
  (c) on the same matrix: greedy's captured at k, the three bounds of `select --bound-out` and the share they certify.

Prints one JSON object and writes it to --out.  Nothing is gated: the figures are reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from utmos_amd import _native, bound, device  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000, help="variants of the synthetic matrix")
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("-k", type=int, default=100)
    p.add_argument("-T", "--iters", type=int, default=200)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    n_var, n, k, T = args.rows, args.n_samp, args.k, args.iters
    wp = max(128, ((n_var + 63) // 64 + 127) // 128 * 128)
    out = {"workload": f"synthetic {n_var} x {n}", "seed": args.seed, "k": k, "iters": T, "env_overrides": _native.env_overrides()}
    column_bytes = n * wp * 8
    with device.DeviceMatrix(n) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=args.seed)
        ms, wall = [], []
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            res = m.coverage_bound(k, iters=T)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(res.pass_ms)
        out["a_call"] = {"launches_ms": spread(ms), "wall_ms": spread(wall), "ms_per_iteration": statistics.median(ms) / T,
                         "bound": res.bound, "best_iter": res.best_iter, "n_live": res.n_live, "trivial": int(res.hist[0] // bound.Q)}
        out["stream_calibration_gbps"] = m.stream_calibration(20)
        # (c) the panel the bound is for, and the three bounds as `select --bound-out` writes them
        m.reset()
        order = m.run(k)[0]
        row = bound.bound_rows(m, order, [len(order)], np.arange(n), (), T)[0]
        out["c_quality"] = dict(zip(("k", "captured", "bound_trivial", "bound_online", "bound_lagrange", "bound", "share"), row))
    with device.DeviceMatrix(n, profile_events=True) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=args.seed)
        kernels = []
        for rep in range(args.repeats + 1):
            timed = m.coverage_bound(k, iters=T)
            if rep:
                kernels.append(m.coverage_bound_times())
        assert timed.hist.tolist() == res.hist.tolist()
        sums, pick, update = (statistics.median(x[i] for x in kernels) / T for i in range(3))
        out["a_kernels_ms_per_iteration"] = {"k_bound_sums": sums, "k_bound_pick": pick, "k_bound_update": update,
                                             "pick_and_update_share_of_iteration": (pick + update) / (sums + pick + update)}
        out["b_sums"] = {"column_bytes": column_bytes, "gbps": column_bytes / (sums * 1e-3) / 1e9}
        out["b_sums"]["share_of_stream_calibration"] = out["b_sums"]["gbps"] / out["stream_calibration_gbps"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
