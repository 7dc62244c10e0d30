#!/usr/bin/env python3
"""Replicated selection on bench.py's default workload (10M x 2,504 synthetic, seed 0), B = 64 replicates of k = 100 rows over
hashed halves of the variants, one process, one GPU (--rows shrinks the variant axis):

  (a) ONE utm_multi_select call: HIP-event time of its launches and host wall time of the call;
  (b) the route there was before, for the first 4 replicates: a fresh matrix filled by the on-device generator (standing
      in for the reload from the host, which costs far more), utm_filter_variants(keep_b), utm_run(k) as `select` runs it
      (decremental scoring on).  Wall time with and without the refill, scaled to B replicates and labelled as scaled;
  (c) one utm_swap_gains(k) in the same process: the pair-words per second of the product k_multi_score is shaped after.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The one
gate: the rows of (a) and (b) are equal for those replicates.  The ratios are reported, not gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from utmos_amd import _native, device  # noqa: E402
from utmos_amd.stability import keep_threshold  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def host_mask(seed, rep, n_var, threshold):
    words = np.zeros((n_var + 63) // 64, dtype=np.uint64)
    _native.check(_native.lib().utm_multi_keep_host(seed, rep, 0, n_var, threshold, words.ctypes.data_as(ctypes.c_void_p)))
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_var].astype(bool)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000, help="variants of the synthetic matrix")
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("-B", "--replicates", type=int, default=64)
    p.add_argument("-k", type=int, default=100)
    p.add_argument("--fraction", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    n_var, n, B, k = args.rows, args.n_samp, args.replicates, args.k
    wp = max(128, ((n_var + 63) // 64 + 127) // 128 * 128)
    threshold = keep_threshold(args.fraction)
    out = {"workload": f"synthetic {n_var} x {n}", "seed": args.seed, "replicates": B, "k": k, "fraction": args.fraction,
           "env_overrides": _native.env_overrides()}
    states = np.ones(n, dtype=np.uint8)
    head = min(4, B)
    with device.DeviceMatrix(n) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=args.seed)
        ms, wall = [], []
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            order, new, kept, done, t = m.multi_select(k, states, seed=args.seed, fraction=args.fraction, n_rep=B, pass_ms=True)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(t)
        iterations = int(done.max())
        pair_words = B * n * wp * iterations
        out["a_multi_select"] = {"launches_ms": spread(ms), "wall_ms": spread(wall), "rows_min": int(done.min()), "rows_max": iterations,
                                 "kept_min": int(kept.min()), "kept_max": int(kept.max()), "pair_words": pair_words,
                                 "pair_words_per_s": pair_words / (statistics.median(ms) * 1e-3),
                                 "ms_per_iteration": statistics.median(ms) / max(iterations, 1)}
        # (c) the product it is shaped after, same process, same matrix
        m.reset()
        panel = m.run(k)[0]
        swap_ms = []
        for rep in range(args.repeats + 1):
            t = m.swap_gains(panel, pass_ms=True)[4]
            if rep:
                swap_ms.append(t)
        swap_words = (len(panel) + 1) * (n + 1) * wp
        out["c_swap_gains"] = {"launches_ms": spread(swap_ms), "pair_words": swap_words,
                               "pair_words_per_s": swap_words / (statistics.median(swap_ms) * 1e-3)}
        out["multi_over_swap_pair_word_rate"] = out["a_multi_select"]["pair_words_per_s"] / out["c_swap_gains"]["pair_words_per_s"]

    # (b) replicate by replicate: refill, filter, run
    equal, with_refill, without_refill = True, [], []
    for b in range(head):
        keep = host_mask(args.seed, b, n_var, threshold)
        for rep in range(2):                                          # the first pass of every replicate warms up
            t0 = time.perf_counter()
            with device.DeviceMatrix(n) as m:
                c = m.add_chunk(n_var)
                m.synth_fill(c, seed=args.seed)
                m.download_columns(c, 0, 1)                           # (a synchronising copy: the fill is done)
                t1 = time.perf_counter()
                got_kept = m.filter_variants(c, keep)
                m.set_decremental(True)
                m.set_state(states)
                idx, gains, _ = m.run(k)
                t2 = time.perf_counter()
            if rep:
                with_refill.append((t2 - t0) * 1e3)
                without_refill.append((t2 - t1) * 1e3)
        equal = equal and got_kept == kept[b] and len(idx) == done[b] and idx.tolist() == order[b, :done[b]].tolist() \
            and gains.tolist() == new[b, :done[b]].tolist()
    out["b_filter_and_run"] = {"replicates_timed": head, "rows_equal": bool(equal),
                               "wall_ms_per_replicate_with_refill": spread(with_refill),
                               "wall_ms_per_replicate_without_refill": spread(without_refill),
                               "wall_ms_scaled_to_B_with_refill": statistics.median(with_refill) * B,
                               "wall_ms_scaled_to_B_without_refill": statistics.median(without_refill) * B, "scaled_by": B}
    a_wall = out["a_multi_select"]["wall_ms"]["median"]
    out["speedup_over_scaled_route_with_refill"] = out["b_filter_and_run"]["wall_ms_scaled_to_B_with_refill"] / a_wall
    out["speedup_over_scaled_route_without_refill"] = out["b_filter_and_run"]["wall_ms_scaled_to_B_without_refill"] / a_wall
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not equal:
        sys.exit("the one call and the filter-and-run route have to give the same rows")


if __name__ == "__main__":
    main()
