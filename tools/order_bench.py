#!/usr/bin/env python3
"""Fixed orders on bench.py's default workload (10M x 2,504 synthetic), one process, one GPU:

  (a) utm_apply_order of all 2,504 samples: HIP-event time of the pass (utm_stats.loop_ms), as GB/s of n * wp * 8 bytes,
      beside utm_stream_calibration of the same context;
  (b) the curve of the first 64 samples by the per-sample route (utm_set_sample_state + utm_step for every position:
      the earlier ones used, the next one the only selectable sample) against one utm_apply_order of those 64 -- host
      wall time around calls that end in a device synchronise, and the gains compared;
  (c) a select-all greedy run (utm_stats.loop_ms) for scale.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from utmos_amd import device  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def per_sample_route(m, order):
    """What the ABI offered before utm_apply_order: one reset (re-ORs every used column) and one step per position."""
    n_samp, gains = m.n_samples, []
    for i, s in enumerate(order):
        state = np.full(n_samp, 2, np.uint8)
        state[order[:i]] = 0
        state[s] = 1
        m.set_state(state)
        row = m.step()
        gains.append(0 if row is None else row[1])
    return gains


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--prefix", type=int, default=64)
    p.add_argument("--no-greedy", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed}
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = (args.n_var + 63) // 64
        wp = (wp + 127) // 128 * 128
        order = np.random.default_rng(args.seed).permutation(args.n_samp)
        ones = np.ones(args.n_samp, np.uint8)

        # (a) the whole order in one pass
        ms, gains_all = [], None
        for rep in range(args.repeats + 1):
            m.set_state(ones)
            m.reset()
            gains_all = m.apply_order(order)
            if rep:
                ms.append(m.stats()["loop_ms"])
        n_done = len(gains_all)
        bytes_pass = args.n_samp * wp * 8          # every listed column is streamed, also behind the row that ends the rows
        out["a_apply_order_all"] = {"rows": n_done, "listed": args.n_samp, "pass_ms": spread(ms),
                                    "gbps": bytes_pass / (statistics.median(ms) * 1e-3) / 1e9,
                                    "stream_calibration_gbps": m.stream_calibration(20)}
        out["a_apply_order_all"]["fraction_of_stream"] = out["a_apply_order_all"]["gbps"] / out["a_apply_order_all"]["stream_calibration_gbps"]

        # (b) the first `prefix` samples: per-sample route against one call
        head = order[:args.prefix]
        slow, fast, fast_ms = [], [], []
        gains_slow = gains_fast = None
        for rep in range(3):
            t0 = time.perf_counter()
            gains_slow = per_sample_route(m, head)
            if rep:
                slow.append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            m.set_state(ones)
            m.reset()
            t0 = time.perf_counter()
            gains_fast = m.apply_order(head).tolist()
            if rep:
                fast.append((time.perf_counter() - t0) * 1e3)
                fast_ms.append(m.stats()["loop_ms"])
        out["b_first_samples"] = {"samples": int(args.prefix), "per_sample_route_wall_ms": spread(slow),
                                  "apply_order_wall_ms": spread(fast), "apply_order_pass_ms": spread(fast_ms),
                                  "gains_equal": gains_slow == gains_fast,
                                  "speedup_wall": statistics.median(slow) / statistics.median(fast)}

        # (c) greedy select-all, for scale
        if not args.no_greedy:
            loop = []
            for rep in range(2):
                m.set_state(ones)
                m.reset()
                rows = len(m.run(args.n_samp)[0])
                if rep:
                    loop.append(m.stats()["loop_ms"])
            out["c_greedy_select_all"] = {"rows": rows, "loop_ms": spread(loop)}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not out["b_first_samples"]["gains_equal"] or out["b_first_samples"]["speedup_wall"] <= 1:
        sys.exit("the one-pass call has to equal the per-sample route and be faster")


if __name__ == "__main__":
    main()
