#!/usr/bin/env python3
"""Capture ranks on bench.py's default workload (10M x 2,504 synthetic), one process, one GPU:

  (a) utm_capture_rank over all 2,504 samples at m = 1, 2 and 4: HIP-event time of the pass and GB/s of n * wp * 8 bytes,
      beside utm_stream_calibration of the same context and the utm_apply_order pass of the same list (the same reads
      with no scattered stores: the difference is what the stores cost);
  (b) the ranks of the first 64 positions by the route the ABI offered before: utm_set_sample_state + utm_step +
      utm_get_covered + a host diff per position, host wall time, against one utm_capture_rank of those 64.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The
one gate: (b)'s single call equals the per-position route and is faster.
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


def per_position_route(m, chunk, order, n_var):
    """One reset and one step per position, the covered mask downloaded after each, the new bits diffed on the host."""
    n_samp = m.n_samples
    rank = np.full(n_var, -1, np.int32)
    before = np.zeros((n_var + 63) // 64, np.uint64)
    for i, s in enumerate(order):
        state = np.full(n_samp, 2, np.uint8)
        state[order[:i]] = 0
        state[s] = 1
        m.set_state(state)
        m.step()
        after = m.covered(chunk)
        newly = np.unpackbits((after & ~before).view(np.uint8), bitorder="little")[:n_var]
        rank[newly.astype(bool)] = i
        before = after
    return rank


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--prefix", type=int, default=64)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed}
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((args.n_var + 63) // 64 + 127) // 128 * 128
        order = np.random.default_rng(args.seed).permutation(args.n_samp)
        ones = np.ones(args.n_samp, np.uint8)
        bytes_pass = args.n_samp * wp * 8
        out["stream_calibration_gbps"] = m.stream_calibration(20)

        # (a) the whole list in one pass, at three depths; the coverage curve's pass of the same list beside it
        legs = {}
        for depth in (1, 2, 4):
            ms, rank = [], None
            for rep in range(args.repeats + 1):
                rank, t = m.capture_rank(c, order, depth, pass_ms=True)
                if rep:
                    ms.append(t)
            legs[f"m{depth}"] = {"pass_ms": spread(ms), "gbps": bytes_pass / (statistics.median(ms) * 1e-3) / 1e9,
                                 "captured": int((rank >= 0).sum()), "stores_bytes": int((rank >= 0).sum()) * 4}
            legs[f"m{depth}"]["fraction_of_stream"] = legs[f"m{depth}"]["gbps"] / out["stream_calibration_gbps"]
        ms = []
        for rep in range(args.repeats + 1):
            m.set_state(ones)
            m.reset()
            gains = m.apply_order(order)
            if rep:
                ms.append(m.stats()["loop_ms"])
        legs["apply_order"] = {"pass_ms": spread(ms), "gbps": bytes_pass / (statistics.median(ms) * 1e-3) / 1e9, "rows": len(gains)}
        legs["stores_cost_ms_m1"] = legs["m1"]["pass_ms"]["median"] - legs["apply_order"]["pass_ms"]["median"]
        out["a_all_samples"] = legs

        # (b) the first `prefix` positions: the per-position route against one call
        head = order[:args.prefix]
        slow, fast, fast_ms = [], [], []
        rank_slow = rank_fast = None
        for rep in range(2):
            t0 = time.perf_counter()
            rank_slow = per_position_route(m, c, head, args.n_var)
            if rep:
                slow.append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            rank_fast, t = m.capture_rank(c, head, 1, pass_ms=True)
            if rep:
                fast.append((time.perf_counter() - t0) * 1e3)
                fast_ms.append(t)
        out["b_first_positions"] = {"positions": int(args.prefix), "per_position_route_wall_ms": spread(slow),
                                    "capture_rank_wall_ms": spread(fast), "capture_rank_pass_ms": spread(fast_ms),
                                    "ranks_equal": bool((rank_slow == rank_fast).all()),
                                    "speedup_wall": statistics.median(slow) / statistics.median(fast)}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not out["b_first_positions"]["ranks_equal"] or out["b_first_positions"]["speedup_wall"] <= 1:
        sys.exit("the one call has to equal the per-position route and be faster")


if __name__ == "__main__":
    main()
