#!/usr/bin/env python3
"""Class counts on bench.py's default workload (10M x 2,504 synthetic; --rows shrinks it), one process, one GPU:

  (a) utm_class_counts over every sample with class = the capture rank of a topN order (the samples by falling variant
      count) at k = 100 and at k = all samples, every mode: HIP-event time of the launch and host wall time of the call;
  (b) the same two class counts with half-dense random labels (uniform over the classes, half of the variants -1);
  (c) the route the ABI offered before, per position i of the order: utm_set_sample_state (rows 0..i used) + utm_reset +
      utm_peek_scores; captured[j] = var_count[j] - count[j].  Host wall time of the first 8 positions, scaled to k;
  (d) ONE utm_swap_gains(k = 100) in the same process: the rate of the dense and + popcount product that a class-mask
      formulation would need (n_classes x n x wp pair-words);
  (e) utm_stream_calibration: GB/s of plain streaming reads, for the ratio of a pass to one stream of the matrix.

Every leg is warmed up once and repeated; the spread is reported.  The first samples' rows are held against
tests/class_ref.py and route (c)'s counts against the cumulative table.  Prints one JSON object and writes it to
profiles/rNN_class_bench.json with the next free round number (or --out).  The gate: at both k the wall time of (a) is
below (c) scaled to k.
"""
import argparse
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import class_ref  # noqa: E402
from utmos_amd import _native, device  # noqa: E402

MODES = (1, 2)     # 0 picks one of them


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def next_profile():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(rounds, default=0) + 1:02d}_class_bench.json")


def timed_classes(m, labels, n_classes, mode, repeats):
    ms, wall, table = [], [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        table, one = m.class_counts([labels], n_classes, mode=mode, pass_ms=True)
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(one)
    return table, {"launch_ms": spread(ms), "wall_ms": spread(wall)}


def position_route(m, var_count, order, positions):
    """captured[i][j] after rows 0..i for the first `positions` rows, by one reset and one full scoring pass each."""
    rows = []
    for i in range(positions):
        state = np.ones(m.n_samples, np.uint8)
        state[order[:i + 1]] = 0
        m.set_state(state)
        m.reset()
        rows.append(var_count - m.peek_scores()[0])
    m.set_state(np.ones(m.n_samples, np.uint8))
    m.reset()
    return np.asarray(rows)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000, help="variants of the synthetic matrix")
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("-k", type=int, default=100, help="the short panel, and the swap-gains panel")
    p.add_argument("--route-positions", type=int, default=8)
    p.add_argument("--check-samples", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    n, n_var = args.n_samp, args.rows
    out = {"workload": f"synthetic {n_var} x {n}", "seed": args.seed, "env_overrides": _native.env_overrides()}
    rng = np.random.default_rng(args.seed)
    with device.DeviceMatrix(n) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((n_var + 63) // 64 + 127) // 128 * 128
        m.reset()
        var_count = m.var_count()
        order = np.argsort(-var_count, kind="stable")                    # topN: the first iteration's scores, best first
        out["matrix_bytes"], out["set_bits"] = int(n * wp * 8), int(var_count.sum())
        out["e_stream_gbps"] = m.stream_calibration()
        stream_ms = out["matrix_bytes"] / (out["e_stream_gbps"] * 1e9) * 1e3
        out["one_stream_of_the_matrix_ms"] = stream_ms
        head_cols = m.download_columns(c, 0, args.check_samples)
        positions = min(args.route_positions, n)
        ok = True
        for k in sorted({min(args.k, n), n}):
            rank = m.capture_rank(c, order[:k])
            labels = np.where(rank < 0, k, rank).astype(np.int32)
            random_labels = rng.integers(0, k + 1, size=n_var).astype(np.int32)
            random_labels[rng.random(n_var) < 0.5] = -1
            leg = {"n_classes": k + 1, "columns_per_workgroup": min(16, 16384 // (k + 1))}
            for name, lab in (("a_rank", labels), ("b_random", random_labels)):
                want = class_ref.class_counts(head_cols, lab, k + 1, None, n_var)
                for mode in MODES:
                    table, times = timed_classes(m, lab, k + 1, mode, args.repeats)
                    times["rows_equal_class_ref"] = bool((table[:args.check_samples] == want).all())
                    times["launch_over_one_stream"] = times["launch_ms"]["median"] / stream_ms
                    ok &= times["rows_equal_class_ref"]
                    leg[f"{name}_mode{mode}"] = times
                    if name == "a_rank" and mode == 1:
                        rank_table = table
            # (c) the route through the loop
            slow_wall, route = [], None
            for rep in range(3):
                t0 = time.perf_counter()
                route = position_route(m, var_count, order, min(positions, k))
                if rep:
                    slow_wall.append((time.perf_counter() - t0) * 1e3)
            per_position = statistics.median(slow_wall) / len(route)
            cum = np.cumsum(rank_table[:, :len(route)], axis=1).T         # [position][sample]
            free = np.ones((len(route), n), bool)
            for i in range(len(route)):
                free[i, order[:i + 1]] = False                           # (a used sample's own score is masked to 0)
            leg["route_equals_table_on_first_positions"] = bool((route[free] == cum[free]).all())
            ok &= leg["route_equals_table_on_first_positions"]
            leg["c_position_route"] = {"wall_ms_first_positions": spread(slow_wall), "per_position_ms": per_position,
                                       "scaled_wall_ms": per_position * k}
            best_wall = min(leg[f"a_rank_mode{mode}"]["wall_ms"]["median"] for mode in MODES)
            leg["speedup_wall_over_route"] = per_position * k / best_wall
            ok &= leg["speedup_wall_over_route"] > 1
            out[f"k{k}"] = leg

        panel = order[:min(args.k, n)]
        swap_ms = []
        for rep in range(args.repeats + 1):
            one = m.swap_gains(panel, pass_ms=True)[4]
            if rep:
                swap_ms.append(one)
        swap_words = int((len(panel) + 1) * (n + 1) * wp)
        rate = swap_words / (statistics.median(swap_ms) * 1e-3)
        out["d_swap_gains"] = {"launches_ms": spread(swap_ms), "pair_words": swap_words, "pair_words_per_s": rate}
        for k in sorted({min(args.k, n), n}):                            # the dense product over k + 1 class masks, at that rate
            out[f"k{k}"]["dense_product_ms_at_swap_rate"] = (k + 1) * n * wp / rate * 1e3
    out["ok"] = bool(ok)
    print(json.dumps(out))
    path = args.out or next_profile()
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        sys.exit("the table has to equal class_ref and the position route, and the one call has to be faster than the route scaled to k")


if __name__ == "__main__":
    main()
