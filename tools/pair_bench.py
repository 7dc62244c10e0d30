#!/usr/bin/env python3
"""Pair counts on bench.py's default workload (10M x 2,504 synthetic), one process, one GPU:

  (a) ONE utm_pair_counts call over all samples: the whole n x n matrix -- HIP-event time of its launches and host wall
      time of the call; also with a `given` panel of the greedy first 100, and with the non-temporal loads forced on and
      off (UTM_NT_LOADS, read at utm_reset);
  (b) the route the ABI offered before, per sample s: utm_set_sample_state (s used) + utm_reset + utm_peek_scores;
      shared[s][t] = var_count[t] - count[t].  Host wall time of the first 8 samples, scaled to all;
  (c) ONE utm_swap_gains(k = 100) in the same process: the same and + popcount arithmetic with the row operand read from
      global memory, for its pair-words per second.  Reported, not gated.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The two
gates: the rows of (b) equal the rows of (a), and the wall time of (a) is below (b) scaled to all samples.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from utmos_amd import _native, device  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def sample_route(m, var_count, samples):
    """shared[s] for the samples `samples` by one reset and one full scoring pass each."""
    rows = []
    for s in samples:
        state = np.ones(m.n_samples, np.uint8)
        state[s] = 0
        m.set_state(state)
        m.reset()
        rows.append(var_count - m.peek_scores()[0])
    m.set_state(np.ones(m.n_samples, np.uint8))
    m.reset()
    return np.asarray(rows)


def timed_pairs(m, indices, given, repeats):
    ms, wall = [], []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        one = m.pair_counts(indices, given, pass_ms=True)[1]
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(one)
    return ms, wall


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("-k", type=int, default=100, help="size of the `given` panel and of the swap-gains panel")
    p.add_argument("--route-samples", type=int, default=8)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    n = args.n_samp
    out = {"workload": f"synthetic {args.n_var} x {n}", "seed": args.seed, "k": args.k, "env_overrides": _native.env_overrides()}
    with device.DeviceMatrix(n) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((args.n_var + 63) // 64 + 127) // 128 * 128
        m.reset()
        panel = m.run(args.k)[0]
        assert len(panel) == args.k
        m.reset()
        var_count = m.var_count()
        everyone = np.arange(n)
        out["pair_words"] = int(n * (n + 1) // 2 * wp)

        # gate 1: equal answers
        head = list(range(min(args.route_samples, n)))
        shared = m.pair_counts(everyone)
        slow = sample_route(m, var_count, head)
        mask = np.ones((len(head), n), bool)
        mask[head, head] = False                                         # (a used sample's own score is masked to 0)
        out["rows_equal_on_first_samples"] = bool((shared[head][mask] == slow[mask]).all() and (np.diagonal(shared) == var_count).all())
        out["shared_sum"], out["shared_max_off_diagonal"] = int(shared.sum()), int((shared - np.diag(np.diagonal(shared))).max())

        ms, wall = timed_pairs(m, everyone, (), args.repeats)
        out["a_pair_counts"] = {"launches_ms": spread(ms), "wall_ms": spread(wall),
                                "pair_words_per_s": out["pair_words"] / (statistics.median(ms) * 1e-3)}
        ms_g, wall_g = timed_pairs(m, everyone, panel, args.repeats)
        out["a_pair_counts_given"] = {"launches_ms": spread(ms_g), "wall_ms": spread(wall_g),
                                      "pair_words_per_s": out["pair_words"] / (statistics.median(ms_g) * 1e-3)}
        for nt in ("0", "1"):                                            # the load form, forced either way (the rule picks one)
            os.environ["UTM_NT_LOADS"] = nt
            m.reset()
            forced = timed_pairs(m, everyone, (), max(1, args.repeats - 1))[0]
            out["a_nt_loads_" + nt] = {"launches_ms": spread(forced)}
        del os.environ["UTM_NT_LOADS"]
        m.reset()

        slow_wall = []
        for rep in range(3):
            t0 = time.perf_counter()
            sample_route(m, var_count, head)
            if rep:
                slow_wall.append((time.perf_counter() - t0) * 1e3)
        per_sample = statistics.median(slow_wall) / len(head)
        out["b_sample_route"] = {"wall_ms_first_samples": spread(slow_wall), "per_sample_ms": per_sample, "scaled_wall_ms": per_sample * n}
        out["speedup_wall"] = per_sample * n / statistics.median(wall)

        swap_ms = []
        for rep in range(args.repeats + 1):
            one = m.swap_gains(panel, pass_ms=True)[4]
            if rep:
                swap_ms.append(one)
        swap_words = int((args.k + 1) * (n + 1) * wp)
        out["c_swap_gains"] = {"launches_ms": spread(swap_ms), "pair_words": swap_words,
                               "pair_words_per_s": swap_words / (statistics.median(swap_ms) * 1e-3)}
        out["pair_words_rate_ratio"] = out["a_pair_counts"]["pair_words_per_s"] / out["c_swap_gains"]["pair_words_per_s"]
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not out["rows_equal_on_first_samples"] or out["speedup_wall"] <= 1:
        sys.exit("the one call has to equal the per-sample route and be faster than it scaled to all samples")


if __name__ == "__main__":
    main()
