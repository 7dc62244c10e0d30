#!/usr/bin/env python3
"""Swap gains on bench.py's default workload (10M x 2,504 synthetic) for the greedy panel of k = 100, one process, one GPU:

  (a) ONE utm_swap_gains call: all k x n gains -- HIP-event time of its launches and host wall time of the call;
  (b) the route the ABI offered before, for the same answers: per panel member utm_set_sample_state (the other k - 1
      members used) + utm_reset + utm_peek_scores; gain[i][t] = count[t] - count[panel[i]].  Host wall time of all k.

Before anything is timed, (a) and (b) have to give equal gains on the panel's first 4 members.  Every leg is warmed up
once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The one gate: (a) equals (b)
and is faster.
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


def member_route(m, panel, members):
    """gains[i] for the positions `members` by one reset and one full scoring pass each."""
    rows = []
    for i in members:
        state = np.ones(m.n_samples, np.uint8)
        state[panel] = 0
        state[panel[i]] = 1
        m.set_state(state)
        m.reset()
        counts = m.peek_scores()[0]
        rows.append(counts - counts[panel[i]])
    return np.asarray(rows)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("-k", type=int, default=100)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed, "k": args.k,
           "env_overrides": _native.env_overrides()}
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((args.n_var + 63) // 64 + 127) // 128 * 128
        m.reset()
        panel = m.run(args.k)[0]
        assert len(panel) == args.k
        out["pair_words"] = int(args.k * args.n_samp * wp)

        # the gate's first half: equal answers
        head = list(range(min(4, args.k)))
        gains, unique, _, base = m.swap_gains(panel)
        slow = member_route(m, panel, head)
        out["gains_equal_on_first_members"] = bool((gains[head] == slow).all())
        out["base"], out["unique_sum"], out["best_gain"] = int(base), int(unique.sum()), int(gains.max())

        fast_ms, fast_wall = [], []
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            ms = m.swap_gains(panel, pass_ms=True)[4]
            if rep:
                fast_wall.append((time.perf_counter() - t0) * 1e3)
                fast_ms.append(ms)
        slow_wall = []
        for rep in range(3):
            t0 = time.perf_counter()
            member_route(m, panel, range(args.k))
            if rep:
                slow_wall.append((time.perf_counter() - t0) * 1e3)
        out["a_swap_gains"] = {"launches_ms": spread(fast_ms), "wall_ms": spread(fast_wall),
                               "pair_words_per_s": out["pair_words"] / (statistics.median(fast_ms) * 1e-3)}
        out["b_member_route"] = {"wall_ms": spread(slow_wall), "per_member_ms": statistics.median(slow_wall) / args.k}
        out["speedup_wall"] = statistics.median(slow_wall) / statistics.median(fast_wall)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not out["gains_equal_on_first_members"] or out["speedup_wall"] <= 1:
        sys.exit("the one call has to equal the per-member route and be faster")


if __name__ == "__main__":
    main()
