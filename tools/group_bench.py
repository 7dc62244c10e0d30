#!/usr/bin/env python3
"""Group curves on bench.py's default workload (10M x 2,504 synthetic, seed 0), 26 groups of near-equal size, one process,
one GPU, over (greedy) the greedy order of all samples (the samples greedy never takes appended by index) and (random) a
seeded random order:

  (a) utm_group_curve: HIP-event time of the whole call's launches with the private bins on and off and the head bins in
      LDS (bin_mode 1) and in global memory (2); k_group_unions alone (the call with an empty list launches nothing
      else), so k_group_curve = the call - the unions pass; beside utm_capture_rank at m = 1 over the same list in the
      same process -- the measured sibling that streams the same bytes -- and utm_stream_calibration of the same context;
  (b) the route the ABI offered before: utm_download_columns of every column, then an OR per group, the first carrier and
      a bincount on the host (at most 16 threads), over a PREFIX of the variants (a matrix of its own from the same seed),
      its wall time scaled to the full size and labelled as scaled, against one utm_group_curve over the same prefix.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The
gates: every leg of (a) gives the same bins, (b)'s two results are equal, and the call beats the scaled host route.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from utmos_amd import device  # noqa: E402

THREADS = 16


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def host_route(m, chunk, group_of, n_groups, order, n_var):
    """Download every column; per slice of the variant axis: OR per group, first carrier in the order, bincount."""
    words = (n_var + 63) // 64
    cols = m.download_columns(chunk)
    step = max(1, (words + 8 * THREADS - 1) // (8 * THREADS))
    n = len(order)

    def curve(lo):
        bits = np.unpackbits(np.ascontiguousarray(cols[:, lo:lo + step]).view(np.uint8), axis=1, bitorder="little").astype(bool)
        bits = bits[:, :max(0, min(bits.shape[1], n_var - lo * 64))]
        unions = np.stack([bits[group_of == g].any(axis=0) for g in range(n_groups)])
        private = unions & ~(unions.sum(axis=0) >= 2)
        listed = bits[order]
        rank = np.where(listed.any(axis=0), listed.argmax(axis=0), -1)
        new, priv = np.zeros((n_groups, n), np.int64), np.zeros((n_groups, n), np.int64)
        for g in range(n_groups):
            new[g] = np.bincount(rank[unions[g] & (rank >= 0)], minlength=n)
            priv[g] = np.bincount(rank[private[g] & (rank >= 0)], minlength=n)
        return new, priv, unions.sum(axis=1), private.sum(axis=1)

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(curve, range(0, words, step)))
    return tuple(sum(p[i] for p in parts) for i in range(4))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--groups", type=int, default=26)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--prefix", type=int, default=400_000)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed, "groups": args.groups}
    G = args.groups
    group_of = (np.arange(args.n_samp) * G // args.n_samp).astype(np.int32)     # near-equal contiguous blocks
    rng = np.random.default_rng(args.seed)
    ok = True
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((args.n_var + 63) // 64 + 127) // 128 * 128
        bytes_pass = args.n_samp * wp * 8
        out["stream_calibration_gbps"] = m.stream_calibration(20)
        m.set_decremental(True)
        m.reset()
        t0 = time.perf_counter()
        winners = m.run(args.n_samp)[0]
        out["greedy_rows"], out["greedy_wall_ms"] = len(winners), (time.perf_counter() - t0) * 1e3
        rest = np.setdiff1d(np.arange(args.n_samp), winners)
        orders = {"greedy": np.concatenate([winners, rest]).astype(np.int64), "random": rng.permutation(args.n_samp)}

        # k_group_unions alone: the call with an empty list (the same launch for every order)
        ms = []
        for rep in range(args.repeats + 1):
            t = m.group_curve(group_of, G, [], pass_ms=True)[-1]
            if rep:
                ms.append(t)
        unions_ms = statistics.median(ms)
        out["k_group_unions"] = {"pass_ms": spread(ms), "gbps": bytes_pass / (unions_ms * 1e-3) / 1e9,
                                 "fraction_of_stream_calibration": bytes_pass / (unions_ms * 1e-3) / 1e9 / out["stream_calibration_gbps"]}
        for label, order in orders.items():
            legs, base = {}, None
            ms = []
            for rep in range(args.repeats + 1):
                _, t = m.capture_rank(c, order, 1, pass_ms=True)
                if rep:
                    ms.append(t)
            rank_ms = statistics.median(ms)
            legs["capture_rank_m1"] = {"pass_ms": spread(ms), "gbps": bytes_pass / (rank_ms * 1e-3) / 1e9}
            for name, kw in (("private_lds", {"private": True, "bin_mode": 1}), ("private_global", {"private": True, "bin_mode": 2}),
                             ("plain_lds", {"private": False, "bin_mode": 1}), ("plain_global", {"private": False, "bin_mode": 2})):
                ms, got = [], None
                for rep in range(args.repeats + 1):
                    got = m.group_curve(group_of, G, order, pass_ms=True, **kw)
                    if rep:
                        ms.append(got[-1])
                call_ms = statistics.median(ms)
                curve_ms = call_ms - unions_ms
                legs[name] = {"call_ms": spread(ms), "k_group_curve_ms": curve_ms, "k_group_curve_gbps": bytes_pass / (curve_ms * 1e-3) / 1e9,
                              "k_group_curve_over_capture_rank": curve_ms / rank_ms, "captured_by_16": int(got[0][:, :16].sum()),
                              "captured": int(got[0].sum()), "total": int(got[2].sum())}
                base = got if base is None else base
                ok &= bool((got[0] == base[0]).all() and (got[2] == base[2]).all())
                if kw["private"]:
                    ok &= bool((got[1] == base[1]).all() and (got[3] == base[3]).all())
                ok &= bool((got[0].sum(axis=1) == got[2]).all())          # every sample grouped and listed
            out[label] = legs
        out["results_equal"] = ok

    # (b) the host route over a prefix of the variants, against one call over the same prefix
    prefix = min(args.prefix, args.n_var)
    order = orders["random"]
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(prefix)
        m.synth_fill(c, seed=args.seed)
        slow, fast, got_slow, got_fast = [], [], None, None
        for rep in range(2):
            t0 = time.perf_counter()
            got_slow = host_route(m, c, group_of, G, order, prefix)
            if rep:
                slow.append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            got_fast = m.group_curve(group_of, G, order)
            if rep:
                fast.append((time.perf_counter() - t0) * 1e3)
    with device.DeviceMatrix(args.n_samp) as m:                                  # the call's wall time at the full size
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        full = []
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            m.group_curve(group_of, G, order)
            if rep:
                full.append((time.perf_counter() - t0) * 1e3)
    scale = args.n_var / prefix
    equal = all(bool((a == b).all()) for a, b in zip(got_slow, got_fast))
    scaled = statistics.median(slow) * scale
    out["b_host_route"] = {"prefix_variants": prefix, "threads": THREADS, "host_route_wall_ms_prefix": spread(slow),
                           "host_route_wall_ms_scaled_to_full": scaled, "scaled_by": scale,
                           "group_curve_wall_ms_prefix": spread(fast), "group_curve_wall_ms_full": spread(full),
                           "speedup_full_call_over_scaled_host_route": scaled / statistics.median(full), "results_equal": equal}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not ok or not equal:
        sys.exit("the legs have to give the same bins, and the host route's have to equal the call's")
    if statistics.median(full) >= scaled:
        sys.exit("the call has to beat the scaled host route")


if __name__ == "__main__":
    main()
