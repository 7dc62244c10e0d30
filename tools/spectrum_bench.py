#!/usr/bin/env python3
"""Carrier counts on bench.py's default workload (10M x 2,504 synthetic), one process, one GPU:

  (a) utm_carrier_counts over all 2,504 samples: HIP-event time of the pass and GB/s of n * wp * 8 bytes, with and
      without the per-variant counts, with the decoded bins in LDS (hist_mode 1) and in global memory (2), and beyond a
      `given` panel of 100 samples; beside utm_capture_rank at m = 1 over the same list in the same process -- the
      measured sibling that streams the same bytes -- and utm_stream_calibration of the same context;
  (b) the route the ABI offered before: utm_download_columns of the listed columns and a count on the host (at most 16
      threads), over a PREFIX of the variants (a matrix of its own from the same seed), its wall time scaled to the full
      size and labelled as scaled, against one utm_carrier_counts over the same prefix.

Every leg is warmed up once and repeated; the spread is reported.  Prints one JSON object and writes it to --out.  The
gates: every leg of (a) gives the same histogram, and (b)'s two histograms are equal.
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


def host_route(m, chunk, order, n_var):
    """Download the listed columns, count the carriers of every variant on the host, bincount."""
    words = (n_var + 63) // 64
    cols = np.empty((len(order), words), np.uint64)
    for i, s in enumerate(order):                                       # (the list is not a range of columns)
        m.download_columns(chunk, int(s), 1, out=cols[i:i + 1])
    step = max(1, (words + 8 * THREADS - 1) // (8 * THREADS))

    def count(lo):
        bits = np.unpackbits(np.ascontiguousarray(cols[:, lo:lo + step]).view(np.uint8), axis=1, bitorder="little")
        return bits.sum(axis=0, dtype=np.int32)

    with ThreadPoolExecutor(THREADS) as pool:
        counts = np.concatenate(list(pool.map(count, range(0, words, step))))[:n_var]
    return np.bincount(counts, minlength=len(order) + 1).astype(np.int64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--given", type=int, default=100)
    p.add_argument("--prefix", type=int, default=400_000)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed}
    order = np.random.default_rng(args.seed).permutation(args.n_samp)
    ok = True
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        wp = ((args.n_var + 63) // 64 + 127) // 128 * 128
        bytes_pass = args.n_samp * wp * 8
        out["stream_calibration_gbps"] = m.stream_calibration(20)

        # (a) the whole list in one pass; the capture-rank pass of the same list beside it
        legs, base = {}, None
        ms = []
        for rep in range(args.repeats + 1):
            _, t = m.capture_rank(c, order, 1, pass_ms=True)
            if rep:
                ms.append(t)
        legs["capture_rank_m1"] = {"pass_ms": spread(ms), "gbps": bytes_pass / (statistics.median(ms) * 1e-3) / 1e9}
        for name, kw in (("hist_lds", {"hist_mode": 1}), ("hist_global", {"hist_mode": 2}),
                         ("hist_lds_counts", {"hist_mode": 1, "counts": True}), ("hist_global_counts", {"hist_mode": 2, "counts": True}),
                         ("given_hist_lds", {"hist_mode": 1, "given": True}), ("given_hist_lds_counts", {"hist_mode": 1, "given": True, "counts": True})):
            given = order[:args.given] if kw.pop("given", False) else ()
            listed = order[args.given:] if len(given) else order
            ms, hist = [], None
            for rep in range(args.repeats + 1):
                got = m.carrier_counts(listed, given, pass_ms=True, **kw)
                hist = got[0]
                if rep:
                    ms.append(got[-1])
            moved = (len(listed) + len(given)) * wp * 8
            legs[name] = {"pass_ms": spread(ms), "gbps": moved / (statistics.median(ms) * 1e-3) / 1e9, "bytes": moved,
                          "variants": int(hist.sum()), "bins_0_to_7": int(hist[:8].sum()), "nonzero_bins": int((hist > 0).sum())}
            legs[name]["fraction_of_capture_rank_rate"] = legs[name]["gbps"] / legs["capture_rank_m1"]["gbps"]
            if len(given) == 0:
                base = hist if base is None else base
                ok &= bool((hist == base).all()) and int(hist.sum()) == args.n_var
        legs["histograms_equal"] = ok
        out["a_all_samples"] = legs

    # (b) the host route over a prefix of the variants, against one call over the same prefix
    prefix = min(args.prefix, args.n_var)
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(prefix)
        m.synth_fill(c, seed=args.seed)
        slow, fast, hist_slow, hist_fast = [], [], None, None
        for rep in range(2):
            t0 = time.perf_counter()
            hist_slow = host_route(m, c, order, prefix)
            if rep:
                slow.append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            hist_fast = m.carrier_counts(order)
            if rep:
                fast.append((time.perf_counter() - t0) * 1e3)
    scale = args.n_var / prefix
    equal = bool((hist_slow == hist_fast).all())
    out["b_host_route"] = {"prefix_variants": prefix, "threads": THREADS, "host_route_wall_ms_prefix": spread(slow),
                           "host_route_wall_ms_scaled_to_full": statistics.median(slow) * scale, "scaled_by": scale,
                           "carrier_counts_wall_ms_prefix": spread(fast), "histograms_equal": equal}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not ok or not equal:
        sys.exit("the legs have to give the same histogram, and the host route's has to equal the call's")


if __name__ == "__main__":
    main()
