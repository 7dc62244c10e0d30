#!/usr/bin/env python3
"""Variant filters on bench.py's default workload (10M x 2,504 synthetic, seed 0), one process, one GPU:

  (a) utm_filter_variants under three masks -- random (about 50 % of the rows), AF-like (about 8 %: the rows whose
      generator AF is above a quantile, clustered the way the generator's site-frequency spectrum clusters them) and all
      ones -- on a freshly generated matrix each time: pass_ms (the zero fill of the new block, k_filter_prefix and
      k_filter_compact), the bytes moved (columns read + columns written) per second, and that rate as a fraction of
      utm_stream_calibration of the same context in the same process;
  (b) what there was before: utm_download_columns, numpy unpack / index / pack on 16 threads, utm_upload_columns, over a
      PREFIX of the variants (a matrix of its own from the same seed), its wall time scaled to the full size and labelled
      as scaled, against utm_filter_variants' wall time over the same prefix and at the full size;
  (c) the select-all loop (run over every sample, decremental scoring on, as `select` runs it) on the matrix filtered to
      about 8 % against the unfiltered matrix.

Prints one JSON object and writes it to --out.  The gates: (b)'s two results are equal, and the call beats the scaled host
round trip.
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


def padded_words(n_var):
    return max(128, ((n_var + 63) // 64 + 127) // 128 * 128)


def masks_for(n_var, n_samp, seed):
    rng = np.random.default_rng(seed)
    af = device.synth_host(seed, n_var, n_samp, want_cols=False)[1]
    return {"random_50": rng.random(n_var) < 0.5, "af_like_8": af >= np.quantile(af, 0.92), "all_ones": np.ones(n_var, bool)}


def host_round_trip(m, chunk, keep):
    """Download, unpack / index / pack per block of columns on THREADS threads, upload into a new chunk."""
    cols = m.download_columns(chunk)
    n_var = len(keep)
    kept = int(keep.sum())
    out = np.zeros((cols.shape[0], (kept + 63) // 64), dtype=np.uint64)
    step = max(1, (cols.shape[0] + 4 * THREADS - 1) // (4 * THREADS))

    def block(lo):
        bits = np.unpackbits(cols[lo:lo + step].view(np.uint8), axis=1, bitorder="little")[:, :n_var]
        packed = np.packbits(bits[:, keep], axis=1, bitorder="little")
        out[lo:lo + step].view(np.uint8)[:, :packed.shape[1]] = packed

    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(block, range(0, cols.shape[0], step)))
    new = m.add_chunk(kept)
    m.upload_columns(new, out)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--prefix", type=int, default=1_000_000)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    out = {"workload": f"synthetic {args.n_var} x {args.n_samp}", "seed": args.seed}
    masks = masks_for(args.n_var, args.n_samp, args.seed)
    loops = {}
    with device.DeviceMatrix(args.n_samp) as m:
        c = m.add_chunk(args.n_var)
        m.synth_fill(c, seed=args.seed)
        out["stream_calibration_gbps"] = m.stream_calibration(20)
        m.set_decremental(True)
        m.reset()
        t0 = time.perf_counter()
        rows = len(m.run(args.n_samp)[0])
        loops["unfiltered"] = {"rows": rows, "wall_ms": (time.perf_counter() - t0) * 1e3, "loop_ms": m.stats()["loop_ms"], "variants": args.n_var}
    for name, keep in masks.items():
        ms, wall, kept = [], [], 0
        for rep in range(args.repeats + 1):
            with device.DeviceMatrix(args.n_samp) as m:               # a fresh matrix for every measurement
                c = m.add_chunk(args.n_var)
                m.synth_fill(c, seed=args.seed)
                t0 = time.perf_counter()
                kept, t = m.filter_variants(c, keep, pass_ms=True)
                if rep:
                    ms.append(t)
                    wall.append((time.perf_counter() - t0) * 1e3)
                if name == "af_like_8" and rep == args.repeats:       # (c): the loop on the filtered matrix
                    m.set_decremental(True)
                    m.reset()
                    t0 = time.perf_counter()
                    rows = len(m.run(args.n_samp)[0])
                    loops["filtered_8"] = {"rows": rows, "wall_ms": (time.perf_counter() - t0) * 1e3, "loop_ms": m.stats()["loop_ms"],
                                           "variants": kept}
        moved = args.n_samp * 8 * (padded_words(args.n_var) + padded_words(kept)) if kept != args.n_var else 0
        leg = {"kept": kept, "kept_share": kept / args.n_var, "pass_ms": spread(ms), "wall_ms": spread(wall), "bytes_moved": moved}
        if moved:
            leg["gbps"] = moved / (statistics.median(ms) * 1e-3) / 1e9
            leg["fraction_of_stream_calibration"] = leg["gbps"] / out["stream_calibration_gbps"]
        out[name] = leg
    loops["unfiltered_over_filtered_wall"] = loops["unfiltered"]["wall_ms"] / loops["filtered_8"]["wall_ms"]
    out["select_all_loop"] = loops

    # (b) the host round trip over a prefix, against the call over the same prefix
    prefix = min(args.prefix, args.n_var)
    keep = masks["random_50"][:prefix]
    slow, fast = [], []
    with device.DeviceMatrix(args.n_samp) as m:
        for rep in range(2):
            c = m.add_chunk(prefix)
            m.synth_fill(c, seed=args.seed)
            t0 = time.perf_counter()
            got_slow = host_round_trip(m, c, keep)
            if rep:
                slow.append((time.perf_counter() - t0) * 1e3)
        for rep in range(args.repeats + 1):
            c = m.add_chunk(prefix)
            m.synth_fill(c, seed=args.seed)
            t0 = time.perf_counter()
            m.filter_variants(c, keep)
            if rep:
                fast.append((time.perf_counter() - t0) * 1e3)
        equal = bool((m.download_columns(c) == got_slow).all())
    scale = args.n_var / prefix
    scaled = statistics.median(slow) * scale
    full = out["random_50"]["wall_ms"]["median"]
    out["b_host_round_trip"] = {"prefix_variants": prefix, "threads": THREADS, "host_wall_ms_prefix": spread(slow),
                                "host_wall_ms_scaled_to_full": scaled, "scaled_by": scale, "filter_wall_ms_prefix": spread(fast),
                                "filter_wall_ms_full": full, "speedup_full_call_over_scaled_host": scaled / full, "results_equal": equal}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if not equal:
        sys.exit("the host round trip and the call have to give the same columns")
    if full >= scaled:
        sys.exit("the call has to beat the scaled host round trip")


if __name__ == "__main__":
    main()
