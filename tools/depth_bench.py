#!/usr/bin/env python3
"""What a coverage depth M > 1 costs: select-all at M = 1 (brute-force launches: the persistent loop and decremental
scoring off) against M = 2 and M = 4 in the same process, on bench.py's default workload (10M x 2,504 synthetic).

All times are HIP-event times (utm_stats.loop_ms / score_ms, utm_get_depth's apply_ms), warm-up excluded.  A run is cut
into blocks of --block iterations so that the depths can be compared per iteration at EQUAL numbers of selectable
samples (block b of every run starts with n_samp - b * block of them; an M > 1 run saturates later, so over a whole run
it does more scoring work by construction).  k_depth_apply is reported on its own: time, launches, and GB/s for the
(2 P + 3) * wp * 8 bytes a launch moves, beside the context's streaming-read calibration.

The one gate: summed over the M = 2 run, k_depth_apply's time stays below the summed time of the scoring launches of
the same run (it streams 7 columns' worth per iteration where a scoring pass streams every selectable column).
--chr22 adds the 1,103,547 x 2,504 size, where M = 1 would run the persistent loop: reported only."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def select_all(m, depth, block):
    """One select-all at `depth`: per block (rows, loop_ms, score_ms, apply_ms) and the totals."""
    m.set_depth(depth)
    m.reset()
    blocks, prev_score, prev_apply, rows = [], 0.0, 0.0, 0
    while True:
        n = len(m.run(block)[0])
        st, dp = m.stats(), m.depth()
        blocks.append({"first_active": m.n_samples - rows, "rows": n, "loop_ms": st["loop_ms"],
                       "score_ms": st["score_ms"] - prev_score, "apply_ms": dp["apply_ms"] - prev_apply})
        prev_score, prev_apply, rows = st["score_ms"], dp["apply_ms"], rows + n
        if n < block:
            break
    st, dp = m.stats(), m.depth()
    return {"depth": depth, "rows": rows, "tot_captured": st["tot_captured"], "loop_ms": sum(b["loop_ms"] for b in blocks),
            "score_ms": st["score_ms"], "score_launches": st["score_launches"], "apply_ms": dp["apply_ms"],
            "apply_launches": dp["apply_launches"], "persist_iterations": st["persist_iterations"], "blocks": blocks}


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values)}


def measure(device, n_var, n_samp, seed, depths, repeats, block, calibration_launches):
    out = {"n_var": n_var, "n_samp": n_samp, "seed": seed, "block": block, "repeats": repeats, "runs": {}}
    with device.DeviceMatrix(n_samp, profile_events=True) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=seed)
        m.set_depth(max(depths))
        m.run(8)                                                     # warm-up: code objects, page tables (not reported)
        out["stream_calibration_gbps"] = m.stream_calibration(calibration_launches)
        wp = (n_var + 63) // 64
        wp = (wp + 127) // 128 * 128
        for depth in depths:
            runs = [select_all(m, depth, block) for _ in range(repeats)]
            first = runs[0]
            assert all(r["rows"] == first["rows"] and r["tot_captured"] == first["tot_captured"] for r in runs)
            planes = depth.bit_length() if depth > 1 else 0
            rec = {"rows": first["rows"], "tot_captured": first["tot_captured"], "score_launches": first["score_launches"],
                   "persist_iterations": first["persist_iterations"], "apply_launches": first["apply_launches"],
                   "loop_ms": spread([r["loop_ms"] for r in runs]), "score_ms": spread([r["score_ms"] for r in runs]),
                   "apply_ms": spread([r["apply_ms"] for r in runs]),
                   # per iteration, block by block (equal numbers of selectable samples across the depths)
                   "per_iteration_us_by_block": [
                       {"first_active": b["first_active"], "rows": b["rows"],
                        "loop_us": statistics.median(r["blocks"][i]["loop_ms"] for r in runs) * 1e3 / max(1, b["rows"]),
                        "score_us": statistics.median(r["blocks"][i]["score_ms"] for r in runs) * 1e3 / max(1, b["rows"]),
                        "apply_us": statistics.median(r["blocks"][i]["apply_ms"] for r in runs) * 1e3 / max(1, b["rows"])}
                       for i, b in enumerate(first["blocks"])]}
            if depth > 1:
                per_launch = (2 * planes + 3) * wp * 8
                rec["apply_bytes_per_launch"] = per_launch
                rec["apply_us_per_launch"] = rec["apply_ms"]["median"] * 1e3 / first["apply_launches"]
                rec["apply_gbps"] = per_launch * first["apply_launches"] / (rec["apply_ms"]["median"] * 1e-3) / 1e9
                rec["apply_share_of_stream_calibration"] = rec["apply_gbps"] / out["stream_calibration_gbps"]
            out["runs"][str(depth)] = rec
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--depths", type=str, default="1,2,4")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--block", type=int, default=128)
    p.add_argument("--calibration-launches", type=int, default=20)
    p.add_argument("--chr22", action="store_true", help="also 1,103,547 x 2,504: M = 1 with and without the persistent loop, M = 2")
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r06_depth_bench.json"))
    args = p.parse_args()
    depths = [int(x) for x in args.depths.split(",")]
    os.environ["UTM_PERSISTENT"] = "0"                               # the yardstick is the brute-force loop of launches
    from utmos_amd import device
    result = {"tool": "tools/depth_bench.py", "timing": "HIP events (utm_stats.loop_ms, score_ms; utm_get_depth apply_ms)",
              "default": measure(device, args.n_var, args.n_samp, args.seed, depths, args.repeats, args.block, args.calibration_launches)}
    if args.chr22:
        result["chr22_launches"] = measure(device, 1_103_547, 2504, args.seed, [1, 2], args.repeats, args.block, args.calibration_launches)
        os.environ["UTM_PERSISTENT"] = "1"                           # (read at the next reset)
        result["chr22_persistent_loop_allowed"] = measure(device, 1_103_547, 2504, args.seed, [1], args.repeats, args.block,
                                                          args.calibration_launches)
    two = result["default"]["runs"].get("2")
    if two:
        result["gate"] = {"apply_ms": two["apply_ms"]["median"], "score_ms": two["score_ms"]["median"],
                          "holds": two["apply_ms"]["median"] < two["score_ms"]["median"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result) + "\n")
    brief = {k: {d: {"rows": r["rows"], "loop_ms": r["loop_ms"]["median"], "score_ms": r["score_ms"]["median"],
                     "apply_ms": r["apply_ms"]["median"], "apply_gbps": r.get("apply_gbps")} for d, r in v["runs"].items()}
             for k, v in result.items() if isinstance(v, dict) and "runs" in v}
    print(json.dumps({"calibration_gbps": result["default"]["stream_calibration_gbps"], "gate": result.get("gate"), "runs": brief}))
    if two:
        assert result["gate"]["holds"], ("k_depth_apply takes longer than the scoring launches of the M = 2 run: %s" % result["gate"])


if __name__ == "__main__":
    main()
