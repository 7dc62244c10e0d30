#!/usr/bin/env python3
"""One select-all run of a synthetic matrix with the list launches' shape forced or left to the rule, for the sweep behind
DESIGN §19 (run each setting under `rocprofv3 --kernel-trace --stats`, then tools/list_phases.py on the trace):

  python3 tools/list_shape_run.py [--lanes 0|16|64] [--target 0|N] [--steps K] [--warmup W] [--n-var N] [--n-samp S]

Prints one JSON object: ms per step (each timed step), the list builds (utm_get_list_stats) and, where the library has
it, the lanes and workgroups of each build (utm_get_list_shape).  Reads nothing but the library."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from utmos_amd import device  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--lanes", type=int, default=0)
    p.add_argument("--target", type=int, default=0)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--n-var", type=int, default=10_000_000)
    p.add_argument("--n-samp", type=int, default=2504)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()
    with device.DeviceMatrix(a.n_samp, device=0) as m:
        c = m.add_chunk(a.n_var)
        m.synth_fill(c, seed=a.seed)
        if hasattr(m, "set_list_shape"):
            m.set_list_shape(a.lanes, a.target)
        elif a.lanes or a.target:
            sys.exit("this library has no utm_set_list_shape")
        ms, rows = [], None
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            m.reset()
            rows = m.run(a.n_samp)
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out = {"n_var": a.n_var, "n_samp": a.n_samp, "lanes": a.lanes, "target_wgs": a.target, "rows": len(rows[0]),
               "ms_per_step": ms, "loop_ms": m.stats()["loop_ms"], "list": m.list_stats(),
               "shape": m.list_shape() if hasattr(m, "list_shape") else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
