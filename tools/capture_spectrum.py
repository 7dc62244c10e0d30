#!/usr/bin/env python3
"""What a panel of the first k selected samples captures, by allele frequency, from a `select --variants-out` file.

The file holds one capture rank per variant (the row at which it was captured, -1: never), so every panel size is
answered from it alone: captured by the first k = (0 <= rank < k).  Prints a tab-separated table: one line per AF bin,
the number of variants in it and the captured fraction for each k; host only.  `--missed K` lists instead the (file,
record) of every variant a panel of K misses.
"""
import argparse

import numpy as np


def main():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("variants", help="the .npz written by select --variants-out")
    p.add_argument("-k", type=int, nargs="+", default=None, help="panel sizes [all selected samples]")
    p.add_argument("--bins", type=float, nargs="+", default=[0.001, 0.01, 0.05], help="inner AF bin edges [%(default)s]")
    p.add_argument("--missed", type=int, default=None, metavar="K", help="list the variants a panel of K misses: file, record, AF")
    args = p.parse_args()
    z = np.load(args.variants, allow_pickle=False)
    rank = z["rank"]
    af = z["af"] if "af" in z.files else None
    if args.missed is not None:
        files = z["files"]
        for v in np.flatnonzero((rank < 0) | (rank >= args.missed)):
            print("\t".join([str(files[z["part"][v]]), str(int(z["row"][v])), "nan" if af is None else repr(float(af[v]))]))
        return
    sizes = args.k or [len(z["samples"])]
    edges = [0.0] + sorted(args.bins) + [1.0]
    groups = []
    if af is not None:
        which = np.digitize(af, edges[1:-1])                      # bin i: edges[i] <= AF < edges[i + 1]; the last one closed
        for i in range(len(edges) - 1):
            groups.append((f"[{edges[i]:g},{edges[i + 1]:g}" + ("]" if i == len(edges) - 2 else ")"), which == i))
    groups.append(("all", np.ones(len(rank), bool)))
    print("\t".join(["af_bin", "variants"] + [f"k={k}" for k in sizes]))
    for label, members in groups:
        r = rank[members]
        cells = [f"{((r >= 0) & (r < k)).mean():.4f}" if len(r) else "nan" for k in sizes]
        print("\t".join([label, str(len(r))] + cells))


if __name__ == "__main__":
    main()
