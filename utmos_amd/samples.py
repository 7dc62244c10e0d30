"""Per-sample capture curves: how much of each individual's own variation a panel holds (`select --samples-out`,
`select --represent-out`).

One capture-rank pass (DeviceMatrix.capture_rank) labels every variant with the row of the printed order that captured
it; one class-count pass (DeviceMatrix.class_counts -> utm_class_counts) with that rank as class then gives, for every
sample of the inputs at once, how many of ITS variants each row captured.  The rows may come from anywhere -- the greedy
loop, --include, --mode, --refine, quotas, filters: only the printed order is read.

    rank_labels(rank, k)                    capture ranks -> class labels, never captured = class k
    sample_table(matrix, order, depth)      (new, missed, total) of every sample under the order
    represent_rows(names, order, new, total)  the lines of --represent-out: a pure function of the table
    write_samples, write_represent          the .npz and the TSV
"""
import logging
import statistics

import numpy as np

from . import _native as nat

CLASSES_MAX = 16384                             # UTM_CLASSES_MAX
MAX_PANEL = CLASSES_MAX - 1                     # k rows + the class of the variants no row captured
REPRESENT_HEADER = "sample\tn_outside\tmean_pct\tmedian_pct\tmin_pct\tmin_sample\n"


def rank_labels(rank, k):
    """int32 class labels of capture ranks under a panel of k rows: the rank itself, -1 (never captured) -> k."""
    rank = np.asarray(rank, dtype=np.int32)
    return np.where(rank < 0, np.int32(k), rank).astype(np.int32)


def sample_table(matrix, order, depth=1, ranks=None):
    """(new, missed, total) for every sample of the matrix, in matrix order: new[j, i] = the variants of sample j that row
    i of `order` (global sample indices) captured at the given depth, missed[j] = those no row captured, total[j] = all
    it carries (int64).  ranks: the per-chunk capture ranks of the order, when the caller has them already."""
    k = len(order)
    if k > MAX_PANEL:
        raise ValueError(f"a panel of {k} rows: the class table holds {MAX_PANEL}")
    if ranks is None:
        ranks = [matrix.capture_rank(chunk, order, depth) for chunk in range(len(matrix.chunk_vars))]
    table = matrix.class_counts([rank_labels(r, k) for r in ranks], k + 1)
    return np.ascontiguousarray(table[:, :k]), table[:, k].copy(), table.sum(axis=1)


def represent_rows(names, order, new, total):
    """One tuple per row i of the order: (sample, n_outside, mean_pct, median_pct, min_pct, min_sample) over the samples
    OUTSIDE the panel of rows 0..i that carry anything (total > 0), with pct_j(i) = sum(new[j, :i + 1]) / total[j], rounded
    to 4 places; ties for the minimum go to the lowest index; nobody outside: nan, nan, nan and '.'."""
    new, total = np.asarray(new, dtype=np.int64), np.asarray(total, dtype=np.int64)
    outside = total > 0
    captured = np.zeros(len(total), dtype=np.int64)
    lines = []
    for i, member in enumerate(order):
        outside[member] = False
        captured += new[:, i]
        who = np.flatnonzero(outside)
        if len(who) == 0:
            lines.append((str(names[member]), 0, float("nan"), float("nan"), float("nan"), "."))
            continue
        pct = captured[who] / total[who]
        low = int(np.argmin(pct))                                        # (the first of equal minima)
        lines.append((str(names[member]), len(who), round(float(pct.mean()), 4), round(float(statistics.median(pct.tolist())), 4),
                      round(float(pct[low]), 4), str(names[who[low]])))
    return lines


def write_represent(path, lines):
    with open(path, "w") as fout:
        fout.write(REPRESENT_HEADER)
        for line in lines:
            fout.write("\t".join(str(field) for field in line) + "\n")


def write_samples(path, names, order, new, missed, total):
    np.savez(path, samples=np.asarray([str(name) for name in names], dtype=str), panel=np.asarray(order, dtype=np.int64),
             new=new, missed=missed, total=total)


def write_outputs(samples_out, represent_out, data, selected, depth, ranks=None):
    """select --samples-out / --represent-out: one class-count pass over the matrix under the printed order."""
    names = [str(name) for name in data["samples"]]
    position = {name: i for i, name in enumerate(names)}
    order = np.asarray([position[name] for name in selected], dtype=np.int64)
    try:
        new, missed, total = sample_table(data["data"], order, depth, ranks)
    except (ValueError, nat.NativeError) as err:
        logging.error("per-sample capture curves: %s", err)
        raise SystemExit(1)
    if samples_out:
        write_samples(samples_out, names, order, new, missed, total)
        logging.info("%s: capture curves of %d samples under %d selected samples", samples_out, len(names), len(order))
    if represent_out:
        write_represent(represent_out, represent_rows(names, order, new, total))
        logging.info("%s: how the %d rows represent the samples outside them", represent_out, len(order))
