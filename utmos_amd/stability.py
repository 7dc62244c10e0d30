"""select --replicates: how far a panel depends on the variants that happened to be called.

Delete-half resampling (stability selection): the greedy selection runs on B random subsets of the variants at once
(DeviceMatrix.multi_select, utm_multi_select); what comes out is how often every sample is selected and the band of
the coverage curves.  Pure functions over the arrays of multi_select, plus the two writers of the command."""
import logging

import numpy as np

TABLE_HEADER = "sample\tselected\tfrequency\tmean_rank\tin_panel\n"
MAX_REPLICATES = 256


def keep_threshold(fraction):
    """The 32-bit threshold of the hashed masks that keeps a share `fraction` of the variants: floor(fraction * 2^32)
    for 0 < fraction <= 1 (1.0 = 2^32 keeps everything)."""
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError("the kept share of the variants must be above 0 and at most 1")
    return int(np.floor(fraction * 2.0 ** 32))


def selection_table(order, n_done, names, panel):
    """One row [sample, selected, frequency, mean_rank, in_panel] per sample that any replicate or the panel selected.
    order (B, k) and n_done (B,) as multi_select returns them; panel = the sample indices of the run's own selection.
    selected = in how many replicates; frequency = selected / B to 4 places; mean_rank = the mean 1-based row over the
    replicates that selected it, to 2 places (nan when only the panel did); in_panel 1 / 0.  Sorted by selected
    descending, then the unrounded mean_rank ascending, then the sample index."""
    order = np.asarray(order)
    n_done = np.asarray(n_done)
    reps = order.shape[0]
    selected = np.zeros(len(names), dtype=np.int64)
    rank_sum = np.zeros(len(names), dtype=np.int64)
    for b in range(reps):
        row = order[b, :int(n_done[b])]
        selected[row] += 1
        rank_sum[row] += np.arange(1, len(row) + 1)
    in_panel = np.zeros(len(names), dtype=bool)
    in_panel[np.asarray(panel, dtype=np.int64)] = True
    listed = np.flatnonzero((selected > 0) | in_panel)
    mean_rank = {int(s): (rank_sum[s] / selected[s] if selected[s] else float("inf")) for s in listed}
    listed = sorted((int(s) for s in listed), key=lambda s: (-int(selected[s]), mean_rank[s], s))
    return [[str(names[s]), int(selected[s]), round(int(selected[s]) / reps, 4),
             round(float(mean_rank[s]), 2) if selected[s] else float("nan"), int(in_panel[s])] for s in listed]


def curve_band(new, kept):
    """(mean, minimum, maximum) per row over the replicates of the share captured so far: cumulative new / kept.  A
    replicate that stopped early carries its last value (its later entries of `new` are 0); one without variants holds 0."""
    new = np.asarray(new, dtype=np.int64)
    kept = np.asarray(kept, dtype=np.int64)
    share = np.cumsum(new, axis=1) / np.maximum(kept, 1)[:, None]
    if share.shape[1] == 0:
        empty = np.zeros(0, dtype=np.float64)
        return empty, empty.copy(), empty.copy()
    return share.mean(axis=0), share.min(axis=0), share.max(axis=0)


def run_replicates(matrix, rounds, states, replicates, fraction, seed):
    """The B replicates of a run: hashed masks of `seed` that keep `fraction` of the variants, the run's own states in
    every replicate.  Returns multi_select's (order, new, kept, n_done)."""
    order, new, kept, n_done, ms = matrix.multi_select(rounds, states, seed=seed, fraction=fraction, n_rep=replicates, pass_ms=True)
    logging.info("%d replicates over %.4g of the variants: %d to %d rows, %.1f ms on the device", replicates, fraction,
                 int(n_done.min()), int(n_done.max()), ms)
    return order, new, kept, n_done


def write_table(path, table):
    with open(path, "w") as fout:
        fout.write(TABLE_HEADER)
        for row in table:
            fout.write("\t".join(str(field) for field in row) + "\n")
    logging.info("%s: selection frequencies of %d samples", path, len(table))


def write_replicates(path, result, names, panel, seed, fraction):
    """numpy .npz: order, new, kept, n_done, the curve band (pct_mean, pct_min, pct_max), samples (every name of the
    input, what `order` and `panel` index), panel, seed, fraction."""
    order, new, kept, n_done = result
    mean, low, high = curve_band(new, kept)
    np.savez(path, order=order, new=new, kept=kept, n_done=n_done, pct_mean=mean, pct_min=low, pct_max=high,
             samples=np.asarray([str(name) for name in names], dtype=str), panel=np.asarray(panel, dtype=np.int64),
             seed=np.int64(seed), fraction=np.float64(fraction))
    logging.info("%s: %d replicates of up to %d rows", path, order.shape[0], order.shape[1])
