"""Numpy restatement of utm_carrier_counts, by definition: unpack the listed columns, sum along the samples, mask with the
OR of the `given` columns and bincount.  No formula of the kernel is used: no planes, no blocks, no popcounted bins."""
import numpy as np


def unpack(cols, n_var):
    """uint64 (S, W) column bitsets -> uint8 (S, n_var) of 0 / 1."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return np.unpackbits(cols.view(np.uint8), axis=1, bitorder="little")[:, :n_var]


def carrier_counts(cols, indices, n_var, given=()):
    """(hist int64 (n + 1), count int32 (n_var) with -1 where a `given` sample carries the variant)."""
    indices, given = [int(i) for i in indices], [int(g) for g in given]
    n = len(indices)
    bits = unpack(cols, n_var)
    count = bits[indices].sum(axis=0, dtype=np.int64) if n else np.zeros(n_var, np.int64)
    masked = bits[given].any(axis=0) if given else np.zeros(n_var, bool)
    hist = np.bincount(count[~masked], minlength=n + 1).astype(np.int64)
    return hist, np.where(masked, -1, count).astype(np.int32)


def carrier_counts_dense(dense, indices, given=()):
    """The same from a bool (variants, samples) matrix."""
    indices, given = [int(i) for i in indices], [int(g) for g in given]
    count = dense[:, indices].sum(axis=1, dtype=np.int64)
    masked = dense[:, given].any(axis=1) if given else np.zeros(len(dense), bool)
    return np.bincount(count[~masked], minlength=len(indices) + 1).astype(np.int64), np.where(masked, -1, count).astype(np.int32)
