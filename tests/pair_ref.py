"""Numpy restatement of utm_pair_counts, by definition: unpack the listed columns, zero the variants a `given` sample
carries, and multiply the 0/1 matrix with its transpose in int64.  No formula of the kernels is used: no blocks, no
mirror, no mask words."""
import numpy as np


def unpack(cols, n_var):
    """uint64 (S, W) column bitsets -> bool (n_var, S)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return np.unpackbits(cols.view(np.uint8), axis=1, bitorder="little")[:, :n_var].T.astype(bool)


def pair_counts_dense(dense, indices, given=()):
    """int64 (n, n) from a bool (variants, samples) matrix."""
    indices, given = [int(i) for i in indices], [int(g) for g in given]
    listed = dense[:, indices]
    if given:
        listed = listed & ~dense[:, given].any(axis=1)[:, None]
    b = listed.T.astype(np.int64)
    return b @ b.T


def pair_counts_unpacked(cols, indices, n_var, given=()):
    """The definition on the unpacked matrix; slow for the larger shapes."""
    return pair_counts_dense(unpack(cols, n_var), indices, given)


def pair_counts(cols, indices, n_var, given=()):
    """The same counts on the packed words (bits past n_var are cut), so that the shapes of the GPU tests take
    milliseconds.  test_pair_host.py holds it against the unpacked one."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    words = (n_var + 63) // 64
    keep = np.full(words, ~np.uint64(0))
    if n_var % 64:
        keep[-1] = np.uint64((1 << (n_var % 64)) - 1)
    given = [int(g) for g in given]
    if given:
        keep = keep & ~np.bitwise_or.reduce(cols[given, :words], axis=0)
    listed = cols[[int(i) for i in indices], :words] & keep
    n = len(listed)
    out = np.zeros((n, n), np.int64)
    for i in range(n):
        out[i] = np.bitwise_count(listed[i][None, :] & listed).sum(axis=1, dtype=np.int64)
    return out
