"""Numpy restatement of utm_swap_gains, by definition: for every panel position i and every sample t, the union of the
columns of (panel - panel[i] + t); F = the number of rows (variants) of that union that are not empty.  No formula of the
kernels is used: no uniquely-covered sets, no product."""
import numpy as np


def unpack(cols, n_var):
    """uint64 (S, W) column bitsets -> bool (n_var, S)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return np.unpackbits(cols.view(np.uint8), axis=1, bitorder="little")[:, :n_var].T.astype(bool)


def captured(dense, members):
    """F: the rows some member carries."""
    return int(dense[:, list(members)].any(axis=1).sum()) if len(members) else 0


def swap_gains_unpacked(cols, panel, n_var):
    """(gains (k, S) int64, base): gains[i, t] = F(panel - panel[i] + t) - F(panel), base = F(panel) -- on the unpacked
    bool matrix, one union per (i, t).  The definition; slow."""
    dense = unpack(cols, n_var)
    panel = [int(p) for p in panel]
    base = captured(dense, panel)
    gains = np.zeros((len(panel), dense.shape[1]), np.int64)
    for i in range(len(panel)):
        for t in range(dense.shape[1]):
            gains[i, t] = captured(dense, panel[:i] + panel[i + 1:] + [t]) - base
    return gains, base


def swap_gains(cols, panel, n_var):
    """The same unions taken on the packed words (a set bit = a row of the union that is not empty; bits past n_var are
    cut), so that the shapes of the GPU tests take milliseconds.  test_swap_host.py holds it against the unpacked one."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    words = (n_var + 63) // 64
    valid = np.full(words, ~np.uint64(0))
    if n_var % 64:
        valid[-1] = np.uint64((1 << (n_var % 64)) - 1)
    cols = cols[:, :words] & valid
    panel = [int(p) for p in panel]
    count = lambda union: np.bitwise_count(union).sum(axis=-1, dtype=np.int64)
    union_of = lambda members: np.bitwise_or.reduce(cols[members], axis=0) if members else np.zeros(words, np.uint64)
    base = int(count(union_of(panel)))
    gains = np.zeros((len(panel), cols.shape[0]), np.int64)
    for i in range(len(panel)):
        rest = union_of(panel[:i] + panel[i + 1:])                      # the members that stay
        gains[i] = count(rest[None, :] | cols) - base                   # ... with every column t in turn
    return gains, base


def unique_counts(cols, panel, n_var):
    """Per member: the variants whose support within the panel is exactly 1 and that the member carries."""
    dense = unpack(cols, n_var)
    support = dense[:, list(panel)].sum(axis=1)
    return np.array([int((dense[:, p] & (support == 1)).sum()) for p in panel], np.int64)


def new_counts(cols, panel, n_var):
    """Per sample: the variants it carries and no member does."""
    dense = unpack(cols, n_var)
    missed = ~dense[:, list(panel)].any(axis=1) if len(panel) else np.ones(n_var, bool)
    return (dense & missed[:, None]).sum(axis=0).astype(np.int64)
