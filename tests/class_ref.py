"""Numpy restatement of utm_class_counts, by definition: unpack every listed column, keep the variants it carries whose
label is not -1, and count the labels.  Shares no code with the kernel's helpers (csrc/classes.hip.h)."""
import numpy as np


def class_counts(cols, class_of, n_classes, indices=None, n_var=None):
    """int64 (n_rows, n_classes): table[j, c] = the variants v < n_var with class_of[v] == c that column indices[j] of
    cols (uint64 (n_samp, words), bit v & 63 of word v >> 6) carries; indices None = every column in index order."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    class_of = np.asarray(class_of, dtype=np.int64)
    n_var = len(class_of) if n_var is None else n_var
    indices = range(cols.shape[0]) if indices is None else indices
    table = np.zeros((len(indices), n_classes), dtype=np.int64)
    for j, s in enumerate(indices):
        bits = np.unpackbits(cols[s].view(np.uint8), bitorder="little")[:n_var].astype(bool)
        labels = class_of[:n_var][bits]
        table[j] = np.bincount(labels[labels >= 0], minlength=n_classes)
    return table


def class_counts_dense(dense, class_of, n_classes, indices=None):
    """The same from a boolean (n_var, n_samp) matrix."""
    dense = np.asarray(dense, dtype=bool)
    class_of = np.asarray(class_of, dtype=np.int64)
    indices = range(dense.shape[1]) if indices is None else indices
    table = np.zeros((len(indices), n_classes), dtype=np.int64)
    for j, s in enumerate(indices):
        labels = class_of[dense[:, s]]
        np.add.at(table[j], labels[labels >= 0], 1)
    return table
