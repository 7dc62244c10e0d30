"""numpy restatement of capture ranks (what the rank tests compare with): unpack the listed columns, cumulative sum along
the list, first position where it equals m."""
import numpy as np


def capture_rank(cols, order, m=1, n_var=None, block=16384):
    """cols: uint64 (S, W) packed columns; order: column indices; -> int32 per variant: the smallest i such that m of the
    columns order[0..i] carry the variant, -1 if none.  Variants are taken in blocks only to bound the memory."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    n_var = cols.shape[1] * 64 if n_var is None else int(n_var)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    rank = np.full(n_var, -1, dtype=np.int32)
    if len(order) == 0:
        return rank
    listed = cols[order].view(np.uint8)                              # (n, W * 8), little-endian bytes of the words
    for lo in range(0, n_var, block):                                # (block is a multiple of 8)
        hi = min(n_var, lo + block)
        bits = np.unpackbits(listed[:, lo // 8:(hi + 7) // 8], axis=1, bitorder="little")[:, :hi - lo]
        reached = np.cumsum(bits, axis=0, dtype=np.int32) == m       # first true: the column that brings the count to m
        rank[lo:hi] = np.where(reached.any(axis=0), reached.argmax(axis=0), -1)
    return rank


def variant_origin(informative_masks):
    """(part, row) per informative variant in matrix order, from every part's boolean mask over its records: what the
    loader has to deliver however it merges and cuts the parts into chunks."""
    part = np.concatenate([np.full(int(mask.sum()), i, np.int32) for i, mask in enumerate(informative_masks)] or [np.zeros(0, np.int32)])
    row = np.concatenate([np.flatnonzero(mask).astype(np.int64) for mask in informative_masks] or [np.zeros(0, np.int64)])
    return part, row
