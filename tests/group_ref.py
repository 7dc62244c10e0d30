"""numpy restatements for the group tests, by definition: unpack, OR per group, first carrier, bincount -- and the greedy
under a per-group quota as an argmax over the eligible samples per iteration."""
import numpy as np


def unpack(cols, n_var):
    """uint64 (S, W) packed columns -> bool (n_var, S)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return np.unpackbits(cols.view(np.uint8), axis=1, bitorder="little")[:, :n_var].T.astype(bool)


def group_curve_dense(dense, group_of, n_groups, order):
    """dense: bool (N, S); group_of: an id in 0..n_groups-1 per sample or -1; order: distinct sample indices.
    -> (new, priv, total, ptotal): new[g, j] = |{v in U_g : rank[v] == j}|, priv the same over P_g = U_g & ~multi,
    total[g] = |U_g|, ptotal[g] = |P_g|; rank[v] = the position of v's first carrier in the order, -1 without one."""
    dense = np.asarray(dense, dtype=bool)
    group_of = np.asarray(group_of)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    n = len(order)
    unions = np.stack([dense[:, group_of == g].any(axis=1) for g in range(n_groups)])      # (G, N); no samples: empty
    multi = unions.sum(axis=0) >= 2
    private = unions & ~multi
    listed = dense[:, order]
    rank = np.where(listed.any(axis=1), listed.argmax(axis=1), -1) if n else np.full(dense.shape[0], -1)
    new, priv = np.zeros((n_groups, n), np.int64), np.zeros((n_groups, n), np.int64)
    for g in range(n_groups):
        new[g] = np.bincount(rank[unions[g] & (rank >= 0)], minlength=n)[:n]
        priv[g] = np.bincount(rank[private[g] & (rank >= 0)], minlength=n)[:n]
    return new, priv, unions.sum(axis=1).astype(np.int64), private.sum(axis=1).astype(np.int64)


def group_curve(cols, group_of, n_groups, order, n_var):
    return group_curve_dense(unpack(cols, n_var), group_of, n_groups, order)


def greedy_with_quota(dense, states, weights, group_of, Q, k, include=()):
    """The greedy under a quota: `include` first (whatever it scores; it counts towards k and Q), then per iteration the
    first maximum of weight * newly captured variants among the samples with state 1 whose group holds fewer than Q
    selected samples (group -1: never limited), stopping at a best score of 0 or when every variant is captured.
    -> [(sample, new_count)] in selection order."""
    dense = np.asarray(dense, dtype=bool)
    states = np.array(states, copy=True)
    group_of = np.asarray(group_of)
    weights = np.ones(dense.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)
    covered = np.zeros(dense.shape[0], dtype=bool)
    taken = {}
    rows = []

    def take(s):
        gain = int((dense[:, s] & ~covered).sum())
        covered[:] |= dense[:, s]
        states[s] = 0
        if group_of[s] >= 0:
            taken[group_of[s]] = taken.get(group_of[s], 0) + 1
        rows.append((int(s), gain))

    for s in include:
        take(s)
        if covered.all():
            return rows
    while len(rows) < k and not covered.all():
        eligible = np.array([states[s] == 1 and (group_of[s] < 0 or taken.get(group_of[s], 0) < Q) for s in range(dense.shape[1])])
        scores = np.where(eligible, (dense & ~covered[:, None]).sum(axis=0) * weights, 0.0)
        best = int(np.argmax(scores))
        if scores[best] <= 0:
            break
        take(best)
    return rows


def topn_with_quota(dense, states, weights, group_of, Q, k, include=()):
    """topN under a quota: `include` first, then the samples with state 1 by their score right after the prefix (weight *
    newly captured variants), highest first, ties to the lower index, positive scores only, the samples of a full group
    skipped; no rescoring.  Rows end after the one that captures the last variant.  -> [(sample, new_count)]."""
    dense = np.asarray(dense, dtype=bool)
    states = np.array(states, copy=True)
    group_of = np.asarray(group_of)
    weights = np.ones(dense.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)
    include = np.asarray(include, dtype=np.int64)
    covered = dense[:, include].any(axis=1)
    rows = greedy_with_quota(dense, states, weights, group_of, Q, len(include), include)
    states[include] = 0
    taken = np.bincount(group_of[include][group_of[include] >= 0], minlength=int(group_of.max()) + 2)
    scores = np.where(states == 1, (dense & ~covered[:, None]).sum(axis=0) * weights, 0.0)
    for s in np.argsort(-scores, kind="stable"):
        if len(rows) >= k or scores[s] <= 0 or covered.all():
            break
        if group_of[s] >= 0:
            if taken[group_of[s]] >= Q:
                continue
            taken[group_of[s]] += 1
        rows.append((int(s), int((dense[:, s] & ~covered).sum())))
        covered |= dense[:, s]
    return rows
