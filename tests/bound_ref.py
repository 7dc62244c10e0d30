"""The coverage bound restated in numpy on dense boolean rows (variants x samples), by the definition in
include/utmos_hip.h (utm_coverage_bound): int64 throughout, np.lexsort for the tie rule.  Also the exhaustive optimum of
tiny instances and the online bound by definition."""
import ctypes
import itertools

import numpy as np

Q = 65536
SENT = 77    # what host_bound prefills its outputs with


def eta(step0, period, t):
    return max(1, step0 >> min(63, t // period))


def coverage_bound(dense, k, cand=None, given=(), iters=200, step0=0, period=0):
    """dict(hist, bound, best_iter, n_live, lambdas): lambdas has one entry per row of `dense`, 0 where a row is not live."""
    dense = np.asarray(dense, dtype=bool)
    n_var, n_samp = dense.shape
    cand = np.arange(n_samp) if cand is None else np.asarray(cand, dtype=np.int64).reshape(-1)
    given = np.asarray(given, dtype=np.int64).reshape(-1)
    step0 = step0 or Q // 4
    period = period or max(1, iters // 14)
    live = ~dense[:, given].any(axis=1) if len(given) else np.ones(n_var, bool)
    a = (dense[:, cand] & live[:, None]).astype(np.int64)            # live rows of the candidate columns
    lam = np.where(live, Q, 0).astype(np.int64)
    kk = min(int(k), len(cand))
    hist = np.zeros(iters, np.int64)
    for t in range(iters):
        s = lam @ a                                                  # int64 column sums
        order = np.lexsort((np.arange(len(cand)), -s))               # largest first, ties to the smaller position
        picked = order[:kk]
        hist[t] = int((Q - lam[live]).sum()) + int(s[picked].sum())
        c = a[:, picked].sum(axis=1)
        lam = np.where(live, np.clip(lam - eta(step0, period, t) * (c - 1), 0, Q), 0)
    floors = hist // Q
    n_live = int(live.sum())
    return dict(hist=hist, bound=min(n_live, int(floors.min())), best_iter=int(np.argmin(floors)), n_live=n_live,
                lambdas=lam.astype(np.uint32))


def captured(dense, panel, given=()):
    """The rows some sample of `panel` carries and no sample of `given` does."""
    dense = np.asarray(dense, dtype=bool)
    panel, given = list(panel), list(given)
    live = ~dense[:, given].any(axis=1) if given else np.ones(dense.shape[0], bool)
    return int((dense[:, panel].any(axis=1) & live).sum()) if panel else 0


def exhaustive_optimum(dense, k, cand=None, given=()):
    """max over every panel of min(k, |cand|) candidates of what it captures beyond `given` (tiny instances only)."""
    dense = np.asarray(dense, dtype=bool)
    cand = list(range(dense.shape[1])) if cand is None else list(cand)
    kk = min(int(k), len(cand))
    return max((captured(dense, panel, given) for panel in itertools.combinations(cand, kk)), default=0)


def online_bound(dense, order, size, cand, given=()):
    """min over the prefixes S_i of `order` (i = 0 .. min(size, len(order))) of F(S_i) + the gains of the given samples
    outside S_i + the size - |given| largest gains(j | S_i) over the candidates.  Submodularity makes every term an upper
    bound on F(given + any size - |given| candidates)."""
    dense = np.asarray(dense, dtype=bool)
    cand, given = np.asarray(cand, dtype=np.int64), [int(g) for g in given]
    best = None
    covered = np.zeros(dense.shape[0], bool)
    for i in range(min(size, len(order)) + 1):
        if i:
            covered |= dense[:, order[i - 1]]
        gains = (dense & ~covered[:, None]).sum(axis=0)
        outside = [g for g in given if g not in list(order[:i])]
        top = np.sort(gains[cand])[::-1][:max(size - len(given), 0)].sum() if len(cand) else 0
        value = int(covered.sum()) + int(gains[outside].sum()) + int(top)
        best = value if best is None else min(best, value)
    return best


def bound_row(dense, order, size, cand, given=(), iters=200):
    """The line of `select --bound-out` for a panel size, by definition: [k, captured, bound_trivial, bound_online,
    bound_lagrange, bound, share] as text."""
    dense = np.asarray(dense, dtype=bool)
    given = [int(g) for g in given]
    base = captured(dense, given)
    got = captured(dense, list(order[:size]))
    res = coverage_bound(dense, size - len(given), cand=cand, given=given, iters=iters)
    trivial, lagrange = base + int(res["hist"][0] // Q), base + res["bound"]
    online = online_bound(dense, order, size, cand, given)
    bound = min(trivial, online, lagrange)
    return [str(x) for x in (size, got, trivial, online, lagrange, bound)] + [f"{1.0 if bound == 0 else got / bound:.4f}"]


# ----------------------------------------------------------------- the CPU build, called the same way
def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_bound(cols, n_var, k, cand=None, given=None, iters=12, step0=0, period=0, wp=None, want_rc=False):
    """dict like bound_ref.coverage_bound by the CPU build; every output is prefilled so that a value that is not written
    shows.  wp: a column stride wider than the words in use."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    n_samp, words = cols.shape
    if wp is not None and wp != words:
        wide = np.full((n_samp, wp), 0, np.uint64)
        wide[:, :words] = cols
        cols = wide
    c32 = None if cand is None else np.ascontiguousarray(cand, dtype=np.uint32)
    g32 = None if given is None else np.ascontiguousarray(given, dtype=np.uint32)
    hist = np.full(max(iters, 1), SENT, np.int64)
    lam = np.full(max(n_var, 1), SENT, np.uint32)
    bound, best, n_live = ctypes.c_int64(SENT), ctypes.c_int32(SENT), ctypes.c_int64(SENT)
    rc = nat.lib().utm_coverage_bound_host(p(cols), cols.shape[1], n_var, n_samp, p(c32), 0 if c32 is None else len(c32), p(g32),
                                           0 if g32 is None else len(g32), k, iters, step0, period, p(hist), ctypes.byref(bound),
                                           ctypes.byref(best), ctypes.byref(n_live), p(lam))
    out = dict(hist=hist[:iters], bound=bound.value, best_iter=best.value, n_live=n_live.value, lambdas=lam[:n_var])
    if want_rc:
        return rc, out
    nat.check(rc)
    return out
