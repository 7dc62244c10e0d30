"""How far is the panel from the best possible one?  (`select --bound-out`)

For every requested panel size K three upper bounds on what ANY K samples -- the --include samples among them -- can
capture, each certified by an inequality, none by a search:

    bound_trivial    F(given) + the K - |given| largest candidate counts beyond `given`
    bound_online     min over the prefixes S_i of the printed order of
                         F(S_i) + sum of gain(g | S_i) over the given samples outside S_i
                                + the K - |given| largest gain(j | S_i) over the candidates
                     (submodularity; the table of samples.sample_table gives every gain at once)
    bound_lagrange   F(given) + DeviceMatrix.coverage_bound: projected subgradient steps on the Lagrangian relaxation of
                     maximum coverage (utm_coverage_bound), which approach its LP bound

given = the --include samples, candidates = the run's selectable samples outside them.  `bound` is the smallest of the
three and `share` = captured / bound: the panel captures at least this share of what any panel of K can.

    refuse(args), refuse_several_processes(args), refuse_small_sizes(sizes, n_given)   the start-up refusals
    online_bound(...)                       the online bound from the per-sample table
    bound_rows(matrix, order, ...)          one row per K
    write_bounds(path, rows)                the TSV
"""
import logging
import os
import sys

import numpy as np

from . import _native as nat

Q = 65536
HEADER = "k\tcaptured\tbound_trivial\tbound_online\tbound_lagrange\tbound\tshare\n"


def parse_bound_at(text):
    """--bound-at K[,K...] -> a list of ints, or None."""
    if text is None:
        return None
    try:
        sizes = [int(item) for item in text.split(",") if item.strip()]
    except ValueError:
        sizes = []
    if not sizes or min(sizes) < 1:
        logging.error("--bound-at takes panel sizes of at least 1, comma separated")
        sys.exit(1)
    return sizes


def refuse(args):
    """The combinations --bound-out does not answer, refused before anything is loaded."""
    if not args.bound_out:
        given = "--bound-at" if args.bound_at is not None else "--bound-iters" if args.bound_iters is not None else None
        if given:
            logging.error("%s needs --bound-out", given)
            sys.exit(1)
        return
    clash = "--af" if args.af else "--weights" if args.weights else "--depth above 1" if args.depth > 1 else None
    if clash:
        logging.error("--bound-out bounds the plain number of captured variants and cannot be combined with %s", clash)
        sys.exit(1)
    if args.bound_iters is not None and not 1 <= args.bound_iters <= 65535:
        logging.error("--bound-iters must be between 1 and 65535")
        sys.exit(1)
    parse_bound_at(args.bound_at)


def refuse_several_processes(args):
    if args.bound_out and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--bound-out needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)


def refuse_small_sizes(sizes, n_given):
    """A K at or below the number of --include samples leaves nobody to choose."""
    for size in sizes or ():
        if size <= n_given:
            logging.error("--bound-at %d: the %d --include samples count towards it, nobody is left to choose", size, n_given)
            sys.exit(1)


def online_bound(new, missed, prefix_total, order, size, cand, given):
    """min over i = 0 .. min(size, len(order)) of F(S_i) + sum over the given samples outside S_i of gain(g | S_i) + the
    size - |given| largest gain(j | S_i) over the candidates, with gain(j | S_i) = missed[j] + sum(new[j, i:]) from the table
    of the order (samples.sample_table) and prefix_total[i] = F(S_i)."""
    new, missed = np.asarray(new, dtype=np.int64), np.asarray(missed, dtype=np.int64)
    rows = new.shape[1]
    # gains[:, i] = gain(. | S_i) for i = 0 .. rows
    tail = np.concatenate([np.cumsum(new[:, ::-1], axis=1)[:, ::-1], np.zeros((len(missed), 1), np.int64)], axis=1)
    gains = tail + missed[:, None]
    extra = size - len(given)
    best = None
    for i in range(min(size, rows, len(order)) + 1):
        outside = [g for g in given if g not in set(order[:i].tolist())]
        top = np.sort(gains[cand, i])[::-1][:extra].sum() if len(cand) and extra > 0 else 0
        value = int(prefix_total[i]) + int(gains[outside, i].sum()) + int(top)
        best = value if best is None else min(best, value)
    return best


def bound_rows(matrix, order, sizes, cand, given, iters=200):
    """One tuple (k, captured, bound_trivial, bound_online, bound_lagrange, bound, share) per size.  order: the printed
    rows' global sample indices; cand / given: global sample indices, disjoint."""
    from .samples import sample_table
    order = np.asarray(order, dtype=np.int64)
    cand, given = np.asarray(cand, dtype=np.int64), np.asarray(given, dtype=np.int64)
    n_variants = matrix.shape[0]
    head = order[:max(sizes)]
    if len(head):
        new, missed, _ = sample_table(matrix, head)
    else:
        new, missed = np.zeros((matrix.n_samples, 0), np.int64), np.asarray(matrix.var_count(), dtype=np.int64)
    # F(S_i) from the table itself: row r's sample carries every variant row r captured, so new[head[r], r] is the row's gain
    own = np.asarray([new[head[r], r] for r in range(len(head))], dtype=np.int64)
    prefix_total = np.concatenate([[0], np.cumsum(own)])
    out = []
    for size in sizes:
        captured = int(prefix_total[min(size, len(head))])
        if len(cand):
            res = matrix.coverage_bound(size - len(given), cand=cand, given=given if len(given) else None, iters=iters)
            base = n_variants - res.n_live                           # F(given)
            trivial, lagrange, ms, best_iter = base + int(res.hist[0] // Q), base + res.bound, res.pass_ms, res.best_iter
        else:                                                        # nobody to choose from: the given samples are the panel
            base = 0
            if len(given):
                base = n_variants - matrix.coverage_bound(1, cand=given[:1], given=given, iters=1).n_live
            trivial, lagrange, ms, best_iter = base, base, 0.0, 0
        online = online_bound(new, missed, prefix_total, head, size, cand, given.tolist())
        bound = min(trivial, online, lagrange)
        share = f"{1.0 if bound == 0 else captured / bound:.4f}"
        out.append((size, captured, trivial, online, lagrange, bound, share))
        logging.info("bound: any %d samples capture at most %d variants (trivial %d, online %d, lagrange %d at step %d of %d, "
                     "%.1f ms); the panel's %d are a share of %s", size, bound, trivial, online, lagrange, best_iter, iters, ms,
                     captured, share)
    return out


def write_bounds(path, rows):
    with open(path, "w") as fout:
        fout.write(HEADER)
        for row in rows:
            fout.write("\t".join(str(field) for field in row) + "\n")


def write_outputs(path, data, selected, sizes, states, included, iters):
    """select --bound-out: the bounds for every size (None: the number of rows the run produced)."""
    matrix = data["data"]
    position = {str(name): i for i, name in enumerate(data["samples"])}
    order = np.asarray([position[name] for name in selected], dtype=np.int64)
    given = np.asarray(included, dtype=np.int64)
    cand = np.asarray([s for s in np.flatnonzero(np.asarray(states) == 1) if s not in set(given.tolist())], dtype=np.int64)
    if sizes is None:
        sizes = [len(order)]
    if any(size <= len(given) for size in sizes):
        logging.warning("--bound-out: a panel of %d is all --include samples, nobody is left to choose: no bound for it", min(sizes))
    sizes = [size for size in sizes if size > len(given)]
    if matrix.shape[0] == 0 or not sizes:
        write_bounds(path, [(size, 0, 0, 0, 0, 0, "1.0000") for size in sizes])
        return
    try:
        rows = bound_rows(matrix, order, sizes, cand, given, iters)
    except (ValueError, nat.NativeError) as err:
        logging.error("coverage bound: %s", err)
        raise SystemExit(1)
    write_bounds(path, rows)
    logging.info("%s: upper bounds for %d panel size(s)", path, len(rows))
