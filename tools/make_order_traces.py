#!/usr/bin/env python3
"""Record what the REFERENCE's own code answers for a forced order of samples (build container only; needs the
reference checkout that tools/make_traces.py names).

The reference has no fixed-order mode any more (utmos/select.py:140-142), but its `calculate_scores(matrix, mask,
weights)` answers the question one sample at a time: with the next forced sample as the only `1`, the ones before it
`0` and everyone else `2`, it returns that sample and its new-variant count (select.py:36-53), or (None, None) when the
count is 0.  After the prefix its `greedy_select`, with the prefix at `0` and everyone else back at their real state,
gives the continuation (its tot_captured starts at 0: the tests add the prefix total).  The module is imported
unmodified from where it lies, exactly as tools/make_traces.py does; only data is written:

  tests/golden/order/<case>.json   inputs (fixture names, or a micro-matrix as hex), options, the forced order, the gain of
                                   every position up to the one that captures the last variant, the continuation's winners
                                   and gains, and the var_count column of every row

Weights are all positive: with a weight <= 0 the reference's argmax lands on a masked zero and it answers None for a
sample that does gain variants.
"""
import json
import os
import tempfile

import numpy as np

import make_traces as mt

OUT = os.path.join(mt.GOLD, "order")
PREFIX = [0, 2400, 17, 999, 5]


def read_names(name):
    return [ln.strip() for ln in open(os.path.join(mt.GOLD, name))]


def read_weights(name):
    return {ln.split("\t")[0]: float(ln.split("\t")[1]) for ln in open(os.path.join(mt.GOLD, name)) if ln.strip()}


def micro_part(seed, n_var, n_samp, twin=None, full=None, zero_af_rows=0):
    """Seeded micro-matrix: `twin` = (a, b) makes column b a copy of column a (b then gains nothing after a); `full` = a
    column that carries every variant."""
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(np.log(1.0 / n_samp), 0.0, size=n_var))[:, None]
    dense = rng.random((n_var, n_samp)) < p
    dense[np.arange(n_var), rng.integers(0, n_samp, size=n_var)] = True
    if twin:
        dense[:, twin[1]] = dense[:, twin[0]]
    if full is not None:
        dense[:, full] = True
    af = np.maximum(dense.sum(axis=1), 1) / (2.0 * n_samp)
    if zero_af_rows:
        af[rng.choice(n_var, zero_af_rows, replace=False)] = 0.0
    return mt.part_from_dense(dense, af, [f"S{i:03d}" for i in range(n_samp)])


def record(sel, tmp, label, parts, inputs, order, count, af=False, f32=False, subset=None, exclude=None, weights=None):
    files = [mt.write_jl(tmp, f"{label}_p{i}", p) for i, p in enumerate(parts)]
    data = sel.load_files(files, None, 32768, af)
    matrix = data["data"].astype(np.float32) if f32 else data["data"]
    names = [str(x) for x in data["samples"].astype(str)]
    n_var, n_samp = matrix.shape
    var_count = np.asarray(data["var_count"][:])
    state = np.ones(n_samp, dtype="uint8")
    if subset:
        state = np.where(np.isin(names, read_names(subset)), 1, 2).astype("uint8")
    if exclude:
        state = np.where(np.isin(names, exclude), 2, state).astype("uint8")
    vector = None
    if weights:
        table = read_weights(weights)
        assert all(w > 0 for w in table.values())
        vector = np.array([table.get(n, 1.0) for n in names], dtype=np.float64)

    gains, total = [], 0
    for i, s in enumerate(order):
        mask = np.full(n_samp, 2, dtype="uint8")
        mask[order[:i]] = 0
        mask[s] = 1
        use, new = sel.calculate_scores(matrix, mask, vector)
        assert use is None or int(use) == s, (label, i, use)
        gains.append(0 if use is None else int(new))
        total += gains[-1]
        if total >= n_var:          # the row that captures the last variant ends the rows
            break
    done = order[:len(gains)]
    cont_idx, cont_gains = [], []
    left = count - len(done)
    if left > 0 and total < n_var:
        mask = state.copy()
        mask[done] = 0
        index = {n: i for i, n in enumerate(names)}
        for row in sel.greedy_select(matrix, var_count, left, np.asarray(names), mask, vector):
            cont_idx.append(index[row[0]])
            cont_gains.append(int(row[2]))
    rec = {"af": bool(af), "af_dtype": ("f32" if f32 else "f64") if af else None, "subset": subset, "exclude": exclude,
           "weights": weights, "include": [names[s] for s in order], "order": [int(s) for s in order], "gains": gains,
           "count": int(count), "cont_idx": cont_idx, "cont_gains": cont_gains, "n_var": int(n_var),
           "rows_var_count": [int(var_count[s]) for s in list(done) + cont_idx],
           "outside_subset": [names[s] for s in order if state[s] != 1]}
    rec.update({"inputs": inputs} if inputs else {"parts": [mt.part_json(p) for p in parts]})
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, label + ".json"), "w") as fh:
        json.dump(rec, fh, indent=0, separators=(",", ":"))
    print(f"{label}: gains={gains} continuation={len(cont_idx)} rows")
    return rec


def main():
    sel = mt.import_reference()
    two = ["chunk0", "chunk1"]
    parts = [mt.load_fixture(n) for n in two]
    with tempfile.TemporaryDirectory() as tmp:
        r = record(sel, tmp, "chunks_int", parts, two, PREFIX, 20)
        assert r["gains"] == [59, 24, 19, 16, 16], r["gains"]
        record(sel, tmp, "chunks_af64", parts, two, PREFIX, 20, af=True)
        record(sel, tmp, "chunks_af32", parts, two, PREFIX, 20, af=True, f32=True)
        record(sel, tmp, "chunks_weights", parts, two, PREFIX, 20, weights="weights.txt")
        record(sel, tmp, "chunks_af64_weights", parts, two, PREFIX, 16, af=True, weights="weights.txt")
        r = record(sel, tmp, "chunks_subset", parts, two, PREFIX, 20, subset="subset.txt", exclude=["HG00097"])
        assert r["outside_subset"], "the prefix should reach outside subset.txt"
        # seeded micro-matrices: a prefix member that gains nothing, a prefix that captures everything before its end,
        # n_var not a multiple of 64 (all of them), AF == 0 rows
        r = record(sel, tmp, "micro_zero_gain", [micro_part(71, 300, 24, twin=(3, 9))], None, [3, 9, 0, 20], 12)
        assert r["gains"][1] == 0
        r = record(sel, tmp, "micro_full_prefix", [micro_part(72, 257, 20, full=6)], None, [2, 6, 11, 4], 10)
        assert len(r["gains"]) == 2 and not r["cont_idx"]
        record(sel, tmp, "micro_two_parts", [micro_part(73, 129, 33), micro_part(74, 70, 33)], None, [32, 0, 7], 33)
        for label, f32 in (("micro_af_zero_rows", False), ("micro_af_zero_rows_f32", True)):
            record(sel, tmp, label, [micro_part(75, 400, 33, zero_af_rows=60)], None, [1, 30, 8, 2], 14, af=True, f32=f32)


if __name__ == "__main__":
    main()
