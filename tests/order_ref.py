"""numpy restatement of a fixed order's coverage curve and of the order helpers (what the order tests compare with)."""
import numpy as np


def order_curve(cols, order, covered=None, n_var=None):
    """cols: uint64 (S, W) packed columns; -> (gains int64 per position, covered words afterwards).  With n_var the
    curve ends after the position that captures the last variant, like utm_apply_order."""
    cov = np.zeros(cols.shape[1], np.uint64) if covered is None else np.array(covered, dtype=np.uint64)
    gains, total = [], 0
    for s in order:
        gains.append(int(np.bitwise_count(cols[s] & ~cov).sum()))
        cov |= cols[s]
        total += gains[-1]
        if n_var is not None and total >= n_var:
            break
    return np.array(gains, dtype=np.int64), cov


def topn_order(scores, states):
    """Selectable (state 1) samples by score descending, ties to the lower index, positive scores only."""
    cand = [i for i in range(len(states)) if states[i] == 1 and scores[i] > 0]
    return np.array(sorted(cand, key=lambda i: (-scores[i], i)), dtype=np.int64)


def random_order(states, seed):
    return np.random.default_rng(seed).permutation(np.flatnonzero(np.asarray(states) == 1))


# ----------------------------------------------------------------- reference-made fixtures (tools/make_order_traces.py)
def case_names():
    import os
    import oracle_util as ou
    return sorted(f[:-5] for f in os.listdir(os.path.join(ou.GOLD, "order")) if f.endswith(".json"))


def load_case(name):
    """A record of tests/golden/order with its parts as arrays (`part_list`) and the packed columns of what the
    reference scored (`cols`: rows nobody carries dropped; with --af, rows whose AF is 0 hold nothing)."""
    import json
    import os
    import oracle_util as ou
    t = json.load(open(os.path.join(ou.GOLD, "order", name + ".json")))
    if "inputs" in t:
        t["part_list"] = [ou.load_part(n) for n in t["inputs"]]
    else:
        t["part_list"] = []
        for p in t["parts"]:
            n_samp = len(p["samples"])
            gt = np.frombuffer(bytes.fromhex(p["gt_hex"]), dtype=np.uint8).reshape(p["n_rows"], (n_samp + 7) // 8)
            t["part_list"].append({"GT": gt, "AF": np.array([float.fromhex(x) for x in p["af_hex"]]),
                                   "samples": np.array(p["samples"])})
    matrix, var_count, samples = ou.npo.build_matrix(t["part_list"], af=t["af"], af_dtype=t["af_dtype"] or "f64")
    t["cols"] = ou.npo.pack_columns(matrix != 0)
    t["var_count"], t["samples"] = var_count, [str(s) for s in samples]
    return t


def case_tsv(t):
    """The TSV `select --include <prefix> -c <count>` has to write for a case, composed from the recorded gains."""
    rows = list(zip(t["order"], t["gains"])) + list(zip(t["cont_idx"], t["cont_gains"]))
    text, total = "sample\tvar_count\tnew_count\ttot_captured\tpct_captured\n", np.int64(0)
    for (sample, gain), var_count in zip(rows, t["rows_var_count"]):
        total += np.int64(gain)
        text += "\t".join(str(x) for x in [t["samples"][sample], var_count, gain, int(total), round(total / t["n_var"], 4)]) + "\n"
    return text
