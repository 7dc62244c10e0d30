"""numpy restatement of the greedy selection with a coverage depth M (set multicover), written the way the reference's
calculate_scores / greedy_select are: rows visited in order, a row skipped once M used samples carry it (the reference
skips it once any does: M = 1), float64 `scores += row`, weights, np.argmax's first maximum, stop on a best score of 0.

It is first held against the recorded traces of the reference's own code at M = 1 (tests/test_depth_host.py) and then
serves as the truth at M > 1, where the reference has nothing to say."""
import numpy as np

SELECTABLE, USED = 1, 0
HEADER = "sample\tvar_count\tnew_count\ttot_captured\tpct_captured\n"
HEADER_DEPTH = "sample\tvar_count\tnew_count\ttot_captured\tpct_captured\tat_depth\n"


def support_of(matrix, state):
    """Per row: how many used samples carry it."""
    return (matrix[:, np.asarray(state) == USED] != 0).sum(axis=1)


def calculate_scores(matrix, state, weights=None, depth=1):
    """One iteration: (best sample, its new count, the score vector handed to argmax) or (None, None, scores).
    The running sum is np.add.accumulate down the rows that still count: strictly row after row per sample, which is the
    reference's `scores += row` (adding the 0.0 of an absent cell changes nothing)."""
    n_samp = matrix.shape[1]
    live = matrix[support_of(matrix, state) < depth]
    scores = np.zeros(n_samp)
    counts = (live != 0).sum(axis=0)
    for lo in range(0, live.shape[0], 2048):
        scores = np.add.accumulate(np.vstack([scores[None, :], live[lo:lo + 2048].astype(np.float64)]), axis=0)[-1].copy()
    scores[np.asarray(state) != SELECTABLE] = 0
    if weights is not None:
        scores = scores * weights
    best = int(np.argmax(scores))
    if scores[best] == 0:
        return None, None, scores
    return best, int(counts[best]), scores


def greedy(matrix, state, k, weights=None, depth=1):
    """Rows (sample, new_count, score, at_depth) of up to k iterations; `state` is updated in place.  Ends on a best
    score of 0 or after the row that brings the total to depth x rows."""
    rows, total = [], 0
    for _ in range(k):
        best, new, scores = calculate_scores(matrix, state, weights, depth)
        if best is None:
            break
        state[best] = USED
        total += new
        rows.append((best, new, float(scores[best]), int((support_of(matrix, state) >= depth).sum())))
        if total >= depth * matrix.shape[0]:
            break
    return rows


def fixed_order(matrix, state, order, depth=1, total=0):
    """The same bookkeeping for samples taken in a given order whatever they score: rows (sample, new_count, at_depth)."""
    rows = []
    for s in order:
        new = int((matrix[support_of(matrix, state) < depth, s] != 0).sum())
        state[s] = USED
        total += new
        rows.append((int(s), new, int((support_of(matrix, state) >= depth).sum())))
        if total >= depth * matrix.shape[0]:
            break
    return rows


def tsv(rows, samples, var_count, n_var, depth, total=0, header=True):
    """The text `select --depth M` writes for rows of (sample, new_count, ..., at_depth)."""
    text = (HEADER_DEPTH if depth > 1 else HEADER) if header else ""
    total = np.int64(total)
    for row in rows:
        total += np.int64(row[1])
        fields = [samples[row[0]], int(var_count[row[0]]), row[1], int(total), round(total / (depth * n_var), 4)]
        if depth > 1:
            fields.append(row[-1])
        text += "\t".join(str(x) for x in fields) + "\n"
    return text


# ----------------------------------------------------------------- the packed form, for matrices of full size
def packed_greedy(cols, n_var, state, k, depth):
    """Integer scores on packed columns (uint64 (S, W)): per-variant uint8 support, gains = popcount(column & ~saturated).
    -> rows (sample, new_count, at_depth) and the support.  Shown equal to greedy() on small cases before it is used."""
    n_samp, n_words = cols.shape
    support = np.zeros(n_words * 64, np.uint8)
    for s in np.flatnonzero(np.asarray(state) == USED):
        support += np.unpackbits(cols[s].view(np.uint8), bitorder="little")
    np.minimum(support, depth, out=support)
    rows, total = [], 0
    for _ in range(k):
        open_words = np.packbits(support < depth, bitorder="little").view(np.uint64)
        gains = np.zeros(n_samp, np.int64)
        for lo in range(0, n_samp, 256):
            gains[lo:lo + 256] = np.bitwise_count(cols[lo:lo + 256] & open_words).sum(axis=1, dtype=np.int64)
        gains[np.asarray(state) != SELECTABLE] = 0
        best = int(np.argmax(gains))
        if gains[best] == 0:
            break
        carried = np.unpackbits((cols[best] & open_words).view(np.uint8), bitorder="little")
        support += carried
        state[best] = USED
        total += int(gains[best])
        rows.append((best, int(gains[best]), int((support[:n_var] >= depth).sum())))
        if total >= depth * n_var:
            break
    return rows, support[:n_var]
