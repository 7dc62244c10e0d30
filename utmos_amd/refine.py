"""1-swap local search on a selected panel: exchange one member for one sample outside it whenever that captures more
variants, until no exchange helps.

Greedy maximum coverage is a (1 - 1/e) approximation; a panel that no single exchange improves is the usual cheap step
beyond it.  Every round is ONE `matrix.swap_gains(panel)` (utm_swap_gains: all k x n gains from two launches per chunk);
the choice among them is made here.
"""
import numpy as np

SELECTABLE = 1      # sample state "can be selected" (select.SELECTABLE)

LOG_HEADER = "swap\tout\tin\tgain\ttot_captured\n"


def best_swap(gains, panel, candidates, pinned=()):
    """(gain, i, t) of the best exchange: panel position i leaves, sample t comes in.  The largest gain wins; ties go to
    the smallest position i, then to the smallest t.  Positions whose member is pinned never leave; only `candidates`
    (a boolean mask over the samples) come in.  None when no pair is allowed."""
    gains = np.asarray(gains)
    movable = ~np.isin(np.asarray(panel), np.asarray(list(pinned), dtype=np.int64))
    allowed = movable[:, None] & np.asarray(candidates, dtype=bool)[None, :]
    if not allowed.any():
        return None
    masked = np.where(allowed, gains, np.iinfo(np.int64).min)
    i, t = np.unravel_index(np.argmax(masked), masked.shape)     # (row-major first maximum: smallest i, then smallest t)
    return int(gains[i, t]), int(i), int(t)


def refine(matrix, panel, states, pinned=(), max_swaps=None):
    """Improve `panel` (sample indices) by 1-swaps.  matrix: anything with swap_gains(panel) -> (gains, unique, new, base)
    (device.DeviceMatrix); states: the samples' states before the selection -- the samples with state 1 that are not in
    the panel may come in; pinned: members that never leave (the --include samples); max_swaps: at most this many
    exchanges, None = until none helps.

    Returns (panel, log): the incoming sample takes the leaver's position; log = [(swap, out, in, gain, tot_captured)],
    swap counting from 1.  Every exchange raises the captured count by at least 1, so the search ends."""
    panel = [int(s) for s in panel]
    states = np.asarray(states)
    log = []
    while panel and (max_swaps is None or len(log) < max_swaps):
        gains, _, _, base = matrix.swap_gains(panel)
        candidates = states == SELECTABLE
        candidates[panel] = False
        best = best_swap(gains, panel, candidates, pinned)
        if best is None or best[0] <= 0:
            break
        gain, i, t = best
        log.append((len(log) + 1, panel[i], t, gain, int(base) + gain))
        panel[i] = t
    return panel, log


def write_log(path, log, names):
    """The swap log as a TSV: swap, the leaver's and the newcomer's name, the gain, tot_captured after the exchange."""
    with open(path, "w") as out:
        out.write(LOG_HEADER)
        for swap, leaver, newcomer, gain, total in log:
            out.write(f"{swap}\t{names[leaver]}\t{names[newcomer]}\t{gain}\t{total}\n")
