"""Population groups for `select`: the --groups file, the per-group coverage curves of --groups-out
(DeviceMatrix.group_curve, utm_group_curve) and the bookkeeping of the --group-max quota.  Nothing here scores a sample:
the quota runs the greedy loop that exists, for as many iterations as no group can fill in, and restarts it from the mask
(select._quota_selection)."""
import logging
import sys

import numpy as np

GROUPS_MAX = 64                     # UTM_GROUPS_MAX
SELECTABLE, EXCLUDED = 1, 2         # sample states, as select.py
GROUPS_HEADER = "k\tsample\tgroup\tnew\tcaptured\tpct_captured\tprivate_new\tprivate_captured\tprivate_pct\n"


def parse_groups(path, names):
    """Tab-delimited `sample<TAB>group` -> (int32 group id per sample of `names`, -1 = in no group; the group names).
    Groups are numbered in order of first appearance among the samples the input has; names it lacks are counted in one
    log line and ignored.  Exits with status 1 on a sample listed with two different groups or more than 64 groups."""
    position = {str(name): i for i, name in enumerate(names)}
    group_of = np.full(len(position), -1, dtype=np.int32)
    number, unknown = {}, 0
    with open(path, "r") as fh:
        for line in fh:
            if not line.strip():
                continue
            name, group = line.rstrip("\n").split("\t")[:2]
            if name not in position:
                unknown += 1
                continue
            if group not in number:
                number[group] = len(number)
            at = position[name]
            if group_of[at] >= 0 and group_of[at] != number[group]:
                logging.error("--groups: sample %s is listed with two different groups", name)
                sys.exit(1)
            group_of[at] = number[group]
    if len(number) > GROUPS_MAX:
        logging.error("--groups: %d groups, at most %d can be told apart", len(number), GROUPS_MAX)
        sys.exit(1)
    if not number:
        logging.error("--groups: %s names no sample of the input", path)
        sys.exit(1)
    logging.info("--groups: %d groups over %d of %d samples; %d listed names are not in the input and are ignored",
                 len(number), int((group_of >= 0).sum()), len(position), unknown)
    return group_of, list(number)


# ---------------------------------------------------------------------------------------------- the quota
def group_taken(group_of, n_groups, samples):
    """How many of `samples` (indices) every group holds."""
    ids = np.asarray(group_of)[np.asarray(samples, dtype=np.int64)]
    return np.bincount(ids[ids >= 0], minlength=n_groups).astype(np.int64)


def close_full_groups(states, group_of, taken, quota):
    """Mark the selectable rest of every group that holds `quota` selected samples excluded (in place)."""
    full = np.flatnonzero(np.asarray(taken) >= quota)
    states[np.isin(group_of, full) & (states == SELECTABLE)] = EXCLUDED
    return states


def quota_run_length(states, group_of, taken, quota, left):
    """For how many greedy iterations no group can fill: min over the groups that still have selectable members of
    quota - taken, at most `left`.  Call it after close_full_groups: every such group has room, so the result is at least
    1 while left is.  Without a selectable grouped sample nothing constrains the run."""
    open_groups = np.unique(np.asarray(group_of)[(np.asarray(states) == SELECTABLE) & (np.asarray(group_of) >= 0)])
    if len(open_groups) == 0:
        return int(left)
    return int(min(left, (quota - np.asarray(taken)[open_groups]).min()))


def quota_filter(order, group_of, taken, quota, left):
    """A fixed order (topN, random) under the quota: samples of a full group are skipped; at most `left` are kept."""
    taken = np.array(taken, dtype=np.int64)
    kept = []
    for sample in order:
        if len(kept) >= left:
            break
        g = group_of[sample]
        if g >= 0:
            if taken[g] >= quota:
                continue
            taken[g] += 1
        kept.append(sample)
    return np.asarray(kept, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- --groups-out
def _pct(part, whole):
    return round(int(part) / int(whole), 4) if whole else 0.0


def group_lines(samples, group_names, new, priv, total, ptotal):
    """The text of --groups-out below its header: one line per (row, group), k 1-based, captured cumulative."""
    captured, pcaptured = np.cumsum(new, axis=1), np.cumsum(priv, axis=1)
    lines = []
    for k, sample in enumerate(samples):
        for g, group in enumerate(group_names):
            lines.append("\t".join(str(field) for field in (
                k + 1, sample, group, int(new[g, k]), int(captured[g, k]), _pct(captured[g, k], total[g]),
                int(priv[g, k]), int(pcaptured[g, k]), _pct(pcaptured[g, k], ptotal[g]))) + "\n")
    return "".join(lines)


def write_group_curve(path, data, selected, group_of, group_names):
    """select --groups-out: one group_curve call over the samples of the TSV's rows, in row order."""
    names = [str(name) for name in data["samples"]]
    position = {name: i for i, name in enumerate(names)}
    order = np.asarray([position[name] for name in selected], dtype=np.int64)
    new, priv, total, ptotal = data["data"].group_curve(group_of, len(group_names), order)
    with open(path, "w") as fh:
        fh.write(GROUPS_HEADER)
        fh.write(group_lines(selected, group_names, new, priv, total, ptotal))
    for g, group in enumerate(group_names):
        logging.info("group %s: %d members, %d variants (%d private), %.1f%% captured", group, int((group_of == g).sum()),
                     int(total[g]), int(ptotal[g]), 100 * _pct(new[g].sum(), total[g]))
