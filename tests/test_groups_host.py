"""No GPU: the CPU build of the group kernels' word arithmetic (utm_group_curve_host) against the numpy restatement by
definition (tests/group_ref.py), the refusals that need no device, the --groups file, the quota's bookkeeping, the text
of --groups-out and the command-line refusals."""
import ctypes
import functools

import numpy as np
import pytest

import group_ref
import oracle_util as ou
from oracle_util import npo

EINVAL = -1
N_SAMP = 70
LENGTHS = (0, 1, 15, 16, 17, 33, N_SAMP)
GROUP_COUNTS = (1, 2, 5, 26, 64)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_curve(cols, group_of, n_groups, order, n_var, private=True):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    groups, idx = np.ascontiguousarray(group_of, dtype=np.int32), np.ascontiguousarray(order, dtype=np.uint32)
    n = len(idx)
    new, total = np.full((n_groups, n), -7, np.int64), np.full(n_groups, -7, np.int64)
    priv, ptotal = (np.full((n_groups, n), -7, np.int64), np.full(n_groups, -7, np.int64)) if private else (None, None)
    nat.check(nat.lib().utm_group_curve_host(_p(cols), cols.shape[1], n_var, cols.shape[0], _p(groups), n_groups,
                                             _p(idx) if n else None, n, _p(new) if n else None, _p(priv) if n else None,
                                             _p(total), _p(ptotal)))
    return new, priv, total, ptotal


def labels(rng, n_samp, n_groups, ungrouped=True):
    """A group id per sample: every id but the last one has a member where there are samples enough (the last id stays
    without samples when n_groups > 1), a few samples in no group."""
    used = max(1, n_groups - 1)
    group_of = rng.integers(0, used, size=n_samp).astype(np.int32)
    group_of[rng.permutation(n_samp)[:min(used, n_samp)]] = np.arange(min(used, n_samp))
    if ungrouped:
        group_of[rng.permutation(n_samp)[:5]] = -1
    return group_of


@functools.lru_cache(maxsize=None)
def matrix(n_var, fill):
    rng = np.random.default_rng(n_var * 3 + len(fill))
    if fill == "sparse":
        dense = ou.random_dense(rng, n_var, N_SAMP)
    else:
        dense = ou.random_dense(rng, n_var, N_SAMP, density=0.9, sfs=False)
    dense.setflags(write=False)
    return dense


def check(dense, group_of, n_groups, order, tag):
    n_var = dense.shape[0]
    cols = npo.pack_columns(dense)
    want = group_ref.group_curve_dense(dense, group_of, n_groups, order)
    got = host_curve(cols, group_of, n_groups, order, n_var)
    for g, w in zip(got, want):
        assert g.shape == w.shape and (g == w).all(), tag
    new, _, total, _ = host_curve(cols, group_of, n_groups, order, n_var, private=False)      # private off: the same bins
    assert (new == want[0]).all() and (total == want[2]).all(), tag
    assert (want[0].sum(axis=1) <= want[2]).all() and (want[1].sum(axis=1) <= want[3]).all()
    return want


# ----------------------------------------------------------------- 1. the CPU build against the restatement
@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 8191, 8192, 8193])
def test_cpu_build_equals_the_restatement(n_var, n_groups, fill):
    dense = matrix(n_var, fill)
    rng = np.random.default_rng(n_var + n_groups)
    group_of = labels(rng, N_SAMP, n_groups)
    perm = rng.permutation(N_SAMP)
    for n in LENGTHS:
        new, priv, total, ptotal = check(dense, group_of, n_groups, perm[:n], (n_var, n_groups, fill, n))
        if n_groups > 1:
            assert total[n_groups - 1] == 0 and (new[n_groups - 1] == 0).all()       # the id without samples
        if n == 0:
            assert new.shape == (n_groups, 0) and total.sum() > 0


def test_a_first_sample_that_carries_everything_takes_every_bin():
    n_var = 8193
    dense = matrix(n_var, "sparse").copy()
    dense[:, 11] = True
    rng = np.random.default_rng(4)
    group_of = labels(rng, N_SAMP, 5)
    order = np.concatenate([[11], np.delete(np.arange(N_SAMP), 11)])
    new, priv, total, ptotal = check(dense, group_of, 5, order, "all in one")
    assert (new[:, 0] == total).all() and (new[:, 1:] == 0).all() and (priv[:, 0] == ptotal).all()


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_every_sample_grouped_and_listed_captures_every_total(n_groups):
    dense = matrix(8193, "sparse")
    rng = np.random.default_rng(n_groups)
    group_of = (rng.permutation(N_SAMP) % n_groups).astype(np.int32)
    new, priv, total, ptotal = check(dense, group_of, n_groups, rng.permutation(N_SAMP), n_groups)
    assert (new.sum(axis=1) == total).all() and (priv.sum(axis=1) == ptotal).all()
    if n_groups == 1:
        assert (priv == new).all() and total[0] == dense.shape[0]


def test_ungrouped_samples_capture_but_own_nothing():
    dense = matrix(8192, "sparse")
    group_of = np.full(N_SAMP, -1, np.int32)
    group_of[:10] = 0
    group_of[10:20] = 1
    order = np.arange(N_SAMP)[::-1]                     # the ungrouped samples come first and capture for the groups
    new, priv, total, ptotal = check(dense, group_of, 2, order, "ungrouped first")
    assert new[:, :50].sum() > 0 and (ptotal <= total).all()


# ----------------------------------------------------------------- 2. refusals that need no device
def test_cpu_build_refuses_bad_arguments_and_leaves_the_outputs():
    from utmos_amd import _native as nat
    lib = nat.lib()
    n_var, n_samp = 100, 6
    cols = npo.pack_columns(ou.random_dense(np.random.default_rng(1), n_var, n_samp))
    new, priv, total, ptotal = (np.full(s, 1234, np.int64) for s in ((3, 2), (3, 2), 3, 3))
    good_groups = np.asarray([0, 1, 2, -1, 0, 1], np.int32)

    def call(groups=good_groups, n_groups=3, order=(4, 1), n=None, t=total, nw=new, n_var=n_var, c=cols):
        order = None if order is None else np.asarray(order, np.uint32)
        groups = None if groups is None else np.asarray(groups, np.int32)
        return lib.utm_group_curve_host(_p(c), cols.shape[1], n_var, n_samp, _p(groups), n_groups, _p(order),
                                        (0 if order is None else len(order)) if n is None else n, _p(nw), _p(priv), _p(t), _p(ptotal))

    assert call(groups=None) == EINVAL and call(t=None) == EINVAL and call(nw=None) == EINVAL
    assert call(order=None, n=2) == EINVAL
    assert call(n_groups=0) == EINVAL and call(n_groups=65) == EINVAL and call(n_groups=-1) == EINVAL
    assert call(groups=[0, 1, 3, -1, 0, 1]) == EINVAL and call(groups=[0, 1, -2, -1, 0, 1]) == EINVAL
    assert b"group" in lib.utm_last_error()
    assert call(order=(4, 6)) == EINVAL and call(order=(4, 4)) == EINVAL
    assert call(n_var=cols.shape[1] * 64 + 1) == EINVAL
    assert all((a == 1234).all() for a in (new, priv, total, ptotal))
    assert call() == 0
    want = group_ref.group_curve(cols, good_groups, 3, [4, 1], n_var)
    assert all((a == w).all() for a, w in zip((new, priv, total, ptotal), want))
    new[:] = 1234
    assert call(order=None, nw=None) == 0 and (new == 1234).all() and (total == want[2]).all()     # n == 0: the totals only


def test_the_abi_call_refuses_a_null_context():
    from utmos_amd import _native as nat
    assert nat.lib().utm_group_curve(None, 0, None, 1, None, 0, 0, None, None, None, None, None) == EINVAL


# ----------------------------------------------------------------- 3. the --groups file
def write(path, text):
    with open(path, "w") as fh:
        fh.write(text)
    return str(path)


def test_groups_are_numbered_by_first_appearance_among_known_samples(tmp_path, caplog):
    from utmos_amd import groups
    names = ["s0", "s1", "s2", "s3", "s4"]
    path = write(tmp_path / "g.tsv", "zz\tGHOST\ns3\tB\ns0\tA\n\ns1\tB\ns3\tB\nyy\tA\ns4\tC\textra\n")
    with caplog.at_level("INFO"):
        group_of, group_names = groups.parse_groups(path, names)
    assert group_names == ["B", "A", "C"] and group_of.dtype == np.int32
    assert group_of.tolist() == [1, 0, -1, 0, 2]
    counted = [r.getMessage() for r in caplog.records if "not in the input" in r.getMessage()]
    assert len(counted) == 1 and "2 listed names" in counted[0] and "3 groups" in counted[0]


def test_a_conflicting_duplicate_and_too_many_groups_exit_1(tmp_path, caplog):
    from utmos_amd import groups
    names = [f"s{i}" for i in range(70)]
    with pytest.raises(SystemExit) as err:
        groups.parse_groups(write(tmp_path / "dup.tsv", "s1\tA\ns2\tB\ns1\tB\n"), names)
    assert err.value.code == 1 and "s1" in caplog.text
    with pytest.raises(SystemExit) as err:
        groups.parse_groups(write(tmp_path / "many.tsv", "".join(f"s{i}\tG{i}\n" for i in range(65))), names)
    assert err.value.code == 1 and "65 groups" in caplog.text
    group_of, group_names = groups.parse_groups(write(tmp_path / "ok.tsv", "".join(f"s{i}\tG{i}\n" for i in range(64))), names)
    assert len(group_names) == 64 and group_of[:64].tolist() == list(range(64)) and (group_of[64:] == -1).all()


# ----------------------------------------------------------------- 4. the quota's bookkeeping
def test_no_group_can_fill_sooner_than_the_run_length():
    from utmos_amd import groups
    group_of = np.asarray([0, 0, 0, 1, 1, 2, -1, -1], np.int32)
    states = np.ones(8, np.uint8)
    taken = np.asarray([1, 0, 0])
    assert groups.quota_run_length(states, group_of, taken, 3, 10) == 2          # group 0 has room for two
    assert groups.quota_run_length(states, group_of, taken, 3, 1) == 1           # never more than what is left
    states[:3] = 2                                                              # group 0 has no selectable member left
    assert groups.quota_run_length(states, group_of, taken, 3, 10) == 3
    states[:6] = 0                                                              # only ungrouped samples remain
    assert groups.quota_run_length(states, group_of, taken, 3, 10) == 10
    # closing: the selectable rest of a full group becomes excluded, used samples and other groups stay
    states = np.asarray([0, 1, 1, 1, 0, 1, 1, 2], np.uint8)
    groups.close_full_groups(states, group_of, np.asarray([1, 1, 0]), 1)
    assert states.tolist() == [0, 2, 2, 2, 0, 1, 1, 2]
    assert groups.group_taken(group_of, 3, [0, 4, 6, 1]).tolist() == [2, 1, 0]
    # every run of a simulated selection ends before any group holds more than Q
    rng = np.random.default_rng(3)
    for quota in (1, 2, 3):
        group_of = rng.integers(-1, 4, size=40).astype(np.int32)
        states, taken, left = np.ones(40, np.uint8), np.zeros(4, np.int64), 25
        while left > 0:
            groups.close_full_groups(states, group_of, taken, quota)
            run = groups.quota_run_length(states, group_of, taken, quota, left)
            picks = rng.permutation(np.flatnonzero(states == 1))[:run]
            if len(picks) == 0:
                break
            assert run >= 1
            states[picks] = 0
            taken += groups.group_taken(group_of, 4, picks)
            assert (taken <= quota).all()
            left -= len(picks)
        assert left == 0 or not (states == 1).any()


def test_a_fixed_order_skips_the_samples_of_a_full_group():
    from utmos_amd import groups
    group_of = np.asarray([0, 0, 1, -1, 0, 1, -1], np.int32)
    assert groups.quota_filter([0, 1, 2, 3, 4, 5, 6], group_of, [0, 0], 1, 10).tolist() == [0, 2, 3, 6]
    assert groups.quota_filter([0, 1, 2, 3, 4, 5, 6], group_of, [1, 0], 2, 3).tolist() == [0, 2, 3]
    assert groups.quota_filter([4, 1], group_of, [2, 0], 2, 5).tolist() == []


# ----------------------------------------------------------------- 5. the text of --groups-out
def test_the_tsv_text():
    from utmos_amd import groups
    new = np.asarray([[3, 0, 1], [0, 0, 0]], np.int64)
    priv = np.asarray([[1, 0, 1], [0, 0, 0]], np.int64)
    text = groups.group_lines(["a", "b", "c"], ["P", "Q"], new, priv, np.asarray([6, 0]), np.asarray([3, 0]))
    assert groups.GROUPS_HEADER == "k\tsample\tgroup\tnew\tcaptured\tpct_captured\tprivate_new\tprivate_captured\tprivate_pct\n"
    assert text == ("1\ta\tP\t3\t3\t0.5\t1\t1\t0.3333\n"
                    "1\ta\tQ\t0\t0\t0.0\t0\t0\t0.0\n"
                    "2\tb\tP\t0\t3\t0.5\t0\t1\t0.3333\n"
                    "2\tb\tQ\t0\t0\t0.0\t0\t0\t0.0\n"
                    "3\tc\tP\t1\t4\t0.6667\t1\t2\t0.6667\n"
                    "3\tc\tQ\t0\t0\t0.0\t0\t0\t0.0\n")
    assert groups.group_lines([], ["P"], new[:1, :0], priv[:1, :0], [6], [3]) == ""


# ----------------------------------------------------------------- 6. the command line
@pytest.mark.parametrize("argv,word", [
    (["--groups-out", "g.tsv"], "--groups"),
    (["--group-max", "2"], "--groups"),
    (["--groups", "g.txt", "--group-max", "0"], "at least 1"),
    (["--groups", "g.txt", "--depth", "2"], "--depth"),
    (["--groups", "g.txt", "--groups-out", "o.tsv", "--refine", "3"], "--refine"),
])
def test_unusable_combinations_exit_1(argv, word, capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as err:
        select.parse_args(argv + ["x.npz"])
    assert err.value.code == 1 and word in capsys.readouterr().err


@pytest.mark.parametrize("extra", [[], ["--groups-out", "o.tsv"], ["--group-max", "2"]])
def test_several_processes_refuse_groups_before_loading(extra, monkeypatch, capsys, tmp_path):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--groups", write(tmp_path / "g.txt", "a\tA\n")] + extra + ["does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_the_options_default_to_off_and_are_not_in_the_options_line_then(capsys):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])
    assert args.groups is None and args.groups_out is None and args.group_max is None
    line = capsys.readouterr().err
    assert "options in effect" in line and "group" not in line
    select.parse_args(["--groups", "g.txt", "--group-max", "3", "--groups-out", "o.tsv", "x.npz"])
    line = capsys.readouterr().err
    assert '"groups": "g.txt"' in line and '"group_max": 3' in line and '"groups_out": "o.tsv"' in line


def test_an_include_list_beyond_the_quota_exits_1(caplog):
    from utmos_amd import select

    class Shape:
        shape = (10, 4)

    data = {"data": Shape(), "samples": ["a", "b", "c", "d"], "var_count": [1, 1, 1, 1]}
    with pytest.raises(SystemExit) as err:
        select.run_selection(data, 3, include=["a", "c"], group_of=[0, 1, 0, -1], group_max=1)
    assert err.value.code == 1 and "--group-max 1" in caplog.text


# ----------------------------------------------------------------- 7. the quota's control flow over a numpy stand-in
class NumpyMatrix:
    """What select's row generators ask of a DeviceMatrix (states, weights, reset, run, apply_order, peek_scores), in
    numpy over a dense bool matrix: the plain greedy and nothing of the quota, which is all the device knows of either."""
    coverage_depth = 1

    def __init__(self, dense):
        self.dense, self.shape = np.asarray(dense, dtype=bool), dense.shape
        self.weights = np.ones(dense.shape[1])
        self.resets = 0

    def set_state(self, states):
        self.states = np.array(states, dtype=np.uint8)

    def set_weights(self, weights):
        self.weights = np.ones(self.shape[1]) if weights is None else np.asarray(weights, dtype=np.float64)

    def reset(self):
        self.covered = self.dense[:, self.states == 0].any(axis=1)
        self.resets += 1

    def peek_scores(self):
        counts = np.where(self.states == 1, (self.dense & ~self.covered[:, None]).sum(axis=0), 0)
        return counts, counts * self.weights

    def run(self, k):
        winners, gains = [], []
        while len(winners) < k and not self.covered.all():
            counts, scores = self.peek_scores()
            best = int(np.argmax(scores))
            if scores[best] <= 0:
                break
            winners.append(best)
            gains.append(counts[best])
            self.covered |= self.dense[:, best]
            self.states[best] = 0
        return np.asarray(winners, np.int64), np.asarray(gains, np.int64), np.zeros(len(winners))

    def apply_order(self, order):
        gains = []
        for s in order:
            gains.append(int((self.dense[:, s] & ~self.covered).sum()))
            self.covered |= self.dense[:, s]
            self.states[s] = 0
            if self.covered.all():
                break
        return np.asarray(gains, np.int64)


@pytest.mark.parametrize("quota", [1, 2, 5])
def test_the_restarted_greedy_is_the_greedy_over_the_groups_that_are_not_full(quota):
    from utmos_amd import select
    rng = np.random.default_rng(quota)
    n_var, n_samp, k = 3000, 60, 14
    dense = ou.random_dense(rng, n_var, n_samp)
    names = [f"s{i}" for i in range(n_samp)]
    group_of = (np.arange(n_samp) % 4).astype(np.int32)
    group_of[3::11] = -1
    weights = {names[i]: 2.5 for i in range(0, n_samp, 7)}
    vector = np.asarray([weights.get(n, 1.0) for n in names])
    states = np.ones(n_samp, np.uint8)
    states[[1, 2]] = 2
    first = group_ref.greedy_with_quota(dense, states, None, group_of, quota, 1)[0][0]
    same = [i for i in range(n_samp) if group_of[i] == group_of[first] and i != first and states[i] == 1][0]
    for kw, want in (
            ({}, group_ref.greedy_with_quota(dense, states, None, group_of, quota, k)),
            ({"weights": weights}, group_ref.greedy_with_quota(dense, states, vector, group_of, quota, k)),
            ({"include": [names[same]]}, group_ref.greedy_with_quota(dense, states, None, group_of, quota, k, [same])),
            ({"mode": "topN"}, group_ref.topn_with_quota(dense, states, None, group_of, quota, k)),
            ({"mode": "topN", "include": [names[same]], "weights": weights}, group_ref.topn_with_quota(dense, states, vector, group_of, quota, k, [same]))):
        matrix = NumpyMatrix(dense)
        data = {"data": matrix, "samples": names, "var_count": dense.sum(axis=0)}
        rows = list(select.run_selection(data, k, exclude=[names[1], names[2]], group_of=group_of, group_max=quota, **kw))
        assert [(names.index(r[0]), r[2]) for r in rows] == want, kw
        assert [r[3] for r in rows] == np.cumsum([w[1] for w in want]).tolist()
        picked = group_of[[names.index(r[0]) for r in rows]]
        assert (np.bincount(picked[picked >= 0], minlength=4) <= quota).all()
        if "mode" not in kw and quota == 1:
            assert matrix.resets >= 3                                    # a restart for every group that fills
    # a quota nobody reaches: one run of the loop, the rows of the plain selection
    plain = list(select.run_selection({"data": NumpyMatrix(dense), "samples": names, "var_count": dense.sum(axis=0)}, k))
    matrix = NumpyMatrix(dense)
    capped = list(select.run_selection({"data": matrix, "samples": names, "var_count": dense.sum(axis=0)}, k, group_of=group_of,
                                       group_max=n_samp))
    assert capped == plain and matrix.resets == 1
