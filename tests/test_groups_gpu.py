"""GPU: group curves through the C ABI (utm_group_curve: k_group_unions + k_group_curve), DeviceMatrix.group_curve and
`select --groups / --groups-out / --group-max`.

The bins and totals are held against the numpy restatement by definition (tests/group_ref.py) and the CPU build of the
kernels' word arithmetic, value for value.  The shapes sit on the kernels' edges: one wave's KiB and one 4 KiB tile +- 1
bit, several tiles with a last one a single wave wide, lists of one round (16 columns) +- 1, group counts from one to the
64 the ABI admits, and lists longer than the LDS head so that both kinds of bins are hit in one call."""
import ctypes
import functools
import os

import numpy as np
import pytest

import group_ref
import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements
GROUP_COUNTS = (1, 2, 5, 26, 64)
LDS_BINS = 8192                               # UTM_GROUP_LDS_BINS
MODES = ((0, True), (1, True), (2, True), (0, False), (1, False), (2, False))     # (bin_mode, private)


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


@functools.lru_cache(maxsize=None)
def seeded(n_var, n_samp):
    rng = np.random.default_rng(n_var * 7 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    dense.setflags(write=False)
    return dense


def lengths(n_samp):
    return (0, 1, 15, 16, 17, 33, n_samp)


def labels(rng, n_samp, n_groups):
    """Every id but the last has a member (the last one stays without samples when n_groups > 1); five samples in no group."""
    used = max(1, n_groups - 1)
    group_of = rng.integers(0, used, size=n_samp).astype(np.int32)
    group_of[rng.permutation(n_samp)[:used]] = np.arange(used)
    group_of[rng.permutation(n_samp)[:5]] = -1
    return group_of


def host_curve(cols, group_of, n_groups, order, n_var):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    groups, idx = np.ascontiguousarray(group_of, dtype=np.int32), np.ascontiguousarray(order, dtype=np.uint32)
    n = len(idx)
    new, priv = np.zeros((n_groups, n), np.int64), np.zeros((n_groups, n), np.int64)
    total, ptotal = np.zeros(n_groups, np.int64), np.zeros(n_groups, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    nat.check(nat.lib().utm_group_curve_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(groups), n_groups, p(idx), n,
                                             p(new), p(priv), p(total), p(ptotal)))
    return new, priv, total, ptotal


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def check_all_modes(mat, want, group_of, n_groups, order, tag=None):
    """Every bin_mode, with and without the private bins, against `want` = (new, priv, total, ptotal)."""
    for mode, private in MODES:
        new, priv, total, ptotal = mat.group_curve(group_of, n_groups, order, private=private, bin_mode=mode)
        assert new.dtype == np.int64 and new.shape == (n_groups, len(order)) and total.shape == (n_groups,)
        assert (new == want[0]).all() and (total == want[2]).all(), (tag, mode, private)
        if private:
            assert (priv == want[1]).all() and (ptotal == want[3]).all(), (tag, mode)
        else:
            assert priv is None and ptotal is None


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_samp", [70, 300])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 8192, 8193, 32767, 32768, 32769, 3 * 32768 + 5])
def test_bins_equal_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    rng = np.random.default_rng(n_var + n_samp)
    perm = rng.permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for n_groups in GROUP_COUNTS:
            group_of = labels(rng, n_samp, n_groups)
            # the restatement once per labelling: a variant's first carrier in a prefix of the list is its first carrier
            # in the list where that stands inside the prefix, so a prefix's bins are the first n columns of the list's
            # (tests/test_groups_host.py holds every prefix against the restatement itself)
            full = group_ref.group_curve_dense(dense, group_of, n_groups, perm)
            for n in lengths(n_samp):
                want = (full[0][:, :n], full[1][:, :n], full[2], full[3])
                host = host_curve(cols, group_of, n_groups, perm[:n], n_var)
                assert all((h == w).all() for h, w in zip(host, want)), (n_groups, n)
                check_all_modes(mat, want, group_of, n_groups, perm[:n], (n_groups, n))
                assert (want[0].sum(axis=1) <= want[2]).all()


@pytest.mark.parametrize("n_groups,private", [(64, True), (64, False), (26, True)])
def test_a_list_longer_than_the_lds_head_hits_both_kinds_of_bins(dev, n_groups, private):
    n_var, n_samp = 32769 + 4096, 300
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    rng = np.random.default_rng(n_groups)
    group_of = (rng.permutation(n_samp) % n_groups).astype(np.int32)         # every sample grouped, every id used
    order = rng.permutation(n_samp)
    head = LDS_BINS // (2 * n_groups if private else n_groups)               # R: 64, 128, 157
    assert head < n_samp
    want = group_ref.group_curve_dense(dense, group_of, n_groups, order)
    assert want[0][:, :head].sum() > 0 and want[0][:, head:].sum() > 0 and want[1][:, head:].sum() > 0
    assert (want[0].sum(axis=1) == want[2]).all() and (want[1].sum(axis=1) == want[3]).all()    # everybody grouped and listed
    with uploaded(dev, [cols], [n_var]) as mat:
        for mode in (0, 1, 2):
            got = mat.group_curve(group_of, n_groups, order, private=private, bin_mode=mode)
            assert (got[0] == want[0]).all() and (got[2] == want[2]).all(), mode
            if private:
                assert (got[1] == want[1]).all() and (got[3] == want[3]).all(), mode


def test_a_dense_matrix_whose_first_listed_sample_carries_everything(dev):
    rng = np.random.default_rng(8)
    n_var, n_samp = 33000, 70
    dense = ou.random_dense(rng, n_var, n_samp, density=0.9, sfs=False)
    dense[:, 7] = True
    cols = npo.pack_columns(dense)
    order = np.concatenate([[7], np.delete(np.arange(n_samp), 7)])
    with uploaded(dev, [cols], [n_var]) as mat:
        for n_groups in (1, 5, 64):
            group_of = labels(rng, n_samp, n_groups)
            want = group_ref.group_curve_dense(dense, group_of, n_groups, order)
            assert (want[0][:, 0] == want[2]).all() and (want[0][:, 1:] == 0).all()
            check_all_modes(mat, want, group_of, n_groups, order, n_groups)
        group_of = np.zeros(n_samp, np.int32)                                # one group of everybody: private == all
        new, priv, total, ptotal = mat.group_curve(group_of, 1, order[::-1])
        assert (priv == new).all() and total[0] == ptotal[0] == n_var == new.sum()


def test_two_chunks_of_unequal_size_add_up(dev):
    chunk_vars, n_samp = [32769, 100], 200
    dense = seeded(sum(chunk_vars), n_samp)
    cols = [npo.pack_columns(dense[:32769]), npo.pack_columns(dense[32769:])]
    rng = np.random.default_rng(2)
    group_of = labels(rng, n_samp, 5)
    with uploaded(dev, cols, chunk_vars) as mat:
        for n in (0, 1, 17, 200):
            order = rng.permutation(n_samp)[:n]
            want = group_ref.group_curve_dense(dense, group_of, 5, order)
            check_all_modes(mat, want, group_of, 5, order, n)
            parts = [host_curve(c, group_of, 5, order, v) for c, v in zip(cols, chunk_vars)]
            assert all((a + b == w).all() for a, b, w in zip(parts[0], parts[1], want))
        got = mat.group_curve(group_of, 5, rng.permutation(n_samp), pass_ms=True)
        assert len(got) == 5 and got[4] > 0


def test_rows_cleared_by_an_af_of_zero_have_no_carriers(dev):
    rng = np.random.default_rng(5)
    n_var, n_samp = 33000, 70
    dense = ou.random_dense(rng, n_var, n_samp)
    af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0
    zero = rng.random(n_var) < 0.05
    zero[[0, 63, 64, n_var - 1]] = True
    af[zero] = 0.0
    group_of = labels(rng, n_samp, 5)
    order = rng.permutation(n_samp)[:66]
    want = group_ref.group_curve_dense(dense & ~zero[:, None], group_of, 5, order)
    assert want[2].sum() < group_ref.group_curve_dense(dense, group_of, 5, order)[2].sum()
    with dev.DeviceMatrix(n_samp) as mat:
        c = mat.add_chunk(n_var)
        mat.upload_columns(c, npo.pack_columns(dense))
        mat.set_af(c, af.astype(np.float64))
        check_all_modes(mat, want, group_of, 5, order, "af")


# ----------------------------------------------------------------- 2. stateless
def test_a_call_in_between_changes_nothing_of_the_selection(dev):
    rng = np.random.default_rng(21)
    n_var, n_samp = 40_000, 120
    dense = ou.random_dense(rng, n_var, n_samp)
    chunk_vars = [25_000, 15_000]
    cols = [npo.pack_columns(dense[:25_000]), npo.pack_columns(dense[25_000:])]
    state = np.ones(n_samp, np.uint8)
    state[[2, 50]] = 0
    state[[9, 10]] = 2
    group_of = labels(rng, n_samp, 5)
    a, b = uploaded(dev, cols, chunk_vars), uploaded(dev, cols, chunk_vars)
    with a, b:
        before = a.group_curve(group_of, 5, [2, 9, 30])                  # valid before any reset
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        order = list(dict.fromkeys([int(s) for s in first[0]] + [2, 9] + list(range(60, 120))))   # winners, a used and an excluded sample
        check_all_modes(a, group_ref.group_curve_dense(dense, group_of, 5, order), group_of, 5, order, "between")
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        after = a.group_curve(group_of, 5, [2, 9, 30])                   # and the selection changes nothing of the curves
        assert all((x == y).all() for x, y in zip(before, after))


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_the_outputs(dev):
    n_var, n_samp = 9000, 30
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    lib = dev.nat.lib()
    good = (np.arange(n_samp) % 4 - 1).astype(np.int32)                  # -1 .. 2
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        new, priv = np.full((3, 3), 1234, np.int64), np.full((3, 3), 1234, np.int64)
        total, ptotal = np.full(3, 1234, np.int64), np.full(3, 1234, np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

        def call(idx=(7, 8, 1), groups=good, n_groups=3, n=None, chunk=0, mode=0, nw=new, pv=priv, t=total, pt=ptotal):
            idx = None if idx is None else np.asarray(idx, dtype=np.int64)
            groups = None if groups is None else np.asarray(groups, dtype=np.int32)
            return lib.utm_group_curve(mat._h, chunk, p(groups), n_groups, p(idx), (0 if idx is None else len(idx)) if n is None else n,
                                       mode, p(nw), p(pv), p(t), p(pt), None)

        assert call(groups=None) == EINVAL and call(t=None) == EINVAL and call(nw=None) == EINVAL     # NULL arguments
        assert call(idx=None, n=2) == EINVAL and call(n=-1) == EINVAL
        assert call(n_groups=0) == EINVAL and call(n_groups=65) == EINVAL and call(n_groups=-3) == EINVAL
        assert call(n_groups=2) == EINVAL                                # a group id of 2 with two groups
        bad = good.copy()
        bad[4] = -2
        assert call(groups=bad) == EINVAL
        assert call(chunk=1) == EINVAL and call(chunk=-1) == EINVAL
        assert call(idx=(1, 30, 2)) == EINVAL and call(idx=(-1, 2, 3)) == EINVAL      # index out of range
        assert call(idx=(4, 5, 4)) == EINVAL                             # a duplicate in the order
        assert call(mode=3) == EINVAL
        assert all((a == 1234).all() for a in (new, priv, total, ptotal))
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        want = group_ref.group_curve_dense(dense, good, 3, [7, 8, 1])
        assert call() == 0 and all((a == w).all() for a, w in zip((new, priv, total, ptotal), want))
        new[:], priv[:], total[:], ptotal[:] = 1234, 1234, 1234, 1234
        assert call(pv=None, pt=None) == 0 and (new == want[0]).all() and (total == want[2]).all()
        assert (priv == 1234).all() and (ptotal == 1234).all()           # not asked for: not written
        new[:], total[:] = 1234, 1234
        assert call(idx=None, nw=None) == 0 and (total == want[2]).all() and (ptotal == want[3]).all()   # n == 0: the totals only
        assert (new == 1234).all() and (priv == 1234).all()
        ms = ctypes.c_double(-1.0)
        idx = np.asarray([7, 8, 1], dtype=np.int64)
        assert lib.utm_group_curve(mat._h, 0, p(good), 3, p(idx), 3, 0, p(new), None, p(total), None, ctypes.byref(ms)) == 0 and ms.value > 0
        assert (new == want[0]).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.group_curve(np.zeros(10, np.int32), 1, [3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


# ----------------------------------------------------------------- 4. select --groups-out
def gold(name):
    return os.path.join(ou.GOLD, name)


def write_groups(path, names, group_of, label="G%d"):
    with open(path, "w") as fh:
        for name, g in zip(names, group_of):
            if g >= 0:
                fh.write(f"{name}\t{label % g}\n")
    return str(path)


def read_tsv(path):
    lines = open(path).read().splitlines()
    return [line.split("\t") for line in lines[1:]]


def expected_groups_text(rows, group_names, new, priv, total, ptotal):
    from utmos_amd import groups
    pct = lambda part, whole: round(int(part) / int(whole), 4) if whole else 0.0
    text = groups.GROUPS_HEADER
    for k, sample in enumerate(rows):
        for g, group in enumerate(group_names):
            c, pc = int(new[g, :k + 1].sum()), int(priv[g, :k + 1].sum())
            text += f"{k + 1}\t{sample}\t{group}\t{new[g, k]}\t{c}\t{pct(c, total[g])}\t{priv[g, k]}\t{pc}\t{pct(pc, ptotal[g])}\n"
    return text


def test_one_group_of_everybody_repeats_the_tsv_s_own_curve(dev, tmp_path):
    from utmos_amd.select import select_main
    case = ou.golden_cases()["select_multi"]
    names = [str(s) for s in ou.load_part(case["inputs"][0])["samples"]]
    groups_file = write_groups(tmp_path / "one.txt", names, np.zeros(len(names), int), "ALL%d")
    out, gout = str(tmp_path / "out.txt"), str(tmp_path / "groups.tsv")
    select_main(["--groups", groups_file, "--groups-out", gout, "-o", out] + [gold(n + ".npz") for n in case["inputs"]])
    assert open(out).read() == ou.golden_text(case)                      # the TSV is what it was
    rows, grows = read_tsv(out), read_tsv(gout)
    assert len(rows) == len(grows) > 10
    for k, (row, grow) in enumerate(zip(rows, grows)):
        assert grow[:3] == [str(k + 1), row[0], "ALL0"]
        assert grow[3] == row[2] and grow[4] == row[3]                   # new and captured are the TSV's own columns
        assert abs(float(grow[5]) - float(row[4])) < 1.5e-4              # (each rounds captured / total to 4 places itself)
        assert grow[6:] == grow[3:6]                                     # one group: everything is private


def test_three_groups_under_a_subset_and_an_include_prefix(dev, tmp_path):
    from utmos_amd.select import select_main
    inputs = ("chunk0", "chunk1", "chunk2")
    parts = [ou.load_part(n) for n in inputs]
    matrix, _, samples = npo.build_matrix(parts)                         # from the ORIGINAL part files
    dense = np.asarray(matrix) != 0
    names = [str(s) for s in samples]
    group_of = np.arange(len(names)) % 3
    group_of[5::7] = -1                                                  # some samples in no group
    groups_file = write_groups(tmp_path / "three.txt", names, group_of)
    with open(groups_file, "a") as fh:
        fh.write("NOBODY\tG9\n")                                         # a name the input lacks: ignored
    include = [names[40], names[300]]                                    # names[300] is outside the subset below
    out, gout = str(tmp_path / "out.txt"), str(tmp_path / "groups.tsv")
    select_main(["--groups", groups_file, "--groups-out", gout, "-o", out, "-c", "12", "--subset", gold("subset.txt"),
                 "--include", ",".join(include), "--maxmem", "0", "--buffer", "640"] + [gold(n + ".npz") for n in inputs])
    rows = [r[0] for r in read_tsv(out)]
    assert rows[:2] == include and len(rows) == 12 and names[300] not in ou.read_list(gold("subset.txt"))
    order = [names.index(s) for s in rows]
    # groups are numbered by first appearance in the file: G0, G1, G2 (sample 0, 1, 2)
    want = group_ref.group_curve_dense(dense, group_of, 3, order)
    assert open(gout).read() == expected_groups_text(rows, ["G0", "G1", "G2"], *want)
    assert want[0].sum() > 0 and (want[1].sum(axis=1) < want[0].sum(axis=1)).all()


# ----------------------------------------------------------------- 5. select --group-max
def quota_case(tmp_path, inputs, n_groups=3):
    parts = [ou.load_part(n) for n in inputs]
    matrix, _, samples = npo.build_matrix(parts)
    names = [str(s) for s in samples]
    group_of = np.arange(len(names)) % n_groups
    group_of[4::9] = -1
    return np.asarray(matrix) != 0, names, group_of, write_groups(tmp_path / "groups.txt", names, group_of)


def run_quota(tmp_path, inputs, groups_file, extra):
    from utmos_amd.select import select_main
    out = str(tmp_path / "quota.txt")
    select_main(["--groups", groups_file, "-o", out] + list(extra) + [gold(n + ".npz") for n in inputs])
    return read_tsv(out)


@pytest.mark.parametrize("name", ["select_intcnt", "select_weights"])
def test_a_quota_nobody_reaches_reproduces_the_plain_tsv(dev, tmp_path, name):
    from utmos_amd.select import select_main
    case = ou.golden_cases()[name]
    _, names, _, groups_file = quota_case(tmp_path, case["inputs"])
    argv = [gold(a) if a == "weights.txt" else a for a in case["args"]]
    out = str(tmp_path / "out.txt")
    select_main(argv + ["--groups", groups_file, "--group-max", str(len(names)), "-o", out] + [gold(n + ".npz") for n in case["inputs"]])
    assert open(out).read() == ou.golden_text(case)


@pytest.mark.parametrize("inputs", [("mid",), ("chunk0", "chunk1")])
@pytest.mark.parametrize("quota", [1, 2])
def test_the_quota_equals_the_restated_greedy(dev, tmp_path, quota, inputs):
    dense, names, group_of, groups_file = quota_case(tmp_path, inputs)
    states = np.ones(len(names), np.uint8)
    weights = np.ones(len(names))
    for name, w in ou.read_weights(gold("weights.txt")).items():
        if name in names:
            weights[names.index(name)] = w
    if inputs == ("mid",):                                               # (the weights file names 1000G samples)
        weights[::5] = 3.0
    weights_file = str(tmp_path / "w.txt")
    with open(weights_file, "w") as fh:
        fh.writelines(f"{n}\t{w}\n" for n, w in zip(names, weights) if w != 1.0)
    first = group_ref.greedy_with_quota(dense, states, None, group_of, quota, 1)[0][0]
    same = [i for i in range(len(names)) if group_of[i] == group_of[first] and i != first][0]
    other = [i for i in range(len(names)) if group_of[i] not in (-1, group_of[first])][0]
    include = [same, other] if quota == 1 else [same, first]             # Q = 2: the prefix fills a group at once
    k = 8
    for extra, want in (
            ([], group_ref.greedy_with_quota(dense, states, None, group_of, quota, k)),
            (["--weights", weights_file], group_ref.greedy_with_quota(dense, states, weights, group_of, quota, k)),
            (["--include", ",".join(names[i] for i in include)], group_ref.greedy_with_quota(dense, states, None, group_of, quota, k, include)),
            (["--mode", "topN"], group_ref.topn_with_quota(dense, states, None, group_of, quota, k)),
            (["--mode", "topN", "--include", names[same]], group_ref.topn_with_quota(dense, states, None, group_of, quota, k, [same]))):
        rows = run_quota(tmp_path, inputs, groups_file, ["-c", str(k), "--group-max", str(quota)] + extra)
        assert [(names.index(r[0]), int(r[2])) for r in rows] == want, extra
        assert [int(r[3]) for r in rows] == np.cumsum([w[1] for w in want]).tolist()
        picked = group_of[[names.index(r[0]) for r in rows]]
        assert len(rows) == k
        assert (np.bincount(picked[picked >= 0], minlength=3) <= quota).all(), extra
    # without ungrouped samples the quota ends the selection: three groups of Q
    grouped_only = ",".join(n for n, g in zip(names, group_of) if g >= 0)
    rows = run_quota(tmp_path, inputs, groups_file, ["-c", str(k), "--group-max", str(quota), "--subset", grouped_only])
    states = np.where(group_of >= 0, 1, 2).astype(np.uint8)
    assert [(names.index(r[0]), int(r[2])) for r in rows] == group_ref.greedy_with_quota(dense, states, None, group_of, quota, k)
    assert len(rows) == 3 * quota


def test_an_include_list_beyond_the_quota_exits_1(dev, tmp_path, capfd):
    from utmos_amd.select import select_main
    _, names, group_of, groups_file = quota_case(tmp_path, ("tiny",))
    pair = [n for n, g in zip(names, group_of) if g == 0][:2]
    with pytest.raises(SystemExit) as err:
        select_main(["--groups", groups_file, "--group-max", "1", "--include", ",".join(pair), "-o", str(tmp_path / "o.txt"),
                     gold("tiny.npz")])
    assert err.value.code == 1 and "--group-max 1" in capfd.readouterr().err
