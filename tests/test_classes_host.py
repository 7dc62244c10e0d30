"""Class counts without a GPU: the CPU build of k_class_counts' word walk (utm_class_counts_host) against the numpy
restatement by definition (tests/class_ref.py), the refusals of the ABI, and the pure functions behind
`select --samples-out / --represent-out`.  All counts are integers: every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

import class_ref
import oracle_util as ou
from oracle_util import npo

EINVAL = -1
CLASSES_MAX = 16384                           # UTM_CLASSES_MAX
CANARY = -77
N_VARS = (1, 63, 64, 65, 8191, 8192, 8193, 40_000)
N_SAMPS = (1, 5, 17)
N_CLASSES = (1, 2, 9, 300, CLASSES_MAX)
PATTERNS = ("one_class", "none", "gap", "random")


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_table(cols, n_var, class_of, n_classes, indices=None):
    """The CPU build's table of one chunk, canary-filled so that a cell that is not written shows."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    labels = np.ascontiguousarray(class_of, dtype=np.int32)
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rows = cols.shape[0] if idx is None else len(idx)
    table = np.full((rows, n_classes), CANARY, np.int64)
    nat.check(nat.lib().utm_class_counts_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(labels), n_classes, p(idx),
                                              0 if idx is None else len(idx), p(table)))
    return table


@functools.lru_cache(maxsize=None)
def columns(n_var, n_samp):
    rng = np.random.default_rng(31 * n_var + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp, density=0.3, sfs=False)
    dense[[0, n_var - 1]] = True                                         # the first and the last bit of every column
    cols = npo.pack_columns(dense)
    cols.setflags(write=False)
    return cols


def labels_of(pattern, n_var, n_classes, rng):
    if pattern == "one_class":
        return np.full(n_var, n_classes - 1, np.int32)
    if pattern == "none":
        return np.full(n_var, -1, np.int32)
    if pattern == "gap":                                                 # class 0 (where there is another) has no variant
        return rng.integers(min(1, n_classes - 1), n_classes, size=n_var).astype(np.int32)
    labels = rng.integers(0, n_classes, size=n_var).astype(np.int32)
    labels[rng.random(n_var) < 0.1] = -1
    return labels


# ----------------------------------------------------------------- the CPU build against the restatement
@pytest.mark.parametrize("n_samp", N_SAMPS)
@pytest.mark.parametrize("n_var", N_VARS)
def test_cpu_build_equals_the_restatement(n_var, n_samp):
    cols = columns(n_var, n_samp)
    rng = np.random.default_rng(n_var + n_samp)
    lists = [None, rng.permutation(n_samp)] + ([rng.permutation(n_samp)[:max(1, n_samp // 2)]] if n_samp > 1 else [])
    for n_classes in N_CLASSES:
        for pattern in PATTERNS:
            labels = labels_of(pattern, n_var, n_classes, rng)
            for indices in lists:                                        # NULL, a permutation, a strict subset
                got = host_table(cols, n_var, labels, n_classes, indices)
                want = class_ref.class_counts(cols, labels, n_classes, indices, n_var)
                assert got.dtype == np.int64 and got.shape == want.shape and (got == want).all(), (n_classes, pattern, indices)
                if pattern == "none":
                    assert not got.any()
                if pattern == "one_class":
                    order = range(n_samp) if indices is None else indices
                    assert got[:, -1].tolist() == [int(np.bitwise_count(cols[s]).sum()) for s in order] and not got[:, :-1].any()
                if pattern == "gap" and n_classes > 1:
                    assert not got[:, 0].any()


def test_the_hand_case():
    dense = np.zeros((6, 3), bool)                                       # A = {0,1,2,3}, B = {0,1,4}, C = {2,3,5}
    dense[[0, 1, 2, 3], 0] = True
    dense[[0, 1, 4], 1] = True
    dense[[2, 3, 5], 2] = True
    cols = npo.pack_columns(dense)
    labels = [0, 1, 1, -1, 2, 0]
    assert host_table(cols, 6, labels, 3).tolist() == [[1, 2, 0], [1, 1, 1], [1, 1, 0]]
    assert host_table(cols, 6, labels, 4, [2, 0]).tolist() == [[1, 1, 0, 0], [1, 2, 0, 0]]
    assert (host_table(cols, 6, labels, 3) == class_ref.class_counts_dense(dense, labels, 3)).all()


def test_padding_bits_and_variants_past_n_var_are_not_counted():
    cols = np.zeros((2, 2), np.uint64)
    cols[0, 0] = 0b0111
    cols[1, 1] = np.uint64(0b101)                                        # variants 64 and 66 of 67
    labels = np.zeros(67, np.int32)
    labels[66] = 1
    assert host_table(cols, 67, labels, 2).tolist() == [[3, 0], [1, 1]]
    assert host_table(cols, 66, labels[:66], 2).tolist() == [[3, 0], [1, 0]]      # bit 66 lies past n_var: no label, no count


# ----------------------------------------------------------------- refusals of the ABI
def test_cpu_build_refuses_bad_arguments_and_leaves_the_table():
    from utmos_amd import _native as nat
    lib = nat.lib()
    cols = np.zeros((4, 1), np.uint64)
    table = np.full((4, 3), CANARY, np.int64)
    good = np.zeros(10, np.int32)
    u32 = lambda a: None if a is None else np.asarray(a, np.uint32)

    def call(labels=good, n_classes=3, idx=None, n=0, out=table, n_var=10, n_samp=4):
        labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
        return lib.utm_class_counts_host(p(cols), 1, n_var, n_samp, p(labels), n_classes, p(u32(idx)), n, p(out))

    assert call(labels=None) == EINVAL                                   # NULL class_of
    assert call(out=None) == EINVAL                                      # NULL table_out
    assert call(idx=None, n=2) == EINVAL                                 # NULL list with a nonzero length
    assert call(n_classes=0) == EINVAL and call(n_classes=-1) == EINVAL and call(n_classes=CLASSES_MAX + 1) == EINVAL
    assert b"classes" in lib.utm_last_error()
    bad = good.copy()
    bad[9] = 3
    assert call(labels=bad) == EINVAL and b"class 3" in lib.utm_last_error()     # a label of n_classes
    bad[9] = -2
    assert call(labels=bad) == EINVAL and b"class -2" in lib.utm_last_error()    # ... below -1
    assert call(idx=[0, 4], n=2) == EINVAL and b"not in" in lib.utm_last_error()   # an index out of range
    assert call(idx=[1, 1], n=2) == EINVAL and b"twice" in lib.utm_last_error()    # a duplicate in the list
    assert call(n_var=65, labels=np.zeros(65, np.int32)) == EINVAL       # more variants than words
    assert call(idx=[0, 1, 2, 3, 0], n=5) == EINVAL                      # more listed than samples
    assert (table == CANARY).all()
    assert call() == 0 and not table.any()                               # an empty matrix: written, all zero
    i64 = np.zeros(3, np.int64)
    assert lib.utm_class_counts(None, 0, p(good), 3, None, 0, 0, 0, p(i64), None) == EINVAL and b"ctx" in lib.utm_last_error()


def test_the_largest_class_count_is_accepted():
    cols = columns(65, 5)
    labels = np.arange(65, dtype=np.int32) + (CLASSES_MAX - 65)
    got = host_table(cols, 65, labels, CLASSES_MAX)
    assert (got == class_ref.class_counts(cols, labels, CLASSES_MAX)).all() and got[:, -1].all()      # variant 64: everybody has it


# ----------------------------------------------------------------- select --samples-out / --represent-out: the pure parts
def test_rank_labels_map_never_captured_to_the_last_class():
    from utmos_amd import samples
    assert samples.rank_labels(np.asarray([0, -1, 2, 1, -1], np.int32), 3).tolist() == [0, 3, 2, 1, 3]
    assert samples.rank_labels(np.zeros(0, np.int32), 0).tolist() == []


def test_the_representation_table_of_a_hand_case(tmp_path):
    from utmos_amd import samples
    names = ["a", "b", "c", "d", "e"]
    new = np.asarray([[4, 0], [1, 1], [0, 2], [0, 0], [1, 0]], np.int64)   # rows: samples, columns: panel rows
    total = np.asarray([4, 4, 2, 0, 4], np.int64)                          # d carries nothing: never outside
    lines = samples.represent_rows(names, [0, 2], new, total)
    assert lines == [("a", 3, 0.1667, 0.25, 0.0, "c"), ("c", 2, 0.375, 0.375, 0.25, "e")]
    # pct after row 0: b 1/4, c 0/2, e 1/4 -> mean 0.1667, median 0.25, min 0 at c; after row 1: b 2/4, e 1/4
    path = tmp_path / "r.tsv"
    samples.write_represent(str(path), lines)
    assert open(path).read() == (samples.REPRESENT_HEADER + "a\t3\t0.1667\t0.25\t0.0\tc\nc\t2\t0.375\t0.375\t0.25\te\n")
    everyone = samples.represent_rows(["a", "b"], [1, 0], np.asarray([[1, 1], [2, 0]], np.int64), np.asarray([2, 2], np.int64))
    assert everyone[0] == ("b", 1, 0.5, 0.5, 0.5, "a")
    assert everyone[1][:2] == ("a", 0) and all(np.isnan(v) for v in everyone[1][2:5]) and everyone[1][5] == "."
    samples.write_represent(str(path), everyone)
    assert open(path).read().splitlines()[2] == "a\t0\tnan\tnan\tnan\t."
    tie = samples.represent_rows(["a", "b", "c"], [0], np.asarray([[2], [1], [1]], np.int64), np.asarray([2, 2, 2], np.int64))
    assert tie[0][5] == "b"                                              # ties go to the lowest index


def test_too_long_a_panel_is_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    for flag in ("--samples-out", "--represent-out"):
        with pytest.raises(SystemExit) as err:
            select.select_main(["-c", str(CLASSES_MAX), flag, "x.out", __file__])
        assert err.value.code == 1 and str(CLASSES_MAX - 1) in capsys.readouterr().err


def test_several_processes_are_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    for flag in ("--samples-out", "--represent-out"):
        with pytest.raises(SystemExit) as err:
            select.select_main([flag, "x.out", __file__])
        assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_the_usage_names_the_new_outputs():
    from utmos_amd import __main__ as cli
    text = cli._usage()
    assert "--samples-out" in text and "--by-sample" in text
