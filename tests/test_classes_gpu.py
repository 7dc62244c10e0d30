"""GPU: class counts through the C ABI (utm_class_counts: k_class_counts) and DeviceMatrix.class_counts.

The table is held against the numpy restatement by definition (tests/class_ref.py) and the CPU build of the kernel's word
walk, cell for cell -- all counts are integers, every comparison is exact.  The shapes sit on the edges of the launch
shape: one wave's KiB and one 4 KiB tile +- 1 bit, a last tile a single wave wide, four tiles; lists on both sides of a
column block of 16; class counts that force fewer columns per workgroup (2,505 -> 6, 16,384 -> 1); tile groups of 1, 3,
automatic and more than there are tiles; every mode."""
import ctypes
import functools

import numpy as np
import pytest

import class_ref
import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements
N_SAMP = 72
LISTS = (1, 15, 16, 17, 70)                   # UTM_CLASS_U = 16 columns per workgroup
TILE_GROUPS = (0, 1, 3, 1000)
MODES = (0, 1, 2)
CANARY = -77


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


@functools.lru_cache(maxsize=None)
def seeded(n_var, n_samp=N_SAMP):
    rng = np.random.default_rng(n_var * 5 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp, density=0.3, sfs=False)
    dense[[0, n_var - 1]] = True                                         # the first and the last bit of every column
    dense.setflags(write=False)
    return dense


def random_labels(rng, n_var, n_classes):
    labels = rng.integers(0, n_classes, size=n_var).astype(np.int32)
    labels[rng.random(n_var) < 0.1] = -1
    return labels


def host_table(cols, n_var, labels, n_classes, indices=None):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    table = np.zeros((cols.shape[0] if idx is None else len(idx), n_classes), np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_class_counts_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(np.ascontiguousarray(labels, np.int32)), n_classes,
                                              p(idx), 0 if idx is None else len(idx), p(table)))
    return table


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def check_shapes(mat, whole, labels, n_classes, indices, shapes, tag=None):
    """The listed rows of `whole` (the restatement over every column) from every (tile_groups, mode) of `shapes`."""
    want = whole if indices is None else whole[np.asarray(indices)]
    for tile_groups, mode in shapes:
        got = mat.class_counts([labels], n_classes, indices, tile_groups=tile_groups, mode=mode)
        assert got.dtype == np.int64 and got.shape == want.shape
        assert (got == want).all(), (tag, tile_groups, mode)


ALL_SHAPES = [(g, 0) for g in TILE_GROUPS] + [(0, m) for m in MODES[1:]] + [(3, 2)]


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_var", [1, 8191, 8192, 8193, 32767, 32768, 32769, 40_000, 98_305])
def test_table_equals_the_restatement_and_the_cpu_build(dev, n_var):
    cols = npo.pack_columns(seeded(n_var))
    rng = np.random.default_rng(n_var)
    labels = random_labels(rng, n_var, 9)
    whole = class_ref.class_counts(cols, labels, 9, None, n_var)
    assert (host_table(cols, n_var, labels, 9) == whole).all()
    with uploaded(dev, [cols], [n_var]) as mat:
        check_shapes(mat, whole, labels, 9, None, ALL_SHAPES, "every sample")
        for n in LISTS:
            indices = rng.permutation(N_SAMP)[:n]                        # (not in index order)
            assert (host_table(cols, n_var, labels, 9, indices) == whole[indices]).all()
            check_shapes(mat, whole, labels, 9, indices, ALL_SHAPES, n)


@pytest.mark.parametrize("n_classes,columns", [(2505, 6), (16384, 1), (1024, 16), (1025, 15)])
def test_class_counts_that_leave_fewer_columns_to_a_workgroup(dev, n_classes, columns):
    assert min(16, 16384 // n_classes) == columns
    n_var = 40_000                                                       # two tiles, the last a single wave wide
    cols = npo.pack_columns(seeded(n_var))
    rng = np.random.default_rng(n_classes)
    labels = random_labels(rng, n_var, n_classes)
    labels[[0, n_var - 1]] = [n_classes - 1, 0]                          # the last and the first bin of every column
    whole = class_ref.class_counts(cols, labels, n_classes, None, n_var)
    assert (host_table(cols, n_var, labels, n_classes) == whole).all()
    with uploaded(dev, [cols], [n_var]) as mat:
        indices = rng.permutation(N_SAMP)[:70]
        check_shapes(mat, whole, labels, n_classes, indices, [(0, 0), (1, 1), (3, 2)], n_classes)
        check_shapes(mat, whole, labels, n_classes, None, [(0, 0)], n_classes)


@pytest.mark.parametrize("pattern", ["one_hot_class", "none", "head_empty"])
def test_label_patterns(dev, pattern):
    n_var, n_classes = 32769 + 8192, 40
    cols = npo.pack_columns(seeded(n_var))
    rng = np.random.default_rng(len(pattern))
    labels = {"one_hot_class": np.full(n_var, 0, np.int32), "none": np.full(n_var, -1, np.int32),
              "head_empty": rng.integers(8, n_classes, size=n_var).astype(np.int32)}[pattern]
    whole = class_ref.class_counts(cols, labels, n_classes, None, n_var)
    if pattern == "one_hot_class":                                       # every lane adds to one bin
        assert whole[:, 0].tolist() == np.bitwise_count(cols).sum(axis=1).tolist() and not whole[:, 1:].any()
    if pattern == "none":
        assert not whole.any()
    if pattern == "head_empty":
        assert not whole[:, :8].any() and whole[:, 8:].all()
    with uploaded(dev, [cols], [n_var]) as mat:
        check_shapes(mat, whole, labels, n_classes, None, ALL_SHAPES, pattern)
        check_shapes(mat, whole, labels, n_classes, [5, 71, 0], ALL_SHAPES, pattern)


def test_one_class_is_every_sample_s_variant_count(dev):
    n_var = 9000
    cols = npo.pack_columns(seeded(n_var))
    with uploaded(dev, [cols], [n_var]) as mat:
        got = mat.class_counts([np.zeros(n_var, np.int32)], 1)
        assert got.shape == (N_SAMP, 1) and got[:, 0].tolist() == mat.var_count().tolist()


def test_two_chunks_of_unequal_size_add_up(dev):
    chunk_vars, n_classes = [32769, 100], 20
    dense = seeded(sum(chunk_vars))
    cols = [npo.pack_columns(dense[:32769]), npo.pack_columns(dense[32769:])]
    rng = np.random.default_rng(2)
    labels = random_labels(rng, sum(chunk_vars), n_classes)
    per_chunk = [labels[:32769], labels[32769:]]
    whole = class_ref.class_counts_dense(dense, labels, n_classes)
    with uploaded(dev, cols, chunk_vars) as mat:
        for indices in (None, rng.permutation(N_SAMP)[:17]):
            want = whole if indices is None else whole[indices]
            for mode in MODES:
                got, ms = mat.class_counts(per_chunk, n_classes, indices, mode=mode, pass_ms=True)
                assert (got == want).all() and ms > 0
            parts = [host_table(c, v, l, n_classes, indices) for c, v, l in zip(cols, chunk_vars, per_chunk)]
            assert (sum(parts) == want).all()
        with pytest.raises(ValueError):
            mat.class_counts(per_chunk[:1], n_classes)
        with pytest.raises(ValueError):
            mat.class_counts([labels[:5], per_chunk[1]], n_classes)


def test_rows_cleared_by_an_af_of_zero_have_no_carriers(dev):
    rng = np.random.default_rng(5)
    n_var, n_classes = 33000, 12
    dense = np.array(seeded(n_var))
    af = rng.integers(1, 2 * N_SAMP, size=n_var) / (2.0 * N_SAMP) / 3.0
    zero = rng.random(n_var) < 0.05
    zero[[0, 63, 64, n_var - 1]] = True
    af[zero] = 0.0
    labels = random_labels(rng, n_var, n_classes)
    want = class_ref.class_counts_dense(dense & ~zero[:, None], labels, n_classes)
    assert (want != class_ref.class_counts_dense(dense, labels, n_classes)).any()
    with dev.DeviceMatrix(N_SAMP) as mat:
        c = mat.add_chunk(n_var)
        mat.upload_columns(c, npo.pack_columns(dense))
        mat.set_af(c, af.astype(np.float64))
        for mode in MODES:
            assert (mat.class_counts([labels], n_classes, mode=mode) == want).all()


# ----------------------------------------------------------------- 2. stateless
def test_a_call_in_between_changes_nothing_of_the_selection(dev):
    rng = np.random.default_rng(21)
    n_var, n_samp, n_classes = 40_000, 120, 30
    dense = ou.random_dense(rng, n_var, n_samp)
    chunk_vars = [25_000, 15_000]
    cols = [npo.pack_columns(dense[:25_000]), npo.pack_columns(dense[25_000:])]
    labels = random_labels(rng, n_var, n_classes)
    per_chunk = [labels[:25_000], labels[25_000:]]
    whole = class_ref.class_counts_dense(dense, labels, n_classes)
    state = np.ones(n_samp, np.uint8)
    state[[2, 50]] = 0
    state[[9, 10]] = 2
    a, b = uploaded(dev, cols, chunk_vars), uploaded(dev, cols, chunk_vars)
    with a, b:
        assert (a.class_counts(per_chunk, n_classes, [2, 9, 30]) == whole[[2, 9, 30]]).all()   # valid before any reset
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        indices = list(dict.fromkeys([int(s) for s in first[0]] + [2, 50, 9, 10] + list(range(60, 120))))   # winners, excluded and used samples
        for mode in MODES:
            assert (a.class_counts(per_chunk, n_classes, indices, mode=mode) == whole[indices]).all()
        assert (a.class_counts(per_chunk, n_classes) == whole).all()
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        assert (a.class_counts(per_chunk, n_classes, [2, 9, 30]) == whole[[2, 9, 30]]).all()   # and the selection changes nothing of the table


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_the_table(dev):
    n_var, n_samp, n_classes = 9000, 30, 4
    cols = npo.pack_columns(seeded(n_var, n_samp))
    lib = dev.nat.lib()
    rng = np.random.default_rng(1)
    good = random_labels(rng, n_var, n_classes)
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        table = np.full((n_samp, n_classes), CANARY, np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        i64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)

        def call(labels=good, classes=n_classes, idx=None, n=None, out=table, chunk=0, tile_groups=0, mode=0):
            idx = i64(idx)
            labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
            return lib.utm_class_counts(mat._h, chunk, p(labels), classes, p(idx), (0 if idx is None else len(idx)) if n is None else n,
                                        tile_groups, mode, p(out), None)

        assert call(labels=None) == EINVAL and call(out=None) == EINVAL  # a NULL class_of or table_out
        assert call(idx=None, n=2) == EINVAL and call(idx=[1, 2], n=-1) == EINVAL
        assert call(classes=0) == EINVAL and call(classes=16385) == EINVAL
        bad = good.copy()
        bad[n_var - 1] = n_classes
        assert call(labels=bad) == EINVAL and b"class 4" in lib.utm_last_error()
        bad[n_var - 1] = -2
        assert call(labels=bad) == EINVAL
        assert call(chunk=1) == EINVAL and call(chunk=-1) == EINVAL
        assert call(idx=[1, 30]) == EINVAL and call(idx=[-1]) == EINVAL  # index out of range
        assert call(idx=[4, 5, 4]) == EINVAL and b"twice" in lib.utm_last_error()
        assert call(mode=3) == EINVAL
        assert (table == CANARY).all()
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        whole = class_ref.class_counts(cols, good, n_classes, None, n_var)
        assert call() == 0 and (table == whole).all()                    # written, not added to
        assert call() == 0 and (table == whole).all()
        ms = ctypes.c_double(-1.0)
        part = np.full((3, n_classes), CANARY, np.int64)
        arr = np.asarray([7, 8, 1], dtype=np.int64)
        assert lib.utm_class_counts(mat._h, 0, p(good), n_classes, p(arr), 3, 0, 0, p(part), ctypes.byref(ms)) == 0 and ms.value > 0
        assert (part == whole[[7, 8, 1]]).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.class_counts([np.zeros(n_var, np.int32)], 1, [3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers
