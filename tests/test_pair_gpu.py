"""GPU: pair counts through the C ABI (utm_pair_counts: k_swap_masks + k_pair_counts), DeviceMatrix.pair_counts and the
`overlap` command.

The counts are held against the numpy restatement by definition (tests/pair_ref.py) and the CPU build of the kernels'
arithmetic bit for bit.  The shapes sit on the kernel's edges: one 4 KiB variant tile +- 1 bit (32,768 variants), lists
of one to four blocks of 64 samples (so diagonal and off-diagonal block pairs and partly filled blocks), several tiles per
workgroup with a last tile that is one wave wide."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import pair_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements
LISTS = (0, 1, 2, 63, 64, 65, 130, 200)


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


def host_pairs(cols, indices, n_var, given=()):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx, panel = np.ascontiguousarray(indices, dtype=np.uint32), np.ascontiguousarray(given, dtype=np.uint32)
    out = np.zeros((len(idx), len(idx)), np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None
    nat.check(nat.lib().utm_pair_counts_host(cols.ctypes.data_as(ctypes.c_void_p), cols.shape[1], n_var, cols.shape[0], p(idx), len(idx),
                                             p(panel), len(panel), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_samp", [70, 200])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 32767, 32768, 32769])
def test_counts_equal_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    cols = npo.pack_columns(seeded(n_var, n_samp))
    rng = np.random.default_rng(n_var + n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for n in LISTS:
            if n > n_samp:
                continue
            order = rng.permutation(n_samp)
            indices = order[:n]
            for given in ((), order[n_samp - 3:], np.concatenate([order[n_samp - 2:], order[:1]])):   # none, apart, one in both
                got = mat.pair_counts(indices, given)
                assert got.dtype == np.int64 and got.shape == (n, n)
                assert (got == pair_ref.pair_counts(cols, indices, n_var, given)).all(), (n, len(given))
                assert (got == host_pairs(cols, indices, n_var, given)).all(), (n, len(given))


def test_a_dense_matrix(dev):
    rng = np.random.default_rng(8)
    n_var, n_samp = 33000, 90
    cols = npo.pack_columns(ou.random_dense(rng, n_var, n_samp, density=0.4, sfs=False))
    indices, given = rng.permutation(n_samp)[:70], [3]
    with uploaded(dev, [cols], [n_var]) as mat:
        for g in ((), given):
            got = mat.pair_counts(indices, g)
            assert (got == pair_ref.pair_counts(cols, indices, n_var, g)).all() and (got == host_pairs(cols, indices, n_var, g)).all()
            assert got.min() > 0 or len(g)


def test_two_chunks_of_unequal_size_add_up(dev):
    chunk_vars, n_samp = [32769, 100], 200
    dense = seeded(sum(chunk_vars), n_samp)
    cols = [npo.pack_columns(dense[:32769]), npo.pack_columns(dense[32769:])]
    whole = npo.pack_columns(dense)
    rng = np.random.default_rng(2)
    with uploaded(dev, cols, chunk_vars) as mat:
        for n in (1, 65, 130):
            order = rng.permutation(n_samp)
            for given in ((), order[-4:]):
                got = mat.pair_counts(order[:n], given)
                assert (got == pair_ref.pair_counts(whole, order[:n], sum(chunk_vars), given)).all(), n
                assert (got == sum(host_pairs(c, order[:n], v, given) for c, v in zip(cols, chunk_vars))).all(), n


@pytest.mark.parametrize("tile_groups", [1, 2])
def test_workgroups_that_walk_several_tiles_give_the_same_counts(dev, tile_groups):
    n_var, n_samp, n = 3 * 32768 + 5, 140, 130                          # four tiles, the last one a single wave wide
    cols = npo.pack_columns(seeded(n_var, n_samp))
    order = np.random.default_rng(tile_groups).permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for given in ((), order[-5:]):
            got = mat.pair_counts(order[:n], given, tile_groups=tile_groups)
            assert (got == mat.pair_counts(order[:n], given)).all()
            assert (got == pair_ref.pair_counts(cols, order[:n], n_var, given)).all()
        assert (mat.pair_counts(order[:n], order[-5:], tile_groups=1000) == got).all()   # clamped to the tile count


def test_rows_cleared_by_an_af_of_zero_have_no_carriers(dev):
    rng = np.random.default_rng(5)
    n_var, n_samp = 33000, 70
    dense = ou.random_dense(rng, n_var, n_samp)
    af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0
    zero = rng.random(n_var) < 0.05
    zero[[0, 63, 64, n_var - 1]] = True
    af[zero] = 0.0
    cleared = npo.pack_columns(dense & ~zero[:, None])
    order = rng.permutation(n_samp)
    with dev.DeviceMatrix(n_samp) as mat:
        c = mat.add_chunk(n_var)
        mat.upload_columns(c, npo.pack_columns(dense))
        mat.set_af(c, af.astype(np.float64))
        for given in ((), order[-2:]):
            got = mat.pair_counts(order[:66], given)
            assert (got == pair_ref.pair_counts(cleared, order[:66], n_var, given)).all()
            assert (got == host_pairs(cleared, order[:66], n_var, given)).all()


# ----------------------------------------------------------------- 2. stateless
def test_a_call_in_between_changes_nothing_of_the_selection(dev):
    rng = np.random.default_rng(21)
    n_var, n_samp = 40_000, 120
    dense = ou.random_dense(rng, n_var, n_samp)
    chunk_vars = [25_000, 15_000]
    cols = [npo.pack_columns(dense[:25_000]), npo.pack_columns(dense[25_000:])]
    whole = npo.pack_columns(dense)
    state = np.ones(n_samp, np.uint8)
    state[[2, 50]] = 0
    state[[9, 10]] = 2
    a, b = uploaded(dev, cols, chunk_vars), uploaded(dev, cols, chunk_vars)
    with a, b:
        before = a.pair_counts([2, 9, 30], [50, 10])                     # valid before any reset
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        indices = list(dict.fromkeys([int(s) for s in first[0]] + [2, 9] + list(range(60, 120))))   # winners, a used and an excluded sample
        given = [50, 10, int(first[0][3])]                               # a used, an excluded and one that is listed too
        got = a.pair_counts(indices, given)
        assert (got == pair_ref.pair_counts(whole, indices, n_var, given)).all() and (got[3] == 0).all()
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        assert (a.pair_counts([2, 9, 30], [50, 10]) == before).all()     # and the selection changes nothing of the counts


def test_against_the_engine_on_mid(dev):
    """What a used sample s takes from every other sample's score is what the two share."""
    matrix, _, samples = npo.build_matrix([ou.load_part("mid")])
    n_samp = len(samples)
    with dev.DeviceMatrix(n_samp) as mat:
        mat.upload_columns(mat.add_chunk(matrix.shape[0]), npo.pack_columns(matrix))
        shared = mat.pair_counts(np.arange(n_samp))
        var_count = mat.var_count()
        assert (np.diagonal(shared) == var_count).all()
        for s in (0, n_samp // 2, n_samp - 1):
            state = np.ones(n_samp, np.uint8)
            state[s] = 0
            mat.set_state(state)
            mat.reset()
            counts = mat.peek_scores()[0]
            selectable = state == 1
            assert ((var_count - counts)[selectable] == shared[s][selectable]).all(), s


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_out(dev):
    n_var, n_samp = 9000, 30
    cols = npo.pack_columns(seeded(n_var, n_samp))
    lib = dev.nat.lib()
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        out = np.full((3, 3), 1234, np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        i64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)

        def call(idx, given=None, dest=out, n=None, n_given=None):
            idx, given = i64(idx), i64(given)
            return lib.utm_pair_counts(mat._h, p(idx), len(idx) if n is None else n, p(given),
                                       (0 if given is None else len(given)) if n_given is None else n_given, 0, p(dest), None)

        assert call(None, n=2) == EINVAL                                 # NULL list with a nonzero length
        assert call([1, 2], None, n_given=1) == EINVAL                   # ... the given list
        assert call([1, 2], dest=None) == EINVAL                         # NULL out with n > 0
        assert call([1, 30]) == EINVAL and call([-1]) == EINVAL          # index out of range
        assert call([1, 2], [30]) == EINVAL and call([1, 2], [-1]) == EINVAL
        assert call([4, 5, 4]) == EINVAL and call([4, 5], [7, 7]) == EINVAL      # a duplicate within either list
        assert call([1, 2], n=-1) == EINVAL
        assert (out == 1234).all()
        assert call(None, dest=None, n=0) == 0 and call(None, [3], dest=None, n=0) == 0 and (out == 1234).all()
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        ms = ctypes.c_double(-1.0)
        arr, given = np.asarray([7, 8, 1], dtype=np.int64), np.asarray([8, 2], dtype=np.int64)
        assert lib.utm_pair_counts(mat._h, p(arr), 3, p(given), 2, 0, p(out), ctypes.byref(ms)) == 0 and ms.value > 0
        assert (out == pair_ref.pair_counts(cols, arr, n_var, given)).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.pair_counts([3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


# ----------------------------------------------------------------- 4. the command line
PARTS = ("chunk0", "chunk1")


def test_the_command_on_two_parts_in_many_chunks(dev, tmp_path):
    from utmos_amd import overlap
    files = [os.path.join(ou.GOLD, name + ".npz") for name in PARTS]
    parts = [ou.load_part(name) for name in PARTS]
    matrix, _, samples = npo.build_matrix(parts)                         # from the ORIGINAL part files
    names = [str(s) for s in samples]
    given, excluded = [names[5], names[1]], [names[0], names[7]]
    npz, tsv = str(tmp_path / "shared.npz"), str(tmp_path / "pairs.tsv")
    overlap.overlap_main(["--maxmem", "0", "--buffer", "64", "--given", ",".join(given), "--exclude", ",".join(excluded),
                          "-o", npz, "--pairs-out", tsv, "--sort", "joint", "--top", "15"] + files)
    listed = [i for i, name in enumerate(names) if name not in excluded]
    want = pair_ref.pair_counts_dense(matrix, listed, [names.index(g) for g in given])
    z = np.load(npz)
    assert z["shared"].dtype == np.int64 and (z["shared"] == want).all() and want.any()
    assert z["samples"].tolist() == [names[i] for i in listed] and z["given"].tolist() == given
    assert (z["count"] == np.diagonal(want)).all() and [os.path.basename(f) for f in z["files"]] == [name + ".npz" for name in PARTS]
    rows = overlap.pair_rows(want, [names[i] for i in listed], "joint", 15)
    assert len(rows) == 15
    assert open(tsv).read() == overlap.PAIRS_HEADER + "".join("\t".join(str(f) for f in row) + "\n" for row in rows)


def test_the_command_writes_the_pairs_to_stdout_and_names_an_unknown_given(dev, tmp_path, capfd):
    from utmos_amd import __main__ as cli
    part = os.path.join(ou.GOLD, "tiny.npz")
    matrix, _, samples = npo.build_matrix([ou.load_part("tiny")])
    from utmos_amd import overlap
    assert cli.main(["overlap", "--top", "-1", part]) == 0
    want = overlap.pair_rows(pair_ref.pair_counts_dense(matrix, range(len(samples))), [str(s) for s in samples], "jaccard", -1)
    assert capfd.readouterr().out == overlap.PAIRS_HEADER + "".join("\t".join(str(f) for f in row) + "\n" for row in want)
    with pytest.raises(SystemExit) as err:
        cli.main(["overlap", "--given", "nobody", part])
    assert err.value.code == 1 and "nobody" in capfd.readouterr().err
