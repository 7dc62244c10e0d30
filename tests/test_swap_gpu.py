"""GPU: swap gains through the C ABI (utm_swap_gains: k_swap_masks + k_swap_pairs), DeviceMatrix.swap_gains and
`select --refine`.

The gains are held against the numpy restatement by definition (tests/swap_ref.py) and the CPU build of the kernels'
arithmetic bit for bit.  The shapes sit on the kernels' edges: one 4 KiB variant tile +- 1 bit (32,768 variants), sample
counts that are no multiple of a candidate block of 16, panels of 1, 2 and 3 row blocks of 64 (k = 64: the row of
uncovered variants is alone in a block of its own)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import swap_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements
PANELS = (0, 1, 64, 65, 130)


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


@functools.lru_cache(maxsize=None)
def seeded(n_var, n_samp):
    rng = np.random.default_rng(n_var * 5 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    dense.setflags(write=False)
    return dense


def host_swap(cols, panel, n_var):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    panel32 = np.ascontiguousarray(panel, dtype=np.uint32)
    k, n = len(panel32), cols.shape[0]
    gains, unique, new = np.zeros((k, n), np.int64), np.zeros(k, np.int64), np.zeros(n, np.int64)
    base = ctypes.c_int64(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_swap_gains_host(p(cols), cols.shape[1], n_var, n, p(panel32), k, p(gains), p(unique), p(new), ctypes.byref(base)))
    return gains, unique, new, base.value


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def same(got, want):
    return all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_samp", [70, 200, 300])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 32767, 32768, 32769])
def test_gains_equal_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    cols = npo.pack_columns(seeded(n_var, n_samp))
    rng = np.random.default_rng(n_var + n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for k in PANELS:
            if k > n_samp:
                continue
            panel = rng.permutation(n_samp)[:k]
            got = mat.swap_gains(panel)
            assert got[0].dtype == np.int64 and got[0].shape == (k, n_samp)
            if k == 0:
                assert got[3] == 0
                continue
            want, base = swap_ref.swap_gains(cols, panel, n_var)
            assert got[3] == base and (got[0] == want).all(), k
            assert (got[1] == swap_ref.unique_counts(cols, panel, n_var)).all(), k
            assert (got[2] == swap_ref.new_counts(cols, panel, n_var)).all(), k
            assert same(got, host_swap(cols, panel, n_var)), k


def test_a_dense_matrix_where_most_variants_have_support_above_one(dev):
    rng = np.random.default_rng(8)
    n_var, n_samp = 33000, 90
    cols = npo.pack_columns(ou.random_dense(rng, n_var, n_samp, density=0.2, sfs=False))
    panel = rng.permutation(n_samp)[:9]
    with uploaded(dev, [cols], [n_var]) as mat:
        got = mat.swap_gains(panel)
    want, base = swap_ref.swap_gains(cols, panel, n_var)
    assert got[3] == base and (got[0] == want).all() and same(got, host_swap(cols, panel, n_var))
    assert (got[1] > 0).all() and got[0].max() > 0


def test_two_chunks_of_unequal_size_add_up(dev):
    chunk_vars, n_samp = [32769, 100], 200
    dense = seeded(sum(chunk_vars), n_samp)
    cols = [npo.pack_columns(dense[:32769]), npo.pack_columns(dense[32769:])]
    whole = npo.pack_columns(dense)
    rng = np.random.default_rng(2)
    with uploaded(dev, cols, chunk_vars) as mat:
        for k in (1, 65, 130):
            panel = rng.permutation(n_samp)[:k]
            got = mat.swap_gains(panel)
            want, base = swap_ref.swap_gains(whole, panel, sum(chunk_vars))
            assert got[3] == base and (got[0] == want).all(), k
            parts = [host_swap(c, panel, n) for c, n in zip(cols, chunk_vars)]
            assert same(got, [parts[0][j] + parts[1][j] for j in range(4)]), k


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_rows_cleared_by_an_af_of_zero_have_no_carriers(dev, kind):
    rng = np.random.default_rng(5)
    n_var, n_samp = 33000, 60
    dense = ou.random_dense(rng, n_var, n_samp)
    af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0
    zero = rng.random(n_var) < 0.05
    zero[[0, 63, 64, n_var - 1]] = True
    af[zero] = 0.0
    cleared = npo.pack_columns(dense & ~zero[:, None])
    panel = rng.permutation(n_samp)[:20]
    with dev.DeviceMatrix(n_samp) as mat:
        c = mat.add_chunk(n_var)
        mat.upload_columns(c, npo.pack_columns(dense))
        mat.set_af(c, af.astype(np.float32 if kind == "f32" else np.float64))
        got = mat.swap_gains(panel)
    want, base = swap_ref.swap_gains(cleared, panel, n_var)
    assert got[3] == base and (got[0] == want).all() and same(got, host_swap(cleared, panel, n_var))


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
        before = a.swap_gains([2, 9, 30])                                # valid before any reset
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        panel = [int(s) for s in first[0]] + [2, 9]                      # winners, a used and an excluded sample
        got = a.swap_gains(panel)
        want, base = swap_ref.swap_gains(whole, panel, n_var)
        assert got[3] == base and (got[0] == want).all()
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        assert same(a.swap_gains([2, 9, 30]), before)                    # and the selection changes nothing of the gains


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_the_outputs(dev):
    n_var, n_samp = 9000, 30
    cols = npo.pack_columns(seeded(n_var, n_samp))
    lib = dev.nat.lib()
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        gains, unique, new = np.full((3, n_samp), 1234, np.int64), np.full(3, 1234, np.int64), np.full(n_samp, 1234, np.int64)
        base = ctypes.c_int64(1234)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

        def call(idx, dest=gains, k=None):
            arr = None if idx is None else np.asarray(idx, dtype=np.int64)
            return lib.utm_swap_gains(mat._h, p(arr), len(arr) if k is None else k, p(dest), p(unique), p(new), ctypes.byref(base), None)

        assert call(None, k=2) == EINVAL                                 # NULL panel with k > 0
        assert call([1, 2], dest=None) == EINVAL                         # NULL gain_out with k > 0
        assert call([1, 30]) == EINVAL and call([-1]) == EINVAL          # index out of range
        assert call([4, 5, 4]) == EINVAL                                 # duplicate
        assert call([1, 2], k=-1) == EINVAL
        assert (gains == 1234).all() and (unique == 1234).all() and (new == 1234).all() and base.value == 1234
        assert call(None, dest=None, k=0) == 0 and base.value == 0 and (new == 1234).all()
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        ms = ctypes.c_double(-1.0)
        arr = np.asarray([7, 8, 1], dtype=np.int64)
        assert lib.utm_swap_gains(mat._h, p(arr), 3, p(gains), None, None, None, ctypes.byref(ms)) == 0 and ms.value > 0
        assert (gains == swap_ref.swap_gains(cols, arr, n_var)[0]).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.swap_gains([3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


# ----------------------------------------------------------------- 4. the command line
def run_cli(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def tsv_rows(path):
    lines = open(path).read().splitlines()
    return lines[0], [line.split("\t") for line in lines[1:]]


def test_refine_on_mid_ends_in_a_local_optimum_and_prints_the_panel_s_greedy_order(dev, tmp_path):
    mid = os.path.join(ou.GOLD, "mid.npz")
    plain, refined, swaps = (str(tmp_path / name) for name in ("plain.tsv", "refined.tsv", "swaps.tsv"))
    run_cli(["-c", "10", "-o", plain, mid])
    run_cli(["-c", "10", "--refine", "-1", "--refine-out", swaps, "-o", refined, mid])
    part = ou.load_part("mid")
    assert open(plain).read() == npo.select_tsv([part], count=10)        # (without the flag: the reference's rows)
    greedy_total = int(tsv_rows(plain)[1][-1][3])
    header, log = tsv_rows(swaps)
    assert header == "swap\tout\tin\tgain\ttot_captured"
    assert [int(e[0]) for e in log] == list(range(1, len(log) + 1)) and all(int(e[3]) > 0 for e in log)
    _, rows = tsv_rows(refined)
    panel_names = [r[0] for r in rows]
    final_total = int(rows[-1][3])
    assert final_total == greedy_total + sum(int(e[3]) for e in log)
    if log:
        assert int(log[-1][4]) == final_total
    # the panel is the greedy one with the logged exchanges made
    members = [r[0] for r in tsv_rows(plain)[1]]
    for _, out, into, _, _ in log:
        members[members.index(out)] = into
    assert sorted(members) == sorted(panel_names)
    # the TSV is what the oracle selects from the panel alone
    assert open(refined).read() == npo.select_tsv([part], count=len(members), subset=members)
    # and no single exchange improves it
    matrix, _, samples = npo.build_matrix([part])
    position = {str(s): i for i, s in enumerate(samples)}
    panel = [position[name] for name in members]
    gains, base = swap_ref.swap_gains(npo.pack_columns(matrix), panel, matrix.shape[0])
    assert base == final_total and gains.max() <= 0


def test_the_hand_case_through_the_command_line(dev, tmp_path):
    dense = np.zeros((6, 3), bool)                                       # A = {1,2,3,4}, B = {1,2,5}, C = {3,4,6}
    dense[[0, 1, 2, 3], 0] = True
    dense[[0, 1, 4], 1] = True
    dense[[2, 3, 5], 2] = True
    path, plain, refined, swaps = (str(tmp_path / name) for name in ("abc.npz", "plain.tsv", "refined.tsv", "swaps.tsv"))
    np.savez(path, GT=np.packbits(dense, axis=1), AF=np.full(6, 0.25), samples=np.array(["A", "B", "C"]))
    run_cli(["-c", "2", "-o", plain, path])
    run_cli(["-c", "2", "--refine", "1", "--refine-out", swaps, "-o", refined, path])
    assert [(r[0], r[3]) for r in tsv_rows(plain)[1]] == [("A", "4"), ("B", "5")]
    assert [(r[0], r[2], r[3]) for r in tsv_rows(refined)[1]] == [("B", "3", "3"), ("C", "3", "6")]
    assert tsv_rows(swaps)[1] == [["1", "A", "C", "1", "6"]]


def test_include_samples_are_pinned(dev, tmp_path):
    dense = np.zeros((6, 3), bool)
    dense[[0, 1, 2, 3], 0] = True
    dense[[0, 1, 4], 1] = True
    dense[[2, 3, 5], 2] = True
    path, refined, swaps = (str(tmp_path / name) for name in ("abc.npz", "refined.tsv", "swaps.tsv"))
    np.savez(path, GT=np.packbits(dense, axis=1), AF=np.full(6, 0.25), samples=np.array(["A", "B", "C"]))
    run_cli(["-c", "2", "--include", "A", "--refine", "-1", "--refine-out", swaps, "-o", refined, path])
    assert [(r[0], r[3]) for r in tsv_rows(refined)[1]] == [("A", "4"), ("B", "5")] and tsv_rows(swaps)[1] == []
