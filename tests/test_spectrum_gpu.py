"""GPU: carrier counts through the C ABI (utm_carrier_counts: k_swap_masks + k_carrier_counts), DeviceMatrix.carrier_counts
and the `spectrum` command.

The histogram and the per-variant counts are held against the numpy restatement by definition (tests/spectrum_ref.py) and
the CPU build of the kernel's word arithmetic, value for value.  The shapes sit on the kernel's edges: one wave's KiB and
one 4 KiB tile +- 1 bit, lists of one carry-save block (16 columns) +- 1 and on both sides of every plane-count
instantiation, several tiles with a last one a single wave wide, and both places the decoded bins can meet (LDS, global)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import spectrum_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements
B = 16                                        # UTM_SPEC_B: columns per carry-save block
LISTS = (0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 255, 256, 257)
LDS_BINS = 4096                               # UTM_SPEC_LDS_BINS


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


def host_counts(cols, indices, n_var, given=()):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx, panel = np.ascontiguousarray(indices, dtype=np.uint32), np.ascontiguousarray(given, dtype=np.uint32)
    hist, count = np.zeros(len(idx) + 1, np.int64), np.zeros(n_var, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None
    nat.check(nat.lib().utm_carrier_counts_host(cols.ctypes.data_as(ctypes.c_void_p), cols.shape[1], n_var, cols.shape[0], p(idx), len(idx),
                                                p(panel), len(panel), p(hist), p(count)))
    return hist, count


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def check_all_modes(mat, cols, indices, n_var, given=(), tag=None):
    """Every hist_mode the list admits, with and without the counts, against the restatement and the CPU build."""
    want_hist, want_count = spectrum_ref.carrier_counts(cols, indices, n_var, given)
    host_hist, host_count = host_counts(cols, indices, n_var, given)
    assert (host_hist == want_hist).all() and (host_count == want_count).all(), tag
    for mode, counts in ((0, True), (0, False), (1, False), (1, True), (2, True), (2, False)):
        if mode == 1 and len(indices) + 1 > LDS_BINS:
            continue
        got = mat.carrier_counts(indices, given, counts=counts, hist_mode=mode)
        hist = got[0] if counts else got
        assert hist.dtype == np.int64 and hist.shape == (len(indices) + 1,)
        assert (hist == want_hist).all(), (tag, mode, counts)
        if counts:
            assert len(got[1]) == 1 and got[1][0].dtype == np.int32 and (got[1][0] == want_count).all(), (tag, mode)
    return want_hist, want_count


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_samp", [70, 300])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 8192, 8193, 32767, 32768, 32769])
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
                hist, count = check_all_modes(mat, cols, indices, n_var, given, (n, len(given)))
                assert hist.sum() == n_var - (count < 0).sum()


def test_a_dense_matrix_with_rows_everybody_carries(dev):
    rng = np.random.default_rng(8)
    n_var, n_samp = 33000, 300
    dense = ou.random_dense(rng, n_var, n_samp, density=0.9, sfs=False)
    dense[5000:5200] = True                                              # bin n, and the longest carry chains
    dense[[0, 63, 64, n_var - 1]] = True
    cols = npo.pack_columns(dense)
    order = rng.permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for n in (255, 256, 300):
            hist, _ = check_all_modes(mat, cols, order[:n], n_var, (), n)
            assert hist[n] >= 204 and hist[:8].sum() == 0                # nothing in the popcounted bins
        hist, count = check_all_modes(mat, cols, order[:290], n_var, order[295:296], "given")
        assert (count < 0).sum() > n_var // 2


def test_the_sparse_matrix_beyond_a_panel_of_twenty(dev):
    n_var, n_samp = 33000, 120
    cols = npo.pack_columns(seeded(n_var, n_samp))
    order = np.random.default_rng(20).permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        # every row of the matrix has a carrier, so bin 0 is hit only where all of a row's carriers are in neither list:
        # 20 samples stay out of both
        hist, count = check_all_modes(mat, cols, order[20:100], n_var, order[:20], "panel")
        assert (count < 0).sum() > n_var // 2 and hist[0] > 0 and hist[1] > 0


def test_several_tiles_with_a_last_one_a_single_wave_wide(dev):
    n_var, n_samp, n = 3 * 32768 + 5, 140, 130
    cols = npo.pack_columns(seeded(n_var, n_samp))
    order = np.random.default_rng(3).permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for given in ((), order[-5:]):
            check_all_modes(mat, cols, order[:n], n_var, given, len(given))


def test_two_chunks_of_unequal_size_add_up(dev):
    chunk_vars, n_samp = [32769, 100], 200
    dense = seeded(sum(chunk_vars), n_samp)
    cols = [npo.pack_columns(dense[:32769]), npo.pack_columns(dense[32769:])]
    whole = npo.pack_columns(dense)
    rng = np.random.default_rng(2)
    with uploaded(dev, cols, chunk_vars) as mat:
        for n in (1, 17, 130):
            order = rng.permutation(n_samp)
            for given in ((), order[-4:]):
                want_hist, want_count = spectrum_ref.carrier_counts(whole, order[:n], sum(chunk_vars), given)
                for mode in (0, 1, 2):
                    hist, counts, ms = mat.carrier_counts(order[:n], given, counts=True, hist_mode=mode, pass_ms=True)
                    assert (hist == want_hist).all() and ms > 0, (n, mode)
                    assert [len(c) for c in counts] == chunk_vars and (np.concatenate(counts) == want_count).all()
                parts = [host_counts(c, order[:n], v, given) for c, v in zip(cols, chunk_vars)]
                assert (sum(p[0] for p in parts) == want_hist).all()


@pytest.mark.parametrize("n_samp,lists", [(4100, (4095, 4096, 4097)), (65540, (65535, 65536))])
def test_the_wider_plane_counts(dev, n_samp, lists):
    """4,096 and 65,536 listed samples: 12 -> 16 -> 20 planes, and the end of what the LDS bins hold."""
    n_var = 65
    rng = np.random.default_rng(11)
    dense = rng.random((n_var, n_samp)) < rng.random(n_var)[:, None]
    dense[[0, 64]] = True
    cols = npo.pack_columns(dense)
    order = rng.permutation(n_samp)
    with uploaded(dev, [cols], [n_var]) as mat:
        for n in lists:
            for given in ((), order[n:n + 2]):
                hist, _ = check_all_modes(mat, cols, order[:n], n_var, given, n)
                assert hist[n] == (0 if len(given) else 2)
        with pytest.raises(dev.nat.NativeError) as e:
            mat.carrier_counts(order[:4096], hist_mode=1)                # 4,097 bins
        assert e.value.code == EINVAL


def test_rows_cleared_by_an_af_of_zero_fall_in_bin_zero(dev):
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
            hist, count = check_all_modes(mat, cleared, order[:66], n_var, given, len(given))
            assert (count[zero] == 0).all() and hist[0] >= zero.sum()


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
        before = a.carrier_counts([2, 9, 30], [50, 10])                  # valid before any reset
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        indices = list(dict.fromkeys([int(s) for s in first[0]] + [2, 9] + list(range(60, 120))))   # winners, a used and an excluded sample
        given = [50, 10, int(first[0][3])]                               # a used, an excluded and one that is listed too
        for mode in (0, 1, 2):
            hist, counts = a.carrier_counts(indices, given, counts=True, hist_mode=mode)
            want_hist, want_count = spectrum_ref.carrier_counts(whole, indices, n_var, given)
            assert (hist == want_hist).all() and (np.concatenate(counts) == want_count).all()
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        assert (a.carrier_counts([2, 9, 30], [50, 10]) == before).all()  # and the selection changes nothing of the counts


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_the_outputs(dev):
    n_var, n_samp = 9000, 30
    cols = npo.pack_columns(seeded(n_var, n_samp))
    lib = dev.nat.lib()
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        hist, count = np.full(4, 1234, np.int64), np.full(n_var, 1234, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        i64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)

        def call(idx, given=None, h=hist, c=count, n=None, n_given=None, chunk=0, mode=0):
            idx, given = i64(idx), i64(given)
            return lib.utm_carrier_counts(mat._h, chunk, p(idx), len(idx) if n is None else n, p(given),
                                          (0 if given is None else len(given)) if n_given is None else n_given, mode, p(h), p(c), None)

        assert call(None, n=2) == EINVAL                                 # NULL list with a nonzero length
        assert call([1, 2], None, n_given=1) == EINVAL                   # ... the given list
        assert call([1, 2], h=None, c=None) == EINVAL                    # both outputs NULL
        assert call([1, 2], chunk=1) == EINVAL and call([1, 2], chunk=-1) == EINVAL
        assert call([1, 30]) == EINVAL and call([-1]) == EINVAL          # index out of range
        assert call([1, 2], [30]) == EINVAL and call([1, 2], [-1]) == EINVAL
        assert call([4, 5, 4]) == EINVAL and call([4, 5], [7, 7]) == EINVAL      # a duplicate within either list
        assert call([1, 2], n=-1) == EINVAL and call([1, 2], mode=3) == EINVAL
        assert call(np.zeros(1 << 20, np.int64)) == EINVAL                # above 2^20 - 1 (and more than the matrix has)
        assert (hist == 1234).all() and (count == 1234).all()
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        want_hist, want_count = spectrum_ref.carrier_counts(cols, [7, 8, 1], n_var, [8, 2])
        assert call([7, 8, 1], [8, 2], c=None) == 0 and (hist == want_hist).all() and (count == 1234).all()
        hist[:] = 1234
        assert call([7, 8, 1], [8, 2], h=None) == 0 and (count == want_count).all() and (hist == 1234).all()
        ms = ctypes.c_double(-1.0)
        arr, given = np.asarray([7, 8, 1], dtype=np.int64), np.asarray([8, 2], dtype=np.int64)
        assert lib.utm_carrier_counts(mat._h, 0, p(arr), 3, p(given), 2, 0, p(hist), None, ctypes.byref(ms)) == 0 and ms.value > 0
        assert (hist == want_hist).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.carrier_counts([3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


# ----------------------------------------------------------------- 4. the command line
PARTS = ("chunk0", "chunk1")


@pytest.mark.parametrize("restricted", [False, True])
def test_the_command_end_to_end(dev, tmp_path, restricted):
    from utmos_amd import spectrum
    files = [os.path.join(ou.GOLD, name + ".npz") for name in PARTS]
    parts = [ou.load_part(name) for name in PARTS]
    matrix, _, samples = npo.build_matrix(parts)                         # from the ORIGINAL part files
    dense = np.asarray(matrix) != 0
    names = [str(s) for s in samples]
    subset, given = (names[3:], [names[1], names[5]]) if restricted else (names, [])
    flags = ["--subset", ",".join(subset), "--given", ",".join(given), "--maxmem", "0", "--buffer", "64"] if restricted else []
    tsv, curve, npz = str(tmp_path / "s.tsv"), str(tmp_path / "c.tsv"), str(tmp_path / "v.npz")
    spectrum.spectrum_main(flags + ["-o", tsv, "--curve-out", curve, "--counts-out", npz] + files)
    listed, panel = [names.index(s) for s in subset], [names.index(g) for g in given]
    want_hist, want_count = spectrum_ref.carrier_counts_dense(dense, listed, panel)
    assert want_hist[1:].sum() > 0
    total = int(want_hist.sum())
    assert open(tsv).read() == spectrum.SPECTRUM_HEADER + "".join(f"{c}\t{v}\t{round(int(v) / total, 4)}\n" for c, v in enumerate(want_hist))
    e = spectrum.expected_curve(want_hist)
    assert open(curve).read() == spectrum.CURVE_HEADER + "".join(
        "%d\t%.2f\t%.2f\t%s\n" % (k, e[k], e[k] - e[k - 1], round(e[k] / total, 4)) for k in range(1, len(listed) + 1))
    with np.load(npz, allow_pickle=False) as z:
        assert z["count"].dtype == np.int32 and (z["count"] == want_count).all() and (z["hist"] == want_hist).all()
        assert z["samples"].tolist() == subset and z["given"].tolist() == given
        assert [os.path.basename(f) for f in z["files"]] == [name + ".npz" for name in PARTS]
        count, part, row = z["count"], z["part"], z["row"]
    assert len(count) == len(part) == len(row) == dense.shape[0]
    for number, p in enumerate(parts):                                   # joined to the original records through part / row
        mine = part == number
        carried = np.unpackbits(p["GT"], axis=1, count=len(names))[row[mine]].astype(bool)
        masked = carried[:, panel].any(axis=1)
        assert (count[mine] == np.where(masked, -1, carried[:, listed].sum(axis=1))).all()
    assert bool((count < 0).any()) == restricted


def test_the_command_writes_the_histogram_to_stdout_and_names_an_unknown_given(dev, capfd):
    from utmos_amd import __main__ as cli
    from utmos_amd import spectrum
    part = os.path.join(ou.GOLD, "tiny.npz")
    matrix, _, samples = npo.build_matrix([ou.load_part("tiny")])
    assert cli.main(["spectrum", part]) == 0
    want, _ = spectrum_ref.carrier_counts_dense(np.asarray(matrix) != 0, range(len(samples)))
    total = int(want.sum())
    assert capfd.readouterr().out == spectrum.SPECTRUM_HEADER + "".join(f"{c}\t{v}\t{round(int(v) / total, 4)}\n" for c, v in enumerate(want))
    with pytest.raises(SystemExit) as err:
        cli.main(["spectrum", "--given", "nobody", part])
    assert err.value.code == 1 and "nobody" in capfd.readouterr().err
