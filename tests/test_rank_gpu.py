"""GPU: capture ranks through the C ABI (utm_capture_rank / k_capture_rank), DeviceMatrix.capture_rank and
`select --variants-out`.

The ranks are held against the numpy restatement (tests/rank_ref.py) and the CPU build of the kernel's walk bit for bit,
against the engine's own rows (bincount of the ranks = new_count, rank >= 0 = covered, at_depth, support), and the
command line's file against the ORIGINAL part files through its part / row columns.  The launch takes one workgroup per
4 KiB tile of the variant axis and is not capped, so no shape has to exceed a cap."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import rank_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
DEPTHS = [1, 2, 3, 4, 7, 8, 255]
LENGTHS = (0, 1, 15, 16, 17, 70)
N_SAMP = 80
TIMING = ("score_ms", "loop_ms")              # utm_stats fields that are measurements


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


@functools.lru_cache(maxsize=None)
def seeded_cols(n_var, fill, n_samp=N_SAMP):
    rng = np.random.default_rng(n_var * 3 + len(fill))
    dense = ou.random_dense(rng, n_var, n_samp) if fill == "sparse" else ou.random_dense(rng, n_var, n_samp, density=0.65, sfs=False)
    cols = npo.pack_columns(dense)
    cols.setflags(write=False)
    return cols


def host_rank(cols, order, m, n_var):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    order32 = np.ascontiguousarray(order, dtype=np.uint32)
    out = np.zeros(n_var, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_capture_rank_host(p(cols), cols.shape[1], n_var, p(order32), len(order32), m, p(out)))
    return out


def uploaded(dev, cols_per_chunk, chunk_vars):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0])
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def covered_bits(m):
    return np.concatenate([np.unpackbits(m.covered(c).view(np.uint8), bitorder="little")[:n] for c, n in enumerate(m.chunk_vars)])


def ranks_all(m, order, depth=1):
    return np.concatenate([m.capture_rank(c, order, depth) for c in range(len(m.chunk_vars))])


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
SHAPES = [(n, f) for n in (1, 63, 64, 65, 1000) for f in ("sparse", "dense")] + \
         [(n, "sparse") for n in (32767, 32768, 32769, 100003)]           # the 4 KiB tile edge; a last tile that ends inside a lane's two words


@pytest.mark.parametrize("n_var,fill", SHAPES)
@pytest.mark.parametrize("m", DEPTHS)
def test_ranks_equal_the_restatement_and_the_cpu_build(dev, m, n_var, fill):
    cols = seeded_cols(n_var, fill)
    rng = np.random.default_rng(m * 7 + n_var)
    with uploaded(dev, [cols], [n_var]) as mat:
        for length in LENGTHS:
            order = rng.permutation(N_SAMP)[:length]
            got = mat.capture_rank(0, order, m)
            assert got.dtype == np.int32 and got.shape == (n_var,)
            assert (got == rank_ref.capture_rank(cols, order, m, n_var)).all(), length
            assert (got == host_rank(cols, order, m, n_var)).all(), length


@pytest.mark.parametrize("m", [8, 255])
def test_depth_255_on_a_dense_matrix(dev, m):
    rng = np.random.default_rng(m)
    n_var, n_samp = 33000, 300
    dense = rng.random((n_var, n_samp)) < 0.93
    dense[:10] = True
    cols = npo.pack_columns(dense)
    order = rng.permutation(n_samp)[:290]
    with uploaded(dev, [cols], [n_var]) as mat:
        got = mat.capture_rank(0, order, m)
    assert (got == rank_ref.capture_rank(cols, order, m, n_var)).all() and (got == host_rank(cols, order, m, n_var)).all()
    assert (got[:10] == m - 1).all() and (got >= 0).sum() > n_var // 2


def test_two_chunks_and_a_list_with_an_excluded_and_a_used_sample(dev):
    chunk_vars = [5000, 70001]
    cols = [seeded_cols(n, "sparse") for n in chunk_vars]
    state = np.ones(N_SAMP, np.uint8)
    state[[3, 40]] = 0
    state[[7, 41, 42]] = 2
    order = [40, 5, 7, 3, 60, 41, 11] + list(range(20, 30))
    with uploaded(dev, cols, chunk_vars) as mat:
        before = [mat.capture_rank(c, order, 2) for c in range(2)]      # valid before any reset
        mat.set_state(state)
        mat.reset()
        winners = mat.run(3)[0].tolist()                                 # winners of the loop are used too
        listed = order + [w for w in winners if w not in order]
        for c, n_var in enumerate(chunk_vars):
            for m in (1, 2, 3):
                assert (mat.capture_rank(c, listed, m) == rank_ref.capture_rank(cols[c], listed, m, n_var)).all()
            assert (mat.capture_rank(c, order, 2) == before[c]).all()    # it starts from an empty mask whatever the states are
            assert (mat.capture_rank(c, [], 1) == -1).all()


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_rows_cleared_by_an_af_of_zero_come_out_minus_one(dev, kind):
    rng = np.random.default_rng(5)
    n_var, n_samp = 33000, 60
    dense = ou.random_dense(rng, n_var, n_samp)
    af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0
    zero = rng.random(n_var) < 0.05
    zero[[0, 63, 64, n_var - 1]] = True
    af[zero] = 0.0
    cleared = npo.pack_columns(dense & ~zero[:, None])
    order = rng.permutation(n_samp)[:40]
    with dev.DeviceMatrix(n_samp) as mat:
        c = mat.add_chunk(n_var)
        mat.upload_columns(c, npo.pack_columns(dense))
        mat.set_af(c, af.astype(np.float32 if kind == "f32" else np.float64))
        for m in (1, 2):
            got = mat.capture_rank(c, order, m)
            assert (got[zero] == -1).all()
            assert (got == rank_ref.capture_rank(cleared, order, m, n_var)).all()
        assert (mat.capture_rank(c, np.arange(n_samp), 1)[~zero] >= 0).all()


# ----------------------------------------------------------------- 2. stateless
@pytest.mark.parametrize("kind,depth", [(None, 1), ("f32", 1), (None, 2)])
def test_a_call_in_between_changes_nothing_of_the_selection(dev, kind, depth):
    rng = np.random.default_rng(21)
    n_var, n_samp, k = 40_000, 120, 25
    dense = ou.random_dense(rng, n_var, n_samp)
    af = (rng.integers(1, 2 * n_samp, n_var) / (2.0 * n_samp)).astype(np.float32)
    chunk_vars = [25_000, 15_000]
    cols = [npo.pack_columns(dense[:25_000]), npo.pack_columns(dense[25_000:])]
    state = np.ones(n_samp, np.uint8)
    state[[2, 50]] = 0
    state[[9, 10]] = 2
    a, b = uploaded(dev, cols, chunk_vars), uploaded(dev, cols, chunk_vars)
    with a, b:
        for mat in (a, b):
            if kind:
                mat.set_af(0, af[:25_000])
                mat.set_af(1, af[25_000:])
            mat.set_state(state)
            mat.set_depth(depth)
            mat.reset()
        first_a, first_b = a.run(k), b.run(k)
        order = [int(s) for s in first_a[0]] + [2, 9]
        ranks = ranks_all(a, order, depth)                               # ... between two batches, on `a` only
        assert all(x.tolist() == y.tolist() for x, y in zip(first_a, first_b))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert (covered_bits(a) == covered_bits(b)).all()
        ranks_all(a, order[::-1], 3)
        second_a, second_b = a.run(k), b.run(k)
        assert len(second_b[0]) == k
        assert all(x.tolist() == y.tolist() for x, y in zip(second_a, second_b))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert (covered_bits(a) == covered_bits(b)).all()
        if depth > 1:
            assert a.at_depth(0, 2 * k).tolist() == b.at_depth(0, 2 * k).tolist()
        assert (ranks_all(a, order, depth) == ranks).all()               # and the selection changes nothing of the ranks


# ----------------------------------------------------------------- 3. against the engine
def engine_matrix(dev, config):
    rng = np.random.default_rng(31)
    if config == "persistent":
        n_var, n_samp, chunk_vars = 70_000, 300, [70_000]
    else:
        n_var, n_samp, chunk_vars = 30_000, 100, [16_000, 14_000]
    dense = ou.random_dense(rng, n_var, n_samp)
    cols, lo = [], 0
    for n in chunk_vars:
        cols.append(npo.pack_columns(dense[lo:lo + n]))
        lo += n
    mat = uploaded(dev, cols, chunk_vars)
    if config == "af64":
        af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0
        af[rng.random(n_var) < 0.03] = 0.0
        lo = 0
        for c, n in enumerate(chunk_vars):
            mat.set_af(c, af[lo:lo + n])
            lo += n
    mat.set_decremental(config == "decremental")
    return mat, n_samp


@pytest.mark.parametrize("config", ["int", "af64", "decremental", "persistent"])
def test_ranks_of_a_select_all_are_its_rows(dev, config):
    mat, n_samp = engine_matrix(dev, config)
    with mat:
        mat.reset()
        winners, new_count, _ = mat.run(n_samp)
        st = mat.stats()
        if config == "decremental":
            assert st["decr_iterations"] > 0
        if config == "persistent":
            assert st["persist_iterations"] > 0
        assert len(winners) > 20
        rank = ranks_all(mat, winners, 1)
        assert np.bincount(rank[rank >= 0], minlength=len(winners)).tolist() == new_count.tolist()
        assert ((rank >= 0) == covered_bits(mat).astype(bool)).all()


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("config", ["int", "af64"])
def test_ranks_at_a_depth_are_the_engine_s_at_depth_and_support(dev, config, depth):
    mat, n_samp = engine_matrix(dev, config)
    with mat:
        mat.set_depth(depth)
        mat.reset()
        winners = mat.run(n_samp)[0]
        assert len(winners) > 20
        rank = ranks_all(mat, winners, depth)
        assert np.cumsum(np.bincount(rank[rank >= 0], minlength=len(winners))).tolist() == mat.at_depth(0, len(winners)).tolist()
        support = np.concatenate([mat.support(c) for c in range(len(mat.chunk_vars))])
        assert ((rank >= 0) == (support == depth)).all()
        first = ranks_all(mat, winners, 1)
        both = (rank >= 0) & (first >= 0)
        assert (first[both] < rank[both]).all() and ((rank >= 0) <= (first >= 0)).all()


# ----------------------------------------------------------------- 4. errors
def test_bad_arguments_are_refused_and_leave_the_output(dev):
    n_var = 9000
    cols = seeded_cols(n_var, "sparse", 30)
    lib = dev.nat.lib()
    with uploaded(dev, [cols], [n_var]) as mat:
        winners = mat.run(3)[0]
        covered, stats = mat.covered(0), deterministic(mat.stats())
        out = np.full(n_var, 1234, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

        def call(chunk, idx, m, dest=out, n=None):
            arr = None if idx is None else np.asarray(idx, dtype=np.int64)
            return lib.utm_capture_rank(mat._h, chunk, p(arr), len(arr) if n is None else n, m, p(dest), None)

        assert call(0, None, 1, n=2) == EINVAL                           # NULL list with n > 0
        assert call(0, [1, 2], 1, dest=None) == EINVAL                   # NULL output
        assert call(1, [1, 2], 1) == EINVAL and call(-1, [1, 2], 1) == EINVAL      # chunk out of range
        assert call(0, [1, 30], 1) == EINVAL and call(0, [-1], 1) == EINVAL        # index out of range
        assert call(0, [4, 5, 4], 1) == EINVAL                           # duplicate
        assert call(0, [1, 2], 0) == EINVAL and call(0, [1, 2], 256) == EINVAL and call(0, [1, 2], -3) == EINVAL
        assert call(0, [1, 2], 1, n=-1) == EINVAL
        assert b"argument" in lib.utm_last_error()
        assert (out == 1234).all()
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        # the context works afterwards; a winner of the loop is an ordinary member of a list
        order = [int(winners[0]), 7, 8]
        assert call(0, order, 1) == 0 and (out == rank_ref.capture_rank(cols, order, 1, n_var)).all()
        ms = ctypes.c_double(-1.0)
        arr = np.asarray(order, dtype=np.int64)
        assert lib.utm_capture_rank(mat._h, 0, p(arr), 3, 2, p(out), ctypes.byref(ms)) == 0 and ms.value > 0
        assert (out == rank_ref.capture_rank(cols, order, 2, n_var)).all()
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = seeded_cols(n_var, "sparse", 8)
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.capture_rank(c, [3])
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


# ----------------------------------------------------------------- 5. the command line
PARTS = ("chunk0", "chunk1")


def run_cli(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def part_files():
    return [os.path.join(ou.GOLD, name + ".npz") for name in PARTS]


@functools.lru_cache(maxsize=None)
def original_parts():
    return [ou.load_part(name) for name in PARTS]


def check_against_the_original_parts(z, tsv, depth=1, af=False):
    """Every variant of the file, looked up in the ORIGINAL part it names: the selected sample at rank[v] brings the number
    of selected carriers of record row[v] of file part[v] to `depth`, and no earlier one does; rank -1: they never do."""
    parts = original_parts()
    names = [str(s) for s in parts[0]["samples"]]
    rows = [line.split("\t") for line in tsv.splitlines()[1:]]
    assert z["samples"].tolist() == [r[0] for r in rows] and int(z["depth"]) == depth
    selected = [names.index(r[0]) for r in rows]
    rank, part, row = z["rank"], z["part"], z["row"]
    assert rank.dtype == np.int32 and part.dtype == np.int32 and row.dtype == np.int64
    assert np.bincount(rank[rank >= 0], minlength=len(rows)).tolist() == [int(r[2]) for r in rows] or depth > 1
    informative = [np.unpackbits(p["GT"], axis=1, count=len(names)).any(axis=1) for p in parts]
    want_part, want_row = rank_ref.variant_origin(informative)
    assert part.tolist() == want_part.tolist() and row.tolist() == want_row.tolist()
    assert [os.path.basename(f) for f in z["files"]] == [name + ".npz" for name in PARTS]
    for number, p in enumerate(parts):
        mine = part == number
        carried = np.unpackbits(p["GT"], axis=1, count=len(names))[row[mine]][:, selected].astype(np.int32)
        values = np.asarray(p["AF"], np.float64).reshape(-1)[row[mine]]
        assert (z["af"][mine] == values).all()
        if af:
            carried[values == 0] = 0                                     # the reference's float matrix holds nothing there
        for m, key in ((depth, "rank"),) + (((1, "first_rank"),) if depth > 1 else ()):
            reached = np.cumsum(carried, axis=1) == m
            want = np.where(reached.any(axis=1), reached.argmax(axis=1), -1)
            assert (z[key][mine] == want).all(), (number, key)
    if depth > 1:
        both = (rank >= 0) & (z["first_rank"] >= 0)
        assert (z["first_rank"][both] <= rank[both]).all()
        assert np.cumsum(np.bincount(rank[rank >= 0], minlength=len(rows))).tolist() == [int(r[5]) for r in rows]
    else:
        assert "first_rank" not in z.files


@pytest.mark.parametrize("extra,depth,af", [
    ([], 1, False),
    (["--maxmem", "0", "--buffer", "64"], 1, False),
    (["--include", "SAMPLES 900 5", "--mode", "topN"], 1, False),
    (["--af"], 1, True),
    (["--depth", "2"], 2, False),
    (["--depth", "2", "--maxmem", "0", "--buffer", "64", "--af"], 2, True),
], ids=["plain", "many-chunks", "include-topN", "af", "depth2", "depth2-af-chunks"])
def test_cli_file_leads_back_to_the_original_records(extra, depth, af, tmp_path):
    plain, with_flag, npz = str(tmp_path / "plain.tsv"), str(tmp_path / "flag.tsv"), str(tmp_path / "variants.npz")
    names = [str(s) for s in original_parts()[0]["samples"]]
    extra = [",".join(names[int(i)] for i in x.split()[1:]) if x.startswith("SAMPLES") else x for x in extra]
    argv = ["-c", "30"] + extra
    run_cli(argv + ["-o", plain] + part_files())
    run_cli(argv + ["-o", with_flag, "--variants-out", npz] + part_files())
    tsv = open(with_flag).read()
    assert tsv == open(plain).read() and tsv.count("\n") > 10           # the TSV is byte-identical with and without
    with np.load(npz, allow_pickle=False) as z:
        check_against_the_original_parts(z, tsv, depth, af)


@pytest.mark.parametrize("af", [False, True])
def test_cli_file_from_an_hdf5_store_written_by_lowmem(af, tmp_path):
    store = str(tmp_path / "store.hdf5")
    flags = ["-c", "30"] + (["--af"] if af else [])
    direct_tsv, direct_npz = str(tmp_path / "a.tsv"), str(tmp_path / "a.npz")
    run_cli(flags + ["--lowmem", store, "-o", direct_tsv, "--variants-out", direct_npz] + part_files())
    back_tsv, back_npz = str(tmp_path / "b.tsv"), str(tmp_path / "b.npz")
    run_cli(flags + ["-o", back_tsv, "--variants-out", back_npz, store])
    assert open(back_tsv).read() == open(direct_tsv).read()
    rows = [line.split("\t") for line in open(back_tsv).read().splitlines()[1:]]
    with np.load(direct_npz, allow_pickle=False) as a, np.load(back_npz, allow_pickle=False) as b:
        assert (b["rank"] == a["rank"]).all() and b["samples"].tolist() == a["samples"].tolist()
        assert (b["part"] == 0).all() and b["row"].tolist() == list(range(len(a["rank"])))
        assert b["files"].tolist() == [store]
        assert np.bincount(b["rank"][b["rank"] >= 0], minlength=len(rows)).tolist() == [int(r[2]) for r in rows]
        if af:
            assert b["af"].dtype == np.float32 and (b["af"] == a["af"].astype(np.float32)).all()
        else:
            assert "af" not in b.files
        check_against_the_original_parts(a, open(direct_tsv).read(), 1, af)


def test_cli_run_that_selects_nothing_still_writes_the_file(tmp_path):
    out, npz = str(tmp_path / "out.tsv"), str(tmp_path / "variants.npz")
    names = [str(s) for s in original_parts()[0]["samples"]]
    run_cli(["-c", "5", "--exclude", ",".join(names), "-o", out, "--variants-out", npz] + part_files())
    assert open(out).read().count("\n") == 1
    with np.load(npz, allow_pickle=False) as z:
        assert len(z["rank"]) == len(z["row"]) > 0 and (z["rank"] == -1).all() and len(z["samples"]) == 0


def test_cli_refuses_several_processes_before_touching_a_gpu(monkeypatch, capsys, tmp_path):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--variants-out", str(tmp_path / "v.npz")] + part_files())
    assert err.value.code == 1 and "single process" in capsys.readouterr().err
