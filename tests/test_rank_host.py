"""Capture ranks without a GPU: the CPU build of k_capture_rank's walk against the numpy restatement (tests/rank_ref.py),
the restatement against what the reference's own code recorded (tests/golden/order, tests/golden/traces), the loader's
origin bookkeeping, the command line's refusals and tools/capture_spectrum.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as ou
import order_ref
import rank_ref
from oracle_util import npo

DEPTHS = [1, 2, 3, 4, 7, 8, 255]
EINVAL = -1


def host_rank(cols, order, m, n_var):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    order32 = np.ascontiguousarray(order, dtype=np.uint32)
    out = np.full(n_var, 77, dtype=np.int32)                 # (every entry has to be written)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_capture_rank_host(p(cols), cols.shape[1], n_var, p(order32), len(order32), m, p(out)))
    return out


def filled(rng, n_var, n_samp, fill):
    """Packed columns of a seeded matrix: 'sparse' = the 1/c carrier spectrum of the other tests, 'dense' = about two
    carriers in three, so that high depths are reached."""
    dense = ou.random_dense(rng, n_var, n_samp) if fill == "sparse" else ou.random_dense(rng, n_var, n_samp, density=0.65, sfs=False)
    return npo.pack_columns(dense)


@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("m", DEPTHS)
def test_cpu_build_equals_the_restatement(m, n_var, fill):
    rng = np.random.default_rng(1000 * m + n_var)
    n_samp = 80
    cols = filled(rng, n_var, n_samp, fill)
    for length in (0, 1, 15, 16, 17, 70):
        order = rng.permutation(n_samp)[:length]
        want = rank_ref.capture_rank(cols, order, m, n_var)
        assert (host_rank(cols, order, m, n_var) == want).all(), length
        if length == 70 and fill == "dense" and m <= 8 and n_var >= 63:
            assert (want >= 0).any()                          # the depth is reached somewhere: the case says something


@pytest.mark.parametrize("m", [8, 254, 255])
def test_depth_255_on_a_dense_matrix_with_enough_listed_samples(m):
    rng = np.random.default_rng(m)
    n_var, n_samp = 1000, 300
    dense = rng.random((n_var, n_samp)) < 0.93
    dense[:10] = True                                         # carried by everyone: captured exactly at position m - 1
    cols = npo.pack_columns(dense)
    order = rng.permutation(n_samp)[:290]
    want = rank_ref.capture_rank(cols, order, m, n_var)
    got = host_rank(cols, order, m, n_var)
    assert (got == want).all()
    assert (got[:10] == m - 1).all() and (got >= 0).sum() > n_var // 2 and got.max() > m - 1


def test_rank_is_the_first_carrier_and_padding_is_never_touched():
    cols = np.zeros((3, 2), np.uint64)
    cols[0, 0] = 0b0101
    cols[1, 0] = 0b0110
    cols[2, 1] = np.uint64(1) << np.uint64(5)                 # variant 69: past n_var below
    cols[1, 1] = np.uint64(1) << np.uint64(3)                 # variant 67
    assert host_rank(cols, [0, 1, 2], 1, 68).tolist()[:4] == [0, 1, 0, -1]
    assert host_rank(cols, [1, 0, 2], 1, 68).tolist()[:4] == [1, 0, 0, -1]
    assert host_rank(cols, [0, 1, 2], 2, 68).tolist()[:4] == [-1, -1, 1, -1]
    assert host_rank(cols, [0, 1, 2], 1, 68)[67] == 1 and host_rank(cols, [0, 2], 1, 68)[64:].tolist() == [-1] * 4


def test_cpu_build_refuses_bad_arguments_and_leaves_the_output():
    from utmos_amd import _native as nat
    cols, order, out = np.zeros((2, 1), np.uint64), np.array([0, 1], np.uint32), np.full(10, 5, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib = nat.lib()
    assert lib.utm_capture_rank_host(p(cols), 1, 10, p(order), 2, 0, p(out)) == EINVAL
    assert lib.utm_capture_rank_host(p(cols), 1, 10, p(order), 2, 256, p(out)) == EINVAL
    assert lib.utm_capture_rank_host(p(cols), 1, 10, None, 2, 1, p(out)) == EINVAL
    assert lib.utm_capture_rank_host(p(cols), 1, 65, p(order), 2, 1, p(out)) == EINVAL       # more variants than words
    assert lib.utm_capture_rank_host(p(cols), 1, 10, p(order), 2, 1, None) == EINVAL
    assert (out == 5).all()
    assert lib.utm_capture_rank_host(p(cols), 1, 10, None, 0, 1, p(out)) == 0 and (out == -1).all()


# ----------------------------------------------------------------- anchored on what the reference's own code recorded
@pytest.mark.parametrize("name", order_ref.case_names())
def test_bincount_of_the_ranks_is_the_reference_made_gain_list(name):
    t = order_ref.load_case(name)
    order = t["order"][:len(t["gains"])] + t["cont_idx"]
    gains = t["gains"] + t["cont_gains"]
    rank = host_rank(t["cols"], order, 1, t["n_var"])
    assert (rank == rank_ref.capture_rank(t["cols"], order, 1, t["n_var"])).all()
    assert np.bincount(rank[rank >= 0], minlength=len(order)).tolist() == gains


def traces_from_scratch():
    names = []
    for name in ou.trace_names():
        t = ou.load_trace(name)
        if "state" in t and (np.asarray(t["state"]) == 0).any():
            continue                                          # a sample used from the start captures without a row
        names.append(name)
    return names


@pytest.mark.parametrize("name", traces_from_scratch())
def test_bincount_of_the_ranks_is_the_trace_s_new_count_column(name):
    t = ou.load_trace(name)
    kw = ou.trace_options(t)
    matrix, _, samples = npo.build_matrix(t["part_list"], af=kw.get("af", False), af_dtype=kw.get("af_dtype", "f64"))
    cols = npo.pack_columns(matrix != 0)                      # with AF, rows whose AF is 0 hold nothing
    rows = [line.split("\t") for line in t["tsv"].splitlines()[1:]]
    position = {str(s): i for i, s in enumerate(samples)}
    order = [position[r[0]] for r in rows]
    if "idx" in t:
        assert order == t["idx"]
    rank = host_rank(cols, order, 1, matrix.shape[0])
    assert np.bincount(rank[rank >= 0], minlength=len(order)).tolist() == [int(r[2]) for r in rows]
    if rows:
        assert int((rank >= 0).sum()) == int(rows[-1][3])     # tot_captured of the last row


def test_the_anchors_include_traces_with_rows():
    assert {"all_int", "all_af64", "af_zero_rows", "compaction_int", "ties_int"} <= set(traces_from_scratch())
    assert "initial_used_int" not in traces_from_scratch()


# ----------------------------------------------------------------- origin bookkeeping of the loader
class _NoDevice:
    """Stands in for a DeviceMatrix where the chunk builder only hands chunks over."""

    def __init__(self):
        self.chunk_vars = []

    def add_chunk(self, n_var):
        self.chunk_vars.append(int(n_var))
        return len(self.chunk_vars) - 1

    def upload_rows_packed(self, chunk, rows):
        assert len(rows) == self.chunk_vars[chunk]


@pytest.mark.parametrize("maxmem,buffer", [(2, 32768), (0, 64), (0, 200)])
def test_origin_travels_with_the_rows_through_merging_and_cutting(maxmem, buffer, monkeypatch):
    from utmos_amd import select
    monkeypatch.setattr(select, "MAXMEM", maxmem)
    rng = np.random.default_rng(buffer)
    n_samp, masks = 24, []
    matrix = _NoDevice()
    with_origin = select._ChunkBuilder(matrix, None, False, False)
    plain = select._ChunkBuilder(_NoDevice(), None, False, False)
    all_rows = []
    for part, n_rec in enumerate([150, 1, 77, 300]):
        rows = np.packbits(rng.random((n_rec, n_samp)) < 0.08, axis=1)
        informative = rows.any(axis=1)
        if part == 1:
            informative[:] = rows[:] = 0                      # a part whose every record is dropped
        masks.append(informative)
        kept = rows[informative]
        if len(kept) == 0:
            continue                                          # (load_files skips it the same way)
        af = rng.random(len(kept))
        select._place_part(with_origin, kept, af, n_samp, False, buffer, select.part_origin(part, informative))
        select._place_part(plain, kept, af, n_samp, False, buffer)
        all_rows.append(kept)
    with_origin.flush()
    plain.flush()
    assert not (~masks[0]).all() and (~masks[0]).any()         # records were dropped in between: row != matrix position
    assert [len(o) for o in with_origin.chunk_origin] == matrix.chunk_vars
    if maxmem == 0:
        assert len(matrix.chunk_vars) > 3 and max(matrix.chunk_vars) <= buffer // 64 * 64
    got = select.chunks_origin(with_origin.chunk_origin, with_origin.chunk_af)
    part, row = rank_ref.variant_origin(masks)
    assert got["part"].dtype == np.int32 and got["row"].dtype == np.int64
    assert got["part"].tolist() == part.tolist() and got["row"].tolist() == row.tolist()
    assert len(got["af"]) == len(part) == sum(len(r) for r in all_rows)
    # off by default: nothing is carried
    assert plain.chunk_origin == [] and plain.origin == []
    assert [len(a) for a in plain.chunk_af] == matrix.chunk_vars


def test_a_store_s_origin_is_its_own_row_numbers():
    from utmos_amd import select
    got = select.store_origin(5, [np.array([0.1, 0.2], np.float32), np.array([0.3, 0.4, 0.5], np.float32)])
    assert got["part"].tolist() == [0] * 5 and got["row"].tolist() == [0, 1, 2, 3, 4] and got["af"].dtype == np.float32
    assert len(got["af"]) == 5 and select.store_origin(3)["af"] is None


# ----------------------------------------------------------------- command line
def test_several_processes_refuse_variants_out_before_loading(monkeypatch, capsys, tmp_path):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--variants-out", str(tmp_path / "v.npz"), "does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err
    assert not (tmp_path / "v.npz").exists()


def test_the_flag_defaults_to_off_and_is_not_in_the_options_line_then(capsys):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])                       # (the command logs to stderr)
    assert args.variants_out is None
    line = capsys.readouterr().err
    assert "options in effect" in line and "variants_out" not in line
    select.parse_args(["--variants-out", "v.npz", "x.npz"])
    assert '"variants_out": "v.npz"' in capsys.readouterr().err


# ----------------------------------------------------------------- the consumer
def test_capture_spectrum_reads_the_file_and_prints_fractions_per_af_bin(tmp_path):
    path = str(tmp_path / "v.npz")
    # 4 rare variants (AF 0.001): ranks 0, 5, -1, -1; 4 common ones (AF 0.3): ranks 0, 0, 1, 9
    np.savez(path, rank=np.array([0, 5, -1, -1, 0, 0, 1, 9], np.int32), part=np.zeros(8, np.int32), row=np.arange(8),
             af=np.array([0.001] * 4 + [0.3] * 4), samples=np.array([f"S{i}" for i in range(10)]), files=np.array(["a.npz"]),
             depth=np.int32(1))
    tool = os.path.join(ou.ROOT, "tools", "capture_spectrum.py")
    out = subprocess.run([sys.executable, tool, path, "-k", "1", "6", "10", "--bins", "0.01", "0.05"], capture_output=True, text=True,
                         check=True).stdout
    table = [line.split("\t") for line in out.strip().splitlines()]
    assert table[0] == ["af_bin", "variants", "k=1", "k=6", "k=10"]
    assert table[1] == ["[0,0.01)", "4", "0.2500", "0.5000", "0.5000"]
    assert table[2] == ["[0.01,0.05)", "0", "nan", "nan", "nan"]
    assert table[3] == ["[0.05,1]", "4", "0.5000", "0.7500", "1.0000"]
    assert table[4] == ["all", "8", "0.3750", "0.6250", "0.7500"]
