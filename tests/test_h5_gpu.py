"""The reference's `--lowmem` HDF5 stores on the GPU: LZF decode and packing (utm_h5_*) byte for byte against the host
build, the reference's four store-reading cases through the CLI (repo_utils/utmos_ssshtests.sh:206-235, answer files
byte-identical), error exits, and larger generated stores against the C oracle."""
import os

import numpy as np
import pytest

import h5_gen
import oracle_util as ou
from test_h5_host import TINY, TINY_AF, dense

pytestmark = pytest.mark.gpu
CASES = ou.golden_cases()


def run_cli(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def gpu_rows(path, **kw):
    """Every batch of the device decoder, concatenated: (packed rows, af or None)."""
    from utmos_amd.h5store import ChunkDecoder, H5Store
    with ChunkDecoder(H5Store(path), 0, **kw) as dec:
        parts = list(dec)
        timing = dec.timing()
    assert [p[0] for p in parts] == sorted(p[0] for p in parts)
    assert all(v >= 0 for v in timing.values())
    rows = np.concatenate([p[1] for p in parts])
    af = None if parts[0][2] is None else np.concatenate([p[2] for p in parts])
    return rows, af


def host_rows(path):
    from utmos_amd.h5store import H5Store, pack_rows
    return pack_rows(dense(H5Store(path)))


@pytest.mark.parametrize("path", [TINY, TINY_AF])
@pytest.mark.parametrize("batching", [{}, {"max_chunks": 3}, {"max_chunks": 1, "stage_bytes": 1}])
def test_device_decode_equals_host_on_the_reference_stores(path, batching):
    rows, af = gpu_rows(path, **batching)
    e_rows, e_af = host_rows(path)
    assert np.array_equal(rows, e_rows)
    assert (af is None) == (e_af is None)
    if af is not None:
        assert af.tobytes() == e_af.tobytes()


def test_device_decode_equals_host_on_generated_stores(tmp_path):
    rng = np.random.default_rng(8)
    # a few thousand small chunks: raw ones, absent ones, a three-level B-tree, a partial last chunk
    data = rng.random((12_003, 150)) < rng.random((12_003, 1)) * 0.2
    path = h5_gen.write_store(str(tmp_path / "b.hdf5"), data, chunk_rows=4, raw={0, 7, 3000}, missing={5, 2999})
    rows, af = gpu_rows(path, max_chunks=1000)
    e_rows, _ = host_rows(path)
    assert af is None and np.array_equal(rows, e_rows)
    # float32, all-zero rows, runs of one value reaching the 8 KiB limit
    cells = h5_gen.af_matrix(rng, 4_001, 700, density=0.03, zero_rows=300)
    cells[10:20] = cells[10]
    path = h5_gen.write_store(str(tmp_path / "f.hdf5"), cells, chunk_rows=3, raw={2})
    rows, af = gpu_rows(path)
    e_rows, e_af = host_rows(path)
    assert np.array_equal(rows, e_rows) and af.tobytes() == e_af.tobytes()
    # one-row chunks (more than 250,000 columns)
    wide = h5_gen.af_matrix(rng, 3, 250_007, density=0.002, zero_rows=1)
    path = h5_gen.write_store(str(tmp_path / "w.hdf5"), wide)
    rows, af = gpu_rows(path)
    e_rows, e_af = host_rows(path)
    assert np.array_equal(rows, e_rows) and af.tobytes() == e_af.tobytes()


def test_slot_errors_leave_the_context_usable():
    from utmos_amd import _native as nat
    from utmos_amd.h5store import ChunkDecoder, H5Store
    lib = nat.lib()
    with ChunkDecoder(H5Store(TINY), 0) as dec, open(TINY, "rb") as fh:
        batch = next(dec._plan())
        assert lib.utm_h5_fetch(dec.h, None, None, None) == -4                          # nothing queued
        inflight = [dec._submit(fh, batch), dec._submit(fh, batch)]
        with pytest.raises(nat.NativeError, match="both slots") as err:
            dec._submit(fh, batch)
        assert err.value.code == -4
        e_rows = host_rows(TINY)[0]
        for k in range(3):
            _, rows, _ = dec._fetch(*inflight.pop(0))
            assert len(rows) and np.array_equal(rows, e_rows[:len(rows)])
            if k == 0:
                inflight.append(dec._submit(fh, batch))                               # into the freed slot


def test_corrupt_chunks_end_in_a_status_not_a_fault(tmp_path):
    from utmos_amd.h5store import H5Store
    s = H5Store(TINY)
    blob = bytearray(open(TINY, "rb").read())
    rng = np.random.default_rng(77)
    for k, (row, offset, size, _mask) in enumerate(s.data.chunks):
        for _ in range(3):
            blob[offset + int(rng.integers(size))] = int(rng.integers(256))
    path = tmp_path / "bad.hdf5"
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="chunk at row"):
        gpu_rows(str(path))
    rows, _ = gpu_rows(TINY)                                     # and the device is fine afterwards
    assert np.array_equal(rows, host_rows(TINY)[0])


# ---------------------------------------------------------------------------------------------- the CLI
REFERENCE_CASES = {
    "p1_lm": (["--maxmem", "1", "--lowmem", TINY], "select_first"),
    "p2_lm": (["--maxmem", "1", TINY], "select_first"),
    "af_p1_lm": (["--maxmem", "1", "-c", "20", "--lowmem", TINY_AF], "select_af_h5"),
    "af_p2_lm": (["--af", "--maxmem", "1", "-c", "20", TINY_AF], "select_af_h5"),
}


@pytest.mark.parametrize("maxmem", ["1", "0"])
@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
def test_reference_store_cases_byte_identical(name, maxmem, tmp_path):
    argv, golden = REFERENCE_CASES[name]
    argv = [maxmem if a == "1" and argv[k - 1] == "--maxmem" else a for k, a in enumerate(argv)]
    out = str(tmp_path / "out.txt")
    run_cli(argv + ["-o", out] + (["--buffer", "256"] if maxmem == "0" else []))
    assert open(out).read() == ou.golden_text(CASES[golden])


def test_af_on_a_bool_store_exits_1():
    with pytest.raises(SystemExit) as e:
        run_cli(["--af", TINY])
    assert e.value.code == 1


def test_store_with_a_mixed_row_exits_1(tmp_path, capsys):
    rng = np.random.default_rng(6)
    cells = h5_gen.af_matrix(rng, 300, 90, density=0.1)
    row = int(np.flatnonzero((cells != 0).sum(axis=1) > 1)[0])
    cells[row, np.flatnonzero(cells[row])[0]] = 2.0           # every AF is below 1
    path = h5_gen.write_store(str(tmp_path / "mixed.hdf5"), cells, chunk_rows=8)
    with pytest.raises(SystemExit) as e:
        run_cli(["--af", path])
    assert e.value.code == 1
    assert f"chunk at row {row // 8 * 8}" in capsys.readouterr().err


@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_generated_store_against_the_c_oracle(kind, tmp_path):
    """About 200k x 2,504 (the reference's chunk shape, 99 rows) built from 150 distinct chunks; the first 300 rows of
    `select -c 300` equal the packed C oracle on the same matrix (var_count from the file, all-zero rows counted)."""
    rng = np.random.default_rng(21 if kind == "bool" else 22)
    n_samples, chunk_rows = 2504, h5_gen.chunk_rows_for(2504)
    n_chunks, n_distinct = 2021, 150
    n_var = n_chunks * chunk_rows - 40                     # a partial last chunk
    blocks, afs = [], []
    for k in range(n_distinct + 1):                        # the last one is the tail: its last 40 rows are fill
        gt = rng.random((chunk_rows, n_samples)) < rng.random() * 0.02 * rng.random((chunk_rows, 1))
        if k == n_distinct:
            gt[-40:] = False
        af = (rng.integers(1, 5008, chunk_rows) / 5008).astype(np.float32) * gt.any(axis=1)
        blocks.append(gt)
        afs.append(af.astype(np.float32))
    order = np.append(rng.integers(0, n_distinct, n_chunks - 1), n_distinct)
    chunks, chunks_of = [], {}
    for k, b in enumerate(order):
        if b not in chunks_of:
            cells = blocks[b] if kind == "bool" else np.where(blocks[b], afs[b][:, None], np.float32(0)).astype(np.float32)
            chunks_of[b] = h5_gen.encode_chunks(cells, chunk_rows)[0][1:]
        chunks.append((k * chunk_rows,) + chunks_of[b])
    present = np.concatenate([blocks[b] for b in order])[:n_var]
    dtype = np.bool_ if kind == "bool" else np.float32
    path = h5_gen.write_store(str(tmp_path / f"big_{kind}.hdf5"), chunks=chunks, shape=(n_var, n_samples),
                              dtype=dtype, var_count=present.sum(axis=0), chunk_rows=chunk_rows)
    out = str(tmp_path / "out.txt")
    run_cli((["--af"] if kind == "float32" else []) + ["-c", "300", "-o", out, path])
    got = [line.split("\t") for line in open(out).read().splitlines()[1:]]
    cols = ou.npo.pack_columns(present)
    af = np.concatenate([afs[b] for b in order])[:n_var] if kind == "float32" else None
    idx, new, _ = ou.c_greedy(cols, n_var, np.ones(n_samples, np.uint8), af=af, k_max=300)
    names = [f"S{k:06d}" for k in range(n_samples)]
    assert [g[0] for g in got] == [names[i] for i in idx]
    assert [int(g[2]) for g in got] == new.tolist()
    assert [int(g[1]) for g in got] == present.sum(axis=0)[idx].tolist()
    assert float(got[-1][4]) == round(int(got[-1][3]) / n_var, 4)


def test_two_ranks_on_one_gpu_read_their_blocks_of_a_store(tmp_path):
    from test_gpu_cli import _run_two_ranks
    out = str(tmp_path / "out.txt")
    res = _run_two_ranks(["--maxmem", "1", "-o", out, TINY], 37500 + os.getpid() % 2000)
    assert res == {0: "ok", 1: "ok"}
    assert open(out).read() == ou.golden_text(CASES["select_first"])
