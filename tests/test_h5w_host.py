"""Writing the reference's `--lowmem` HDF5 store without a GPU: the CPU build of the device's LZF encoder
(utm_lzf_encode_host) against every stored chunk of the reference's two stores and against a plain Python restatement
(tests/lzf_ref.py), round trips through the decoder, and utmos_amd/h5write.py fed by the host encoder: byte-identical
to the reference's files, and stores of other shapes read back exactly through H5Store."""
import ctypes
import os

import numpy as np
import pytest

import lzf_ref
import oracle_util as ou
from test_h5_host import TINY, TINY_AF, dense


def encode(raw, cap=None):
    from utmos_amd.h5write import lzf_host
    return lzf_host(bytes(raw), cap)


def decode(blob, n):
    from utmos_amd.h5store import lzf_decode
    return lzf_decode(blob, n)


def stored_chunks(path):
    """(decoded bytes, stored bytes) of every chunk of the three datasets."""
    from utmos_amd.h5store import H5Store
    s = H5Store(path)
    blob = open(path, "rb").read()
    s.fh = open(path, "rb")
    try:
        entries = s._group(*_root(blob))
        datasets = [s._dataset(name, entries[name]) for name in ("data", "samples", "var_count")]
    finally:
        s.fh.close()
    out = []
    for ds in datasets:
        for _row, at, size, mask in ds.chunks:
            assert mask == 0
            out.append((decode(blob[at:at + size], ds.chunk_bytes), blob[at:at + size]))
    return out


def _root(blob):
    import struct
    return struct.unpack_from("<QQ", blob, 80)                    # the superblock's cached B-tree and heap


@pytest.mark.parametrize("path", [TINY, TINY_AF])
def test_host_encoder_reproduces_every_stored_chunk(path):
    chunks = stored_chunks(path)
    assert len(chunks) == (15 if path == TINY else 25)             # data + 2 samples + 2 var_count chunks
    for raw, stored in chunks:
        assert encode(raw) == stored
        assert lzf_ref.lzf_compress(raw) == stored


def round_trip_cases():
    rng = np.random.default_rng(5)
    period = rng.integers(0, 256, 8192, dtype=np.uint8).tobytes()
    return {
        "empty": b"", "1": b"a", "2": b"ab", "3": b"abc", "4": b"abcd",
        "zeros": bytes(247_896), "ones": b"\x01" * 10_016,
        "match264": b"xy" + b"q" * 600 + b"z",
        "back8192": period + period[:3000] + bytes(50),
        "back8193": period + b"!" + period[:3000],
        "random": rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(),
        "sparse": (rng.random(200_000) < 0.01).astype(np.uint8).tobytes(),
    }


@pytest.mark.parametrize("name", sorted(round_trip_cases()))
def test_round_trips_and_agrees_with_the_python_restatement(name):
    raw = round_trip_cases()[name]
    roomy = len(raw) + len(raw) // 16 + 64
    for cap in (len(raw), roomy):
        got = encode(raw, cap)
        assert got == lzf_ref.lzf_compress(raw, cap)
        if got is not None:
            assert len(got) <= cap
            assert decode(got, len(raw)) == raw
    if len(raw) >= 1:
        assert encode(raw, roomy) is not None                      # with room, everything encodes
    if len(raw) < 4:
        assert encode(raw) is None                                 # in its own size: too short (stored raw)


def test_incompressible_chunk_takes_the_raw_path():
    from utmos_amd.h5write import store_chunk
    raw = np.random.default_rng(9).integers(0, 256, 247_896, dtype=np.uint8).tobytes()
    assert encode(raw) is None
    assert store_chunk(raw) == (raw, 1)
    zeros = bytes(247_896)
    blob, mask = store_chunk(zeros)
    assert mask == 0 and decode(blob, len(zeros)) == zeros


def test_long_match_and_far_reference_tokens():
    raw = b"xy" + b"q" * 600 + b"z"
    blob = encode(raw, 100)
    assert blob[0:1] == b"\x02"                                    # "xyq" literal run
    assert blob[4] == 0xE0 and blob[5] == 264 - 9                   # a match of 264 bytes, one back
    period = np.random.default_rng(1).integers(0, 256, 8192, dtype=np.uint8).tobytes()
    raw = period + period[:100] + bytes(20)
    blob = encode(raw, len(raw) + 400)
    assert bytes([0xE0 | 31, 99 - 9, 0xFF]) in blob                 # 99 bytes, 8,192 back (position 0 is never a
    #                                                                  reference, so the match starts one byte in)


def parts(names):
    rows, afs, samples = [], [], None
    for name in names:
        with np.load(os.path.join(ou.GOLD, f"{name}.npz")) as z:
            gt = z["GT"]
            keep = gt.any(axis=1)
            rows.append(gt[keep])
            afs.append(z["AF"].reshape(-1)[keep])
            samples = z["samples"]
    return np.concatenate(rows), np.concatenate(afs).astype(np.float32), samples


def write(path, rows, af, samples, with_af, encoder="host", piece=300, **kw):
    from utmos_amd.h5write import H5Writer
    gt = np.unpackbits(rows, axis=1, count=len(samples))
    with H5Writer(str(path), samples, with_af, encoder, **kw) as w:
        for lo in range(0, max(1, len(rows)), piece):
            if lo < len(rows):
                w.add_rows(rows[lo:lo + piece], af[lo:lo + piece])
        w.finish(gt.sum(axis=0))
    return str(path)


@pytest.mark.parametrize("names, with_af, golden", [(["chunk2"], False, TINY), (["chunk0", "chunk1"], True, TINY_AF)])
@pytest.mark.parametrize("piece", [1, 300, 100_000])
def test_writer_reproduces_the_reference_files(names, with_af, golden, piece, tmp_path):
    rows, af, samples = parts(names)
    path = write(tmp_path / "out.hdf5", rows, af, samples, with_af, piece=piece)
    assert open(path, "rb").read() == open(golden, "rb").read()


def check_read_back(path, rows, af, samples, with_af):
    from utmos_amd.h5store import H5Store, pack_rows
    s = H5Store(path)
    n = len(samples)
    assert s.data.shape == (len(rows), n)
    assert s.samples.tolist() == [str(x) for x in samples]
    gt = np.unpackbits(rows, axis=1, count=n)
    assert s.var_count.tolist() == gt.sum(axis=0).tolist()
    cells = dense(s)
    if with_af:
        assert cells.dtype == np.float32
        assert cells.tobytes() == (gt.astype(np.float32) * af[:, None]).tobytes()
    else:
        assert np.array_equal(cells != 0, gt.astype(bool))
    packed, got_af = pack_rows(cells)
    assert np.array_equal(packed, rows)


@pytest.mark.parametrize("n_samples, n_rows, with_af", [
    (1, 5, False), (7, 40, True), (3000, 250, False), (3000, 77, True),   # a partial last chunk
    (40, 6250 * 12 + 11, False),                                           # 13 chunks of 6,250 rows
    (9000, 27 * 70 + 5, False),                                            # 71 chunks: a two-level `data` B-tree
    (250_007, 3, True),                                                    # one-row chunks
])
def test_written_stores_read_back(n_samples, n_rows, with_af, tmp_path):
    rng = np.random.default_rng(n_samples + n_rows)
    gt = rng.random((n_rows, n_samples)) < 0.03
    gt[:, 0] |= ~gt.any(axis=1)
    rows = np.packbits(gt, axis=1)
    af = (rng.integers(1, 1000, n_rows) / 1000).astype(np.float32)
    samples = np.array([f"HG{k:05d}" for k in range(n_samples)])
    path = write(tmp_path / "s.hdf5", rows, af, samples, with_af, piece=997)
    check_read_back(path, rows, af, samples, with_af)


def test_many_samples_give_multi_level_samples_and_var_count_trees(tmp_path):
    from utmos_amd.h5store import H5Store
    from utmos_amd.h5write import guess_chunk
    n = 300_000
    assert -(-n // guess_chunk(n, 8)) > 64
    rows = np.packbits(np.eye(2, n, dtype=bool), axis=1)
    samples = np.array([f"S{k}" for k in range(n)])
    path = write(tmp_path / "m.hdf5", rows, np.ones(2, np.float32), samples, False)
    s = H5Store(path)
    assert s.samples.tolist() == samples.tolist()
    assert s.var_count.tolist()[:3] == [1, 1, 0] and int(s.var_count.sum()) == 2


def test_guess_chunk_pins_the_fixture_lengths():
    from utmos_amd.h5write import data_chunk_rows, guess_chunk
    assert guess_chunk(2504, 7) == 1252 and guess_chunk(2504, 8) == 1252
    assert data_chunk_rows(2504) == 99 and data_chunk_rows(250_007) == 1


def test_hdf5_output_no_longer_exits_before_reading(tmp_path):
    """parse_args accepts --lowmem X.hdf5 with inputs; a missing input still exits 1 before any file exists."""
    from utmos_amd.select import parse_args, select_main
    a = parse_args(["--lowmem", str(tmp_path / "n.hdf5"), "a.npz"])
    assert a.lowmem.endswith("n.hdf5") and a.in_files == ["a.npz"]
    with pytest.raises(SystemExit) as e:
        select_main(["--lowmem", str(tmp_path / "n.hdf5"), str(tmp_path / "missing.npz")])
    assert e.value.code == 1 and not (tmp_path / "n.hdf5").exists()
