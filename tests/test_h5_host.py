"""The reference's `--lowmem` HDF5 store without a GPU: the structure reader (utmos_amd/h5store.py) on the reference's
own two stores and on generated ones, the CPU build of the device's LZF decoder (utm_lzf_decode_host) against a plain
Python decoder, corrupted chunks, and select's argument rules for .hdf5 inputs."""
import ctypes
import os

import numpy as np
import pytest

import h5_gen
import oracle_util as ou

H5 = os.path.join(ou.GOLD, "h5")
TINY, TINY_AF = os.path.join(H5, "tiny.hdf5"), os.path.join(H5, "tiny.af.hdf5")


def py_lzf(stored, n_out):
    """liblzf's decoder, byte by byte; None for a malformed stream."""
    out = bytearray()
    i = 0
    while i < len(stored):
        c = stored[i]
        i += 1
        if c < 32:
            if i + c + 1 > len(stored):
                return None
            out += stored[i:i + c + 1]
            i += c + 1
        else:
            length = c >> 5
            if length == 7:
                if i >= len(stored):
                    return None
                length += stored[i]
                i += 1
            if i >= len(stored):
                return None
            ref = len(out) - ((c & 31) << 8) - stored[i] - 1
            i += 1
            if ref < 0:
                return None
            for k in range(length + 2):
                out.append(out[ref + k])
        if len(out) > n_out:
            return None
    return bytes(out) if len(out) == n_out else None


def host_decode(stored, n_out):
    from utmos_amd import _native as nat
    src = np.frombuffer(bytes(stored), np.uint8)
    out = np.zeros(n_out, np.uint8)
    status = ctypes.c_uint32(99)
    nat.check(nat.lib().utm_lzf_decode_host(src.ctypes.data if len(src) else None, len(src),
                                            out.ctypes.data if n_out else None, n_out, ctypes.byref(status)))
    return status.value, out.tobytes()


def stored_chunks(store):
    ds = store.data
    with open(store.path, "rb") as fh:
        for row, offset, size, mask in ds.chunks:
            fh.seek(offset)
            yield row, fh.read(size), mask


def dense(store):
    """The whole `data` dataset through the host decoder."""
    ds = store.data
    out = np.zeros(ds.shape, ds.dtype)
    for row, blob, mask in stored_chunks(store):
        raw = blob if mask & 1 else host_decode(blob, ds.chunk_bytes)[1]
        cells = np.frombuffer(raw, ds.dtype).reshape(ds.chunk_shape)
        out[row:row + ds.chunk_rows] = cells[:min(ds.chunk_rows, ds.shape[0] - row)]
    return out


# ---------------------------------------------------------------------------------------------- the reference's stores
def test_reader_on_the_reference_stores():
    from utmos_amd.h5store import H5Store
    s = H5Store(TINY)
    assert s.data.shape == (995, 2504) and s.data.kind == "bool" and s.data.itemsize == 1
    assert s.data.chunk_shape == (99, 2504) and s.data.filtered
    assert [c[0] for c in s.data.chunks] == list(range(0, 995, 99))
    assert all(c[3] == 0 for c in s.data.chunks)
    assert s.samples[0] == "HG00096" and len(s.samples) == 2504
    cells = dense(s)
    assert (cells.astype(bool).sum(axis=0) == s.var_count).all()
    af = H5Store(TINY_AF)
    assert af.data.shape == (1989, 2504) and af.data.kind == "float" and len(af.data.chunks) == 21
    assert list(af.samples) == list(s.samples)
    cells = dense(af)
    assert (cells != 0).any(axis=1).all()                            # no all-zero rows in this one
    assert (af.var_count >= (cells != 0).sum(axis=0)).all()          # var_count is from GT, not from the cells


def test_reference_store_packs_to_the_informative_rows_of_chunk2():
    from utmos_amd.h5store import H5Store, pack_rows
    packed, af = pack_rows(dense(H5Store(TINY)))
    part = ou.load_part("chunk2")
    gt = np.asarray(part["GT"], np.uint8)
    assert af is None and np.array_equal(packed, gt[gt.any(axis=1)])


def test_host_decoder_equals_python_on_every_fixture_chunk():
    from utmos_amd.h5store import H5Store
    for path in (TINY, TINY_AF):
        s = H5Store(path)
        for row, blob, mask in stored_chunks(s):
            status, got = host_decode(blob, s.data.chunk_bytes)
            assert status == 0 and got == py_lzf(blob, s.data.chunk_bytes), (path, row)


# ---------------------------------------------------------------------------------------------- LZF streams
def literal(data):
    assert 1 <= len(data) <= 32
    return bytes([len(data) - 1]) + bytes(data)


def match(length, offset):
    assert 3 <= length <= 264 and 1 <= offset <= 8192
    off = offset - 1
    if length < 9:
        return bytes([(length - 2) << 5 | off >> 8, off & 255])
    return bytes([7 << 5 | off >> 8, length - 9, off & 255])


def handmade_streams():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    lits = b"".join(literal(noise[k:k + 32]) for k in range(0, 8192, 32))          # 8 KiB of 32-byte literals
    yield "32-byte literals", lits, 8192
    yield "offset 1 runs", literal(b"x") + match(264, 1) + match(3, 1), 268
    yield "offset 8192", lits + match(264, 8192) + match(264, 8192) + match(9, 8192), 8192 + 537
    yield "overlap", literal(b"abcde") + match(264, 5) + match(200, 3) + match(10, 7), 479
    yield "every length", literal(b"q") + b"".join(match(n, 1) for n in range(3, 265)), 1 + sum(range(3, 265))
    yield "one byte", literal(b"z"), 1
    yield "empty", b"", 0


@pytest.mark.parametrize("name,stream,n_out", list(handmade_streams()), ids=[s[0] for s in handmade_streams()])
def test_host_decoder_on_handmade_streams(name, stream, n_out):
    expect = py_lzf(stream, n_out)
    assert expect is not None
    assert host_decode(stream, n_out) == (0, expect)


def test_generated_compressor_round_trips():
    rng = np.random.default_rng(11)
    for data in (b"", b"a", b"ab" * 5000, rng.integers(0, 3, 70000, dtype=np.uint8).tobytes(),
                 (rng.random(20000) < 0.02).astype(np.float32).tobytes()):
        stored = h5_gen.lzf_compress(data)
        assert host_decode(stored, len(data)) == (0, data)
        assert py_lzf(stored, len(data)) == data


def test_malformed_streams_give_a_status_code():
    assert host_decode(literal(b"abc")[:-1], 3)[0] == 1                  # literal past the input
    assert host_decode(bytes([7 << 5]), 300)[0] == 1                     # length byte missing
    assert host_decode(bytes([1 << 5]), 300)[0] == 1                     # offset byte missing
    assert host_decode(literal(b"abcd"), 3)[0] == 2                      # more output than the chunk
    assert host_decode(literal(b"ab") + match(20, 2), 10)[0] == 2
    assert host_decode(literal(b"ab"), 3)[0] == 3                        # less
    assert host_decode(literal(b"ab") + match(3, 3), 5)[0] == 4          # before the chunk start
    assert host_decode(match(3, 1), 3)[0] == 4


def test_seeded_corruption_never_crashes():
    from utmos_amd.h5store import H5Store
    s = H5Store(TINY)
    rng = np.random.default_rng(2024)
    blobs = [blob for _row, blob, _mask in stored_chunks(s)]
    bad = 0
    for trial in range(300):
        blob = bytearray(blobs[trial % len(blobs)])
        for _ in range(1 + trial % 4):
            blob[rng.integers(len(blob))] = rng.integers(256)
        if trial % 7 == 0:
            blob = blob[:rng.integers(1, len(blob))]
        status, got = host_decode(blob, s.data.chunk_bytes)
        expect = py_lzf(bytes(blob), s.data.chunk_bytes)
        assert (status == 0) == (expect is not None)
        if status == 0:
            assert got == expect
        bad += status != 0
    assert bad > 0


# ---------------------------------------------------------------------------------------------- generated stores
def test_generated_store_covers_raw_missing_multilevel_and_partial(tmp_path):
    from utmos_amd.h5store import H5Store
    rng = np.random.default_rng(3)
    data = rng.random((1003, 40)) < 0.1
    path = h5_gen.write_store(str(tmp_path / "g.hdf5"), data, chunk_rows=7, raw={0, 5, 143}, missing={9, 70},
                              split_headers=True)
    s = H5Store(path)
    assert s.data.shape == (1003, 40) and s.data.chunk_shape == (7, 40)
    assert len(s.data.chunks) == 144 - 2                              # 144 chunks, a three-node leaf level
    assert {c[0] // 7 for c in s.data.chunks if c[3] & 1} == {0, 5, 143}
    expect = data.copy()
    expect[63:70] = False
    expect[490:497] = False
    assert np.array_equal(dense(s).astype(bool), expect)
    assert (s.var_count == data.sum(axis=0)).all()


def test_generated_one_row_chunks_and_float_rows(tmp_path):
    from utmos_amd.h5store import H5Store, pack_rows
    rng = np.random.default_rng(4)
    cells = h5_gen.af_matrix(rng, 5, 250_001, density=0.001, zero_rows=2)
    path = h5_gen.write_store(str(tmp_path / "wide.hdf5"), cells)
    s = H5Store(path)
    assert s.data.chunk_shape == (1, 250_001) and len(s.data.chunks) == 5
    got = dense(s)
    assert np.array_equal(got, cells)
    packed, af = pack_rows(got)
    assert np.array_equal(packed, np.packbits(cells != 0, axis=1))
    assert (af[~(cells != 0).any(axis=1)] == 0).all()
    mixed = cells[(cells != 0).any(axis=1)][:1].copy()
    mixed[0, np.flatnonzero(mixed[0])[0]] *= 2
    with pytest.raises(ValueError):
        pack_rows(mixed)


@pytest.mark.parametrize("what,patch,message", [
    ("superblock", (8, 2), "superblock version 2"),
    ("signature", (0, 0), "not an HDF5 file"),
])
def test_unsupported_files_are_named(tmp_path, what, patch, message):
    from utmos_amd.h5store import H5Store
    blob = bytearray(open(TINY, "rb").read())
    blob[patch[0]] = patch[1]
    path = tmp_path / "x.hdf5"
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match=message):
        H5Store(str(path))


def test_other_filters_and_dtypes_are_refused(tmp_path):
    from utmos_amd.h5store import H5Store
    rng = np.random.default_rng(1)
    path = h5_gen.write_store(str(tmp_path / "g.hdf5"), rng.random((30, 9)) < 0.5, chunk_rows=4)
    blob = bytearray(open(path, "rb").read())
    at = blob.index(b"lzf\0") - 8                                     # the filter's id
    blob[at:at + 2] = (1).to_bytes(2, "little")                       # deflate
    (tmp_path / "gz.hdf5").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="filter 1"):
        H5Store(str(tmp_path / "gz.hdf5"))
    path = h5_gen.write_store(str(tmp_path / "f64.hdf5"), rng.random((30, 9)).astype(np.float64), chunk_rows=4)
    with pytest.raises(ValueError, match="float"):
        H5Store(path)


# ---------------------------------------------------------------------------------------------- select's argument rules
def test_hdf5_arguments_follow_the_reference():
    from utmos_amd.select import parse_args
    a = parse_args(["x.hdf5"])
    assert a.lowmem == 1 and a.in_files == ["x.hdf5"]
    a = parse_args(["--lowmem", "y.hdf5"])
    assert a.lowmem == 1 and a.in_files == ["y.hdf5"]


@pytest.mark.parametrize("argv", [["x.hdf5", "a.npz"], ["--lowmem", "new.hdf5", "a.npz"], ["old.hdf5"]])
def test_hdf5_argument_errors_exit_1(argv):
    from utmos_amd.select import select_main
    with pytest.raises(SystemExit) as e:
        select_main(argv)
    assert e.value.code == 1
