"""BGZF inflated on the GPU (csrc/inflate.hip.h, GpuVcfReader(inflate="gpu")) against host inflation and the CPU reader
vcfio.read_vcf: GT, AF, samples, stats and singleton flags on the reference's fixtures and on seeded call sets written
by BGZF writers of every level and strategy, with records across members and batches, long records, wide rows, headers
over several members or ending at a member border, no end-of-file member and no final newline.  Corrupted members fail
with ValueError naming the member's byte offset and leave the reader usable.  `convert --inflate gpu` reproduces the
reference's .jl files, and the ABI keeps the carry between batches on the device."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import oracle_util as ou
import vcf_gen

VCF = os.path.join(ou.GOLD, "vcf")
pytestmark = pytest.mark.gpu


def assert_same(got, want, full=True):
    assert [str(s) for s in got["samples"]] == [str(s) for s in want["samples"]]
    assert got["GT"].dtype == np.uint8 and got["GT"].shape == want["GT"].shape
    assert (got["GT"] == want["GT"]).all()
    assert got["AF"].dtype == np.float64 and got["AF"].shape == want["AF"].shape
    assert (got["AF"].view(np.int64) == want["AF"].view(np.int64)).all()
    if full:
        assert got["stats"] == want["stats"]
        assert (got["singleton"] == want["singleton"]).all()


def bgzf(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, block=0xFF00, eof=True, borders=()):
    """A BGZF writer with a zlib strategy; `borders`: text offsets where a member must end."""
    cuts = sorted(set(list(range(0, len(data), block)) + [b for b in borders if 0 < b < len(data)] + [len(data)]))
    out = []
    for lo, hi in list(zip(cuts, cuts[1:])) or [(0, 0)]:       # (no text: one empty member)
        piece = data[lo:hi]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        body = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + (len(body) + 25).to_bytes(2, "little")
                   + body + zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))
    if eof:
        out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)


def read_all(path, batch=64 << 20, full=True):
    """gpu == host == vcfio.read_vcf -> the GPU-inflated result and its timing."""
    from utmos_amd.vcfgpu import GpuVcfReader
    from utmos_amd.vcfio import read_vcf
    with GpuVcfReader(device=0, batch_bytes=batch, inflate="gpu") as g, \
            GpuVcfReader(device=0, batch_bytes=batch, inflate="host") as h:
        got = g.read(path)
        timing = dict(g.timing)
        want = h.read(path)
    assert_same(got, want)
    assert_same(got, read_vcf(path), full=False)
    return got, timing


@pytest.fixture(scope="module")
def reader():
    from utmos_amd.vcfgpu import GpuVcfReader
    with GpuVcfReader(device=0, inflate="gpu") as r:
        yield r


@pytest.mark.parametrize("name", ["chunk0.vcf.gz", "chunk1.vcf.gz"])
def test_fixtures(name):
    got, timing = read_all(os.path.join(VCF, name))
    assert timing["inflate_ms"] > 0 and set(timing) == {"fill_s", "h2d_ms", "kernel_ms", "d2h_ms", "inflate_ms", "total_s"}


@pytest.mark.parametrize("writer", ["L0", "L1", "L6", "L9", "Z_FIXED", "Z_RLE", "Z_HUFFMAN_ONLY"])
def test_writers(writer, tmp_path):
    from utmos_amd.vcfgpu import bgzf_compress
    data = vcf_gen.make_vcf(21, 300, 90, big_alt=True, meta_among=True)
    path = str(tmp_path / "w.vcf.gz")
    if writer.startswith("L"):
        blob = bgzf_compress(data, level=int(writer[1:]), block=5000)
    else:
        blob = bgzf(data, strategy=getattr(zlib, writer), block=7000)
    open(path, "wb").write(blob)
    for batch in (64 << 20, 4096, 70_000):     # small batches: records across members and batches
        read_all(path, batch)


def test_record_longer_than_a_batch(tmp_path):
    data = vcf_gen.make_vcf(9, 6, 300, long_info=(1 << 20) + 12345, long_cells=True)
    path = str(tmp_path / "l.vcf.gz")
    open(path, "wb").write(bgzf(data, level=1))
    for batch in (64 << 10, 1 << 20):
        read_all(path, batch)


def test_hundred_thousand_samples(tmp_path):
    data = vcf_gen.make_vcf(5, 3, 100_000, formats=("GT", "GT:AD:DP", "DP:GT"))
    path = str(tmp_path / "w.vcf.gz")
    open(path, "wb").write(bgzf(data, level=6))
    read_all(path, 1 << 20)


@pytest.mark.parametrize("shape", ["header-over-members", "header-at-border", "no-eof", "no-final-newline", "crlf",
                                   "header-only", "empty-members"])
def test_shapes(shape, tmp_path):
    data = vcf_gen.make_vcf(33, 80, 3000 if shape == "header-over-members" else 50,
                            crlf=shape == "crlf", final_newline=shape not in ("no-final-newline", "crlf"))
    head_end = data.index(b"#CHROM")
    head_end = data.index(b"\n", head_end) + 1
    if shape == "header-only":
        data = data[:head_end]
    borders = [head_end] if shape == "header-at-border" else []
    if shape == "empty-members":
        blob = bgzf(data[:head_end], block=1000)[:-28] + bgzf(b"", eof=False) * 3 + bgzf(data[head_end:], block=3000)
    else:
        blob = bgzf(data, level=6, block=1000 if "header" in shape else 5000, eof=shape != "no-eof", borders=borders)
    path = str(tmp_path / "s.vcf.gz")
    open(path, "wb").write(blob)
    for batch in (64 << 20, 2000):
        got, _ = read_all(path, batch)
        assert got["GT"].shape[0] == (0 if shape == "header-only" else 80)


def _members(blob):
    from utmos_amd.vcfgpu import bgzf_members
    return bgzf_members(blob)


@pytest.mark.parametrize("case", ["flip", "crc", "isize-down", "isize-up", "truncate-body"])
def test_corrupt_member_names_its_offset(case, tmp_path, reader):
    from utmos_amd.vcfio import read_vcf
    data = vcf_gen.make_vcf(41, 200, 40)
    blob = bytearray(bgzf(data, level=6, block=3000))
    members = _members(bytes(blob))
    off, size, isize = members[len(members) // 2]       # a member after the header's
    if case == "flip":
        blob[off + 18 + 5] ^= 0x40
    elif case == "crc":
        blob[off + size - 8] ^= 1
    elif case in ("isize-down", "isize-up"):
        blob[off + size - 4:off + size] = (isize + (-1 if case == "isize-down" else 1)).to_bytes(4, "little")
    else:                                              # the member keeps its BSIZE but its deflate data ends early
        body = blob[off + 18:off + size - 8]
        blob[off + 18:off + size - 8] = body[:len(body) // 2] + bytes(len(body) - len(body) // 2)
    bad = str(tmp_path / "bad.vcf.gz")
    open(bad, "wb").write(bytes(blob))
    handle = reader.handle.value if reader.handle is not None else None
    for batch in (None, 4000):
        from utmos_amd.vcfgpu import GpuVcfReader
        r = reader if batch is None else GpuVcfReader(device=0, batch_bytes=batch, inflate="gpu")
        with pytest.raises(ValueError, match=f"bad.vcf.gz: BGZF member at byte {off}: ") as info:
            r.read(bad)
        if case.startswith("isize"):
            assert "ISIZE says" in str(info.value)
        good = str(tmp_path / "good.vcf.gz")
        open(good, "wb").write(bgzf(data, level=1, block=2500))
        assert_same(r.read(good), read_vcf(good), full=False)
        if batch is None:
            assert handle is None or reader.handle.value == handle
        else:
            r.close()


def test_gpu_refuses_plain_gzip_and_auto_reads_it(tmp_path):
    import gzip
    from utmos_amd.vcfgpu import GpuVcfReader
    from utmos_amd.vcfio import read_vcf
    data = vcf_gen.make_vcf(2, 30, 20)
    path = str(tmp_path / "g.vcf.gz")
    open(path, "wb").write(gzip.compress(data))
    with pytest.raises(ValueError, match="BGZF"):
        GpuVcfReader(device=0, inflate="gpu").read(path)
    with GpuVcfReader(device=0) as r:
        assert_same(r.read(path), read_vcf(path), full=False)
        assert r.timing["inflate_ms"] == 0


@pytest.mark.parametrize("n", [0, 1])
def test_convert_inflate_gpu_matches_the_references_conversion(n, tmp_path):
    import joblib
    from utmos_amd.__main__ import main
    got = {}
    for mode in ("gpu", "host"):
        out = str(tmp_path / f"chunk{n}.{mode}.jl")
        assert main(["convert", os.path.join(VCF, f"chunk{n}.vcf.gz"), out, "--inflate", mode]) == 0
        got[mode] = joblib.load(out)
    want = joblib.load(os.path.join(ou.GOLD, "jl", f"chunk{n}.jl"))
    for g in got.values():
        assert (g["GT"] == want["GT"]).all() and g["GT"].shape == want["GT"].shape
        assert [str(s) for s in g["samples"]] == [str(s) for s in want["samples"]]
        assert (int(g["stats"]["num_het"]), int(g["stats"]["num_hom"])) == \
            (int(want["stats"]["num_het"]), int(want["stats"]["num_hom"]))
        assert g["AF"].shape == want["AF"].shape
    assert (got["gpu"]["AF"].view(np.int64) == got["host"]["AF"].view(np.int64)).all()


def test_abi_carry_with_prefix_and_a_batch_without_newline():
    from utmos_amd import _native as nat
    lib = nat.lib()
    calls = [(b"0|1", b"1|1"), (b"0|0", b"1|0"), (b"1|1", b"1|1"), (b"0|1", b"0|0")]
    rec = [b"c\t%d\t.\tA\tC\t.\t.\t.\tGT\t%s\t%s\n" % (i, x, y) for i, (x, y) in enumerate(calls)]
    text = b"".join(rec)
    # prefix: record 0 and 5 bytes of record 1; batch 1 ends 7 bytes into record 2 (carry 7); batch 2 adds 5 bytes
    # and no newline (all 12 bytes carry, no record); batch 3 (last) ends record 3 without its newline
    a = len(rec[0]) + 5
    b = len(rec[0]) + len(rec[1]) + 7
    c = b + 5
    prefix, pieces = text[:a], [text[a:b], text[b:c], text[c:-1]]
    h = ctypes.c_void_p()
    nat.check(lib.utm_vcf_create(0, 2, 1 << 16, ctypes.byref(h)))

    def fetch(n):
        r, fl = np.empty((max(n, 1), 1), np.uint8), np.empty(max(n, 1), np.uint8)
        af, het, hom = np.empty(max(n, 1)), np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32)
        nat.check(lib.utm_vcf_fetch(h, r.ctypes.data, af.ctypes.data, het.ctypes.data, hom.ctypes.data, fl.ctypes.data))
        return r[:n, 0].tolist()

    try:
        assert lib.utm_vcf_fetch(h, None, None, None, None, None) == -4                   # nothing queued
        got, counts = [], []
        for k, piece in enumerate(pieces):
            members = [bgzf(piece[i:i + 9], eof=False) for i in range(0, len(piece), 9)]
            packed = b"".join(members)
            table = np.array([[len(m), int.from_bytes(m[-4:], "little")] for m in members], np.uint32)
            flags = (1 if k == 0 else 0) | (2 if k == len(pieces) - 1 else 0)
            n_rec, carry = ctypes.c_uint64(), ctypes.c_uint64()
            pre = prefix if k == 0 else None
            nat.check(lib.utm_vcf_parse_bgzf(h, pre, len(pre) if pre else 0, packed, len(packed), table.ctypes.data,
                                             len(members), flags, ctypes.byref(n_rec), ctypes.byref(carry)))
            counts.append((n_rec.value, carry.value))
            if k == 1:                       # two batches queued: a third is refused, then collect the first
                assert lib.utm_vcf_parse(h, text, len(text), ctypes.byref(n_rec)) == -4
                assert b"both slots" in lib.utm_last_error()
                got += fetch(counts[0][0])
        got += fetch(counts[1][0]) + fetch(counts[2][0])
        assert counts == [(2, 7), (0, 12), (2, 0)]
        assert got == [0b11000000, 0b01000000, 0b11000000, 0b10000000]      # het or hom-alt, MSB = first sample
        # a fresh file on the same context: FIRST drops nothing stale, the plain path still works after it
        n_rec, carry = ctypes.c_uint64(), ctypes.c_uint64()
        m = bgzf(text, eof=False)
        t = np.array([[len(m), len(text)]], np.uint32)
        nat.check(lib.utm_vcf_parse_bgzf(h, None, 0, m, len(m), t.ctypes.data, 1, 3, ctypes.byref(n_rec), ctypes.byref(carry)))
        assert (n_rec.value, carry.value) == (4, 0) and fetch(4) == [192, 64, 192, 128]
    finally:
        lib.utm_vcf_destroy(h)
