"""The DEFLATE encoder of csrc/deflate.hip.h built for the CPU (utm_deflate_host), against zlib: every level on edge
sizes, runs, far periods, incompressible bytes, VCF text and the raw pickles of the reference's .jl parts; the Adler-32,
determinism, the ratio against zlib, argument errors and the `convert --deflate` option.  Needs no GPU."""
import ctypes
import io
import mmap
import os
import zlib

import numpy as np
import pytest

import oracle_util as ou
import vcf_gen

SEG = 65536
LEVELS = range(1, 10)


def raw_pickle(n):
    import joblib
    buf = io.BytesIO()
    joblib.dump(joblib.load(os.path.join(ou.GOLD, "jl", f"chunk{n}.jl")), buf, compress=0)
    return buf.getvalue()


def encode(data, level):
    from utmos_amd.zwrite import deflate_host
    return deflate_host(data, level)


def as_zlib(body, adler, level=5):
    from utmos_amd.zwrite import zlib_header
    return zlib_header(level) + body + adler.to_bytes(4, "big")


RNG = np.random.default_rng(11)
PERIOD = RNG.integers(0, 256, 40000, dtype=np.uint8).tobytes()
TEXTS = {
    "empty": b"",
    "one": b"x",
    "seg-1": bytes(RNG.integers(0, 4, SEG - 1, dtype=np.uint8)),
    "seg": bytes(RNG.integers(0, 4, SEG, dtype=np.uint8)),
    "seg+1": bytes(RNG.integers(0, 4, SEG + 1, dtype=np.uint8)),
    "segments": (vcf_gen.make_vcf(5, 1500, 40) * 3)[:5 * SEG + 123],
    "zeros": bytes(3 * SEG + 77),
    "far-period": PERIOD * 4,
    "vcf": vcf_gen.make_vcf(3, 400, 60),
}


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_round_trip_and_adler(name, level):
    data = TEXTS[name]
    body, adler = encode(data, level)
    assert zlib.decompress(body, -15) == data
    assert adler == zlib.adler32(data)
    assert zlib.decompress(as_zlib(body, adler, level)) == data


@pytest.mark.parametrize("level", LEVELS)
def test_incompressible_bytes_take_stored_blocks(level):
    data = RNG.integers(0, 256, 3 * SEG + 5000, dtype=np.uint8).tobytes()
    body, adler = encode(data, level)
    assert zlib.decompress(body, -15) == data and adler == zlib.adler32(data)
    n_seg = -(-len(data) // SEG)
    assert len(body) <= len(data) + 15 * n_seg
    bound = ctypes.c_uint64()
    from utmos_amd import _native as nat
    nat.check(nat.lib().utm_deflate_bound(len(data), ctypes.byref(bound)))
    assert len(body) <= bound.value == len(data) + 15 * n_seg


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("level", LEVELS)
def test_raw_pickles_of_the_reference_parts(n, level):
    data = raw_pickle(n)
    body, adler = encode(data, level)
    assert zlib.decompress(as_zlib(body, adler, level)) == data


@pytest.mark.parametrize("n", [0, 1])
def test_level5_ratio_against_zlib(n):
    data = raw_pickle(n)
    body, _ = encode(data, 5)
    assert len(body) + 6 <= 1.15 * len(zlib.compress(data, 5))


def test_segment_borders_and_sync_flush():
    """Every segment but the last ends with an empty stored block; the last sets BFINAL: inflating all but the final
    segment's bytes with a streaming inflater yields whole segments of text."""
    data = TEXTS["segments"]
    body, _ = encode(data, 5)
    assert body.count(b"\x00\x00\xff\xff") >= len(data) // SEG
    d = zlib.decompressobj(-15)
    cut = body.rfind(b"\x00\x00\xff\xff") + 4
    assert d.decompress(body[:cut]) == data[:len(data) // SEG * SEG]
    assert d.decompress(body[cut:]) == data[len(data) // SEG * SEG:] and d.eof


def test_deterministic():
    data = TEXTS["segments"]
    for level in (1, 5, 9):
        assert encode(data, level) == encode(data, level)


def test_argument_errors():
    from utmos_amd import _native as nat
    lib = nat.lib()
    out = ctypes.create_string_buffer(100)
    n, adler = ctypes.c_uint64(), ctypes.c_uint32()
    for level in (0, 10, -1):
        assert lib.utm_deflate_host(b"abc", 3, level, out, 100, ctypes.byref(n), ctypes.byref(adler)) == -1
        assert b"level" in lib.utm_last_error()
    assert lib.utm_deflate_host(None, 3, 5, out, 100, ctypes.byref(n), ctypes.byref(adler)) == -1
    assert lib.utm_deflate_host(b"abc", 3, 5, None, 100, ctypes.byref(n), ctypes.byref(adler)) == -1
    assert lib.utm_deflate_host(b"abc", 3, 5, out, 100, None, ctypes.byref(adler)) == -1
    assert lib.utm_deflate_host(b"abc", 3, 5, out, 100, ctypes.byref(n), None) == -1
    assert b"NULL" in lib.utm_last_error()
    assert lib.utm_deflate_host(b"abc", 3, 5, out, 3, ctypes.byref(n), ctypes.byref(adler)) == -1
    assert b"too small" in lib.utm_last_error()
    assert lib.utm_deflate_bound(10, None) == -1
    h = ctypes.c_void_p()
    assert lib.utm_deflate_create(0, 1 << 20, 0, ctypes.byref(h)) == -1 and not h.value
    assert lib.utm_deflate_push(None, None, 0, 1) == -1
    assert lib.utm_deflate_destroy(None) == 0


def test_small_out_cap_stops_at_the_buffer_end():
    """The output ends right at a page the process may not write: any write past out_cap faults the test."""
    libc = ctypes.CDLL(None)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = mmap.PAGESIZE
    size = 40 * page
    buf = mmap.mmap(-1, size + page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(buf))
    assert libc.mprotect(base + size, page, 0) == 0
    try:
        from utmos_amd import _native as nat
        lib = nat.lib()
        n, adler = ctypes.c_uint64(), ctypes.c_uint32()
        for data in (TEXTS["segments"], RNG.integers(0, 256, 2 * SEG + 9, dtype=np.uint8).tobytes()):
            want, _ = encode(data, 5)
            for cap in sorted({0, 1, 5, len(want) // 3, len(want) - 1, min(len(want), size)}):
                at = size - cap
                rc = lib.utm_deflate_host(data, len(data), 5, ctypes.c_void_p(base + at), cap, ctypes.byref(n),
                                          ctypes.byref(adler))
                if cap >= len(want):
                    assert rc == 0 and buf[at:at + n.value] == want
                else:
                    assert rc == -1 and b"too small" in lib.utm_last_error()
    finally:
        libc.mprotect(base + size, page, 3)
        buf.close()


def test_zlib_header_bytes():
    from utmos_amd.zwrite import zlib_header
    for level in LEVELS:
        h = zlib_header(level)
        assert h == zlib.compress(b"", level)[:2]
        assert (h[0] << 8 | h[1]) % 31 == 0


def test_convert_deflate_option():
    from utmos_amd.convert import parse_args
    assert parse_args(["a.vcf", "b.jl"]).deflate == "host"
    assert parse_args(["a.vcf", "b.jl", "--deflate", "gpu"]).deflate == "gpu"
    assert parse_args(["a.vcf", "b.jl", "--deflate", "host"]).deflate == "host"
    with pytest.raises(SystemExit):
        parse_args(["a.vcf", "b.jl", "--deflate", "cpu"])


def test_convert_write_host_path_is_unchanged(tmp_path):
    """convert.write with the default deflate="host" writes exactly what joblib.dump writes; a bad deflate is refused."""
    import joblib
    from utmos_amd import convert
    data = joblib.load(os.path.join(ou.GOLD, "jl", "chunk0.jl"))
    for c in (0, 3):
        a, b = str(tmp_path / f"a{c}.jl"), str(tmp_path / f"b{c}.jl")
        convert.write(data, a, c)
        joblib.dump(dict(data, samples=np.asarray(data["samples"]).astype(object)), b, compress=c)
        assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(ValueError):
        convert.write(data, str(tmp_path / "x.jl"), 5, deflate="cpu")
