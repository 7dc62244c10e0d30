"""The DEFLATE encoder on the GPU (csrc/deflate.hip.h through utm_deflate_* and utmos_amd.zwrite): the device bytes
equal the CPU build's across levels, sizes and batch splits; GpuZlibWriter as a joblib target; `convert --deflate gpu`
against `--deflate host` on the reference's VCF fixtures, and `select` on its parts against the goldens."""
import ctypes
import io
import os
import zlib

import numpy as np
import pytest

import oracle_util as ou
import vcf_gen

pytestmark = pytest.mark.gpu
SEG = 65536
VCF = os.path.join(ou.GOLD, "vcf")
CASES = ou.golden_cases()
RNG = np.random.default_rng(5)


def host_stream(data, level):
    from utmos_amd.zwrite import deflate_host, zlib_header
    body, adler = deflate_host(data, level)
    return zlib_header(level) + body + adler.to_bytes(4, "big")


def pickle_bytes(n):
    import joblib
    buf = io.BytesIO()
    joblib.dump(joblib.load(os.path.join(ou.GOLD, "jl", f"chunk{n}.jl")), buf, compress=0)
    return buf.getvalue()


DATA = {
    "empty": b"",
    "one": b"x",
    "short": b"abcabcabcabd" * 1000,
    "seg": bytes(RNG.integers(0, 3, SEG, dtype=np.uint8)),
    "vcf": (vcf_gen.make_vcf(2, 1500, 40) * 2)[:4 * SEG + 4321],
    "random": RNG.integers(0, 256, 2 * SEG + 17, dtype=np.uint8).tobytes(),
    "zeros": bytes(3 * SEG + 77),
}


@pytest.mark.parametrize("level", [1, 2, 5, 6, 9])
@pytest.mark.parametrize("name", sorted(DATA))
def test_device_bytes_equal_the_host_build(name, level):
    from utmos_amd.zwrite import zlib_compress
    data = DATA[name]
    got = zlib_compress(data, level)
    assert got == host_stream(data, level)
    assert zlib.decompress(got) == data


@pytest.mark.parametrize("batch", [SEG, 2 * SEG, 3 * SEG])
def test_several_batches_and_a_short_final_batch(batch):
    """Batches of one to three segments (the writer pushes full batches, the last one shorter than a segment)."""
    from utmos_amd.zwrite import zlib_compress
    for n in (pickle_bytes(0), DATA["vcf"]):
        for level in (1, 5):
            got = zlib_compress(n, level, batch_bytes=batch)
            assert got == host_stream(n, level) and zlib.decompress(got) == n


def test_writes_of_every_size_through_the_writer():
    from utmos_amd.zwrite import GpuZlibWriter
    data = DATA["vcf"]
    out = io.BytesIO()
    with GpuZlibWriter(out, 5, batch_bytes=2 * SEG) as w:
        off, k = 0, 1
        while off < len(data):
            w.write(data[off:off + k])
            off += k
            k = k * 7 % 100_003 + 1
            assert w.tell() == min(off, len(data))
    assert out.getvalue() == host_stream(data, 5)


def test_large_input_round_trips():
    """A >= 100 MB generated input through 32 MiB batches; zlib reads it back."""
    from utmos_amd.zwrite import zlib_compress
    rows = np.zeros((330_000, 313), np.uint8)
    hits = RNG.integers(0, rows.size, rows.size // 40)
    rows.reshape(-1)[hits] = RNG.integers(1, 256, len(hits), dtype=np.uint8)
    data = rows.tobytes() + vcf_gen.make_vcf(9, 3000, 50)
    assert len(data) >= 100_000_000
    got = zlib_compress(data, 5)
    assert zlib.decompress(got) == data
    assert len(got) < len(data) // 2


def test_gpu_writer_as_a_joblib_target(tmp_path):
    import joblib
    from utmos_amd.zwrite import GpuZlibWriter
    want = joblib.load(os.path.join(ou.GOLD, "jl", "chunk1.jl"))
    path = str(tmp_path / "w.jl")
    with GpuZlibWriter(path, 5) as w:
        joblib.dump(want, w, compress=0)
    got = joblib.load(path)
    assert open(path, "rb").read(1) == b"\x78"
    assert set(got) == set(want)
    assert (got["GT"] == want["GT"]).all() and (got["AF"] == want["AF"]).all()
    assert list(got["samples"]) == list(want["samples"]) and got["stats"] == want["stats"]


def run(argv):
    from utmos_amd.__main__ import main
    assert main(["convert"] + argv) == 0


@pytest.mark.parametrize("n", [0, 1])
def test_convert_deflate_gpu_loads_like_host(n, tmp_path):
    import joblib
    path = os.path.join(VCF, f"chunk{n}.vcf.gz")
    h, g = str(tmp_path / "h.jl"), str(tmp_path / "g.jl")
    run([path, h, "--deflate", "host"])
    run([path, g, "--deflate", "gpu"])
    assert open(g, "rb").read(1) == b"\x78"
    a, b = joblib.load(h), joblib.load(g)
    assert set(a) == set(b) == {"samples", "GT", "AF", "stats"}
    assert a["GT"].dtype == b["GT"].dtype and (a["GT"] == b["GT"]).all()
    assert a["AF"].dtype == b["AF"].dtype and (a["AF"] == b["AF"]).all()
    assert [str(s) for s in a["samples"]] == [str(s) for s in b["samples"]]
    assert a["stats"] == b["stats"]
    h0, g0 = str(tmp_path / "h0.jl"), str(tmp_path / "g0.jl")
    run([path, h0, "-c", "0", "--deflate", "host"])
    run([path, g0, "-c", "0", "--deflate", "gpu"])
    assert open(h0, "rb").read() == open(g0, "rb").read()


def test_select_on_gpu_written_parts(tmp_path):
    from utmos_amd.select import select_main
    parts = {}
    for n in (0, 1):
        parts[n] = str(tmp_path / f"chunk{n}.jl")
        run([os.path.join(VCF, f"chunk{n}.vcf.gz"), parts[n], "--deflate", "gpu", "-c", "9"])
    out = str(tmp_path / "o.tsv")
    select_main(["-o", out, parts[1]])
    assert open(out).read() == ou.golden_text(CASES["select_fileout"])
    select_main(["-o", out, parts[0], os.path.join(ou.GOLD, "chunk2.npz")])
    assert open(out).read() == ou.golden_text(CASES["select_multi"])


def test_errors_and_context_reuse():
    from utmos_amd import _native as nat
    from utmos_amd.zwrite import GpuZlibWriter
    lib = nat.lib()
    h = ctypes.c_void_p()
    assert lib.utm_deflate_create(0, 4 * SEG, 10, ctypes.byref(h)) == -1 and b"level" in lib.utm_last_error()
    with pytest.raises(ValueError):
        GpuZlibWriter(io.BytesIO(), 0)
    nat.check(lib.utm_deflate_create(0, 4 * SEG, 5, ctypes.byref(h)))
    try:
        data = DATA["vcf"][:3 * SEG + 10]
        ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
        assert lib.utm_deflate_pull(h, ctypes.byref(ptr), ctypes.byref(n)) == -4          # nothing pushed
        assert lib.utm_deflate_push(h, data, SEG + 1, 0) == -1                            # not whole segments
        assert b"multiple" in lib.utm_last_error()
        assert lib.utm_deflate_push(h, data, 5 * SEG, 1) == -1                            # above the batch
        assert lib.utm_deflate_push(h, data, 10, 4) == -1                                 # unknown flag
        body = b""
        for off, k, flags in ((0, 2 * SEG, 0), (2 * SEG, SEG, 0), (3 * SEG, 10, 1)):
            nat.check(lib.utm_deflate_push(h, data[off:off + k], k, flags))
            nat.check(lib.utm_deflate_pull(h, ctypes.byref(ptr), ctypes.byref(n)))
            body += ctypes.string_at(ptr.value, n.value)
        adler = ctypes.c_uint32()
        nat.check(lib.utm_deflate_adler(h, ctypes.byref(adler)))
        assert adler.value == zlib.adler32(data)
        from utmos_amd.zwrite import deflate_host
        assert body == deflate_host(data, 5)[0]
        # a second stream on the same context starts afresh
        nat.check(lib.utm_deflate_push(h, b"hello", 5, 1))
        nat.check(lib.utm_deflate_pull(h, ctypes.byref(ptr), ctypes.byref(n)))
        assert zlib.decompress(ctypes.string_at(ptr.value, n.value), -15) == b"hello"
        nat.check(lib.utm_deflate_adler(h, ctypes.byref(adler)))
        assert adler.value == zlib.adler32(b"hello")
        ms = (ctypes.c_double * 4)()
        nat.check(lib.utm_deflate_timing(h, ms))
        assert ms[1] > 0 and 0 <= ms[3] <= ms[1]
    finally:
        lib.utm_deflate_destroy(h)
