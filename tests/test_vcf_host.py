"""Host side of the GPU VCF reader, without a GPU: BGZF member splitting and threaded inflate, batch cutting helpers,
the header reader, the convert command's arguments, and the het / hom-alt totals the convert tests pin."""
import gzip
import io
import os

import numpy as np
import pytest

import oracle_util as ou
import vcf_gen

VCF = os.path.join(ou.GOLD, "vcf")


class _Chunks:
    """A source that hands out at most `step` bytes per fill (batch borders anywhere)."""

    def __init__(self, data, step):
        self.fh, self.step = io.BytesIO(data), step

    def fill(self, view):
        return self.fh.readinto(view[:self.step])


def _drain(src, size):
    out, buf = bytearray(), bytearray(size)
    while True:
        k = src.fill(memoryview(buf))
        if not k:
            return bytes(out)
        out += buf[:k]


@pytest.mark.parametrize("name", ["chunk0.vcf.gz", "chunk1.vcf.gz"])
@pytest.mark.parametrize("threads,size", [(1, 1 << 20), (4, 1 << 20), (16, 100_000), (3, 777)])
def test_bgzf_threaded_inflate_equals_gzip(name, threads, size):
    from utmos_amd import vcfgpu
    path = os.path.join(VCF, name)
    raw = open(path, "rb").read()
    assert vcfgpu.is_bgzf(raw[:18])
    members = vcfgpu.bgzf_members(raw)
    assert sum(m[1] for m in members) == len(raw)
    if name == "chunk0.vcf.gz":
        assert len(members) == 158
    src = vcfgpu.open_source(path, threads)
    try:
        assert _drain(src, size) == gzip.decompress(raw)      # members smaller and larger than the buffer
    finally:
        src.close()


def test_bgzf_writer_round_trip_and_plain_gzip_is_not_bgzf(tmp_path):
    from utmos_amd import vcfgpu
    data = vcf_gen.make_vcf(3, 30, 50, crlf=True)
    b = vcfgpu.bgzf_compress(data, block=1000, threads=2)
    assert gzip.decompress(b) == data
    members = vcfgpu.bgzf_members(b)
    assert members[-1][2] == 0 and sum(m[2] for m in members) == len(data)
    assert not vcfgpu.is_bgzf(gzip.compress(data)[:18])
    with pytest.raises(ValueError):
        vcfgpu.bgzf_members(b + gzip.compress(b"x"))           # a member without the BC field
    paths = vcf_gen.write_forms(str(tmp_path), "f", data)
    for form, path in paths.items():
        src = vcfgpu.open_source(path, 2)
        try:
            assert _drain(src, 4096) == data, form
        finally:
            src.close()


def test_last_newline():
    from utmos_amd.vcfgpu import _last_newline
    a = np.zeros(300_000, np.uint8)
    assert _last_newline(a, len(a)) == -1 and _last_newline(a, 0) == -1
    a[5] = 10
    assert _last_newline(a, len(a)) == 5 and _last_newline(a, 5) == -1 and _last_newline(a, 6) == 5
    a[200_000] = 10
    assert _last_newline(a, len(a)) == 200_000 and _last_newline(a, 200_000) == 5


@pytest.mark.parametrize("step", [1, 7, 4096])
def test_header_reader(step):
    from utmos_amd.vcfgpu import GpuVcfReader
    data = b"##a\r\n\n##b\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\r\nc\t1\n"
    samples, n_head, rest = GpuVcfReader._header("x.vcf", _Chunks(data, step))
    assert samples.tolist() == ["S1", "S2"] and n_head == 4
    assert data[data.index(b"c\t1"):].startswith(rest)
    with pytest.raises(ValueError, match="x.vcf"):
        GpuVcfReader._header("x.vcf", _Chunks(b"##a\nc\t1\n#CHROM\tPOS\n", step))
    with pytest.raises(ValueError, match="no #CHROM"):
        GpuVcfReader._header("x.vcf", _Chunks(b"##a\n##b", step))


def test_convert_arguments():
    from utmos_amd.convert import parse_args
    a = parse_args(["in.vcf.gz", "out.jl"])
    assert (a.in_file, a.out_file, a.no_singleton, a.lowmem, a.buffer, a.compress, a.device) == \
        ("in.vcf.gz", "out.jl", False, False, 50000, 5, 0)
    a = parse_args(["--no-singleton", "--lowmem", "-B", "100", "-c", "9", "--device", "3", "i.vcf", "o.npz"])
    assert (a.no_singleton, a.lowmem, a.buffer, a.compress, a.device) == (True, True, 100, 9, 3)
    a = parse_args(["--buffer", "7", "--compress", "2", "i", "o"])
    assert (a.buffer, a.compress) == (7, 2)
    with pytest.raises(SystemExit):
        parse_args(["only-one"])


def test_convert_is_a_command():
    from utmos_amd.__main__ import COMMANDS, _usage
    assert "convert" in COMMANDS and "convert" in _usage()


@pytest.mark.parametrize("n,het,hom", [(0, 58258, 43479), (1, 47978, 27512)])
def test_cpu_reader_gives_the_fixture_stats(n, het, hom):
    """The het / hom-alt totals of the reference's chunkN.jl, restated cell by cell over the VCF on the CPU."""
    h = o = 0
    with gzip.open(os.path.join(VCF, f"chunk{n}.vcf.gz"), "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            for cell in line.rstrip("\n").split("\t")[9:]:
                al = [-1 if a == "." else int(a) for a in cell.split(":")[0].replace("|", "/").split("/")]
                called = len(al) > 1 and min(al) >= 0
                h += called and any(a != al[0] for a in al)
                o += called and all(a == al[0] for a in al) and al[0] > 0
    assert (h, o) == (het, hom)
