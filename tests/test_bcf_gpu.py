"""The GPU BCF reader (vcfgpu.GpuVcfReader on .bcf, csrc/bcf.hip.h) against its numpy restatement bcfio.read_bcf -- GT
bytes, AF bit for bit, sample names, het / hom-alt counts, singleton flags and stats -- on BCF encodings (tests/bcf_gen.py)
of the reference's VCF fixtures and of seeded synthetic call sets: every GT width, the bare stream, BGZF inflated on the
GPU and on the host, batches down to one byte; malformed files raise ValueError and leave the context usable."""
import os

import numpy as np
import pytest

import bcf_cases
import bcf_gen
import oracle_util as ou
import vcf_gen

VCF = os.path.join(ou.GOLD, "vcf")
pytestmark = pytest.mark.gpu


def assert_same(got, want):
    assert [str(s) for s in got["samples"]] == [str(s) for s in want["samples"]]
    assert got["GT"].dtype == np.uint8 and got["GT"].shape == want["GT"].shape
    assert (got["GT"] == want["GT"]).all()
    assert got["AF"].dtype == np.float64 and got["AF"].shape == want["AF"].shape
    assert (got["AF"].view(np.int64) == want["AF"].view(np.int64)).all()     # bit for bit
    assert got["het"].tolist() == want["het"].tolist() and got["hom"].tolist() == want["hom"].tolist()
    assert got["singleton"].tolist() == want["singleton"].tolist()
    assert got["stats"] == want["stats"]


@pytest.fixture(scope="module")
def reader():
    from utmos_amd.vcfgpu import GpuVcfReader
    with GpuVcfReader(device=0) as r:
        yield r


def write_forms(tmp_dir, name, stream, block=4000):
    """The stream bare and in BGZF with small members (records and their 8-byte prefixes cross member borders)."""
    paths = {"raw": os.path.join(tmp_dir, name + ".raw.bcf"), "bgzf": os.path.join(tmp_dir, name + ".bcf")}
    open(paths["raw"], "wb").write(stream)
    open(paths["bgzf"], "wb").write(bcf_gen.bgzf(stream, block, 1))
    return paths


def read_all_routes(paths, want, batch_bytes, reader=None):
    """raw, BGZF on the GPU, BGZF on the host: all equal `want`."""
    from utmos_amd.vcfgpu import GpuVcfReader
    own = reader is None
    r = reader or GpuVcfReader(device=0, batch_bytes=batch_bytes)
    try:
        for path in paths.values():
            assert_same(r.read(path), want)
        r.inflate = "host"
        assert_same(r.read(paths["bgzf"]), want)
    finally:
        r.inflate = "auto"
        if own:
            r.close()


@pytest.mark.parametrize("name", ["chunk0.vcf.gz", "chunk1.vcf.gz", "chunk_tiny.vcf", "build_tiny.vcf"])
def test_fixtures_equal_the_cpu_restatement(name, reader, tmp_path):
    from utmos_amd import bcfio
    from utmos_amd.vcfio import read_vcf
    stream = bcf_gen.make_bcf(bcf_gen.vcf_bytes(os.path.join(VCF, name)), raw=True, idx=name == "chunk1.vcf.gz")
    paths = write_forms(str(tmp_path), "f", stream)
    want = bcfio.read_bcf(paths["raw"])
    vcf = read_vcf(os.path.join(VCF, name))
    assert (want["GT"] == vcf["GT"]).all() and (want["AF"] == vcf["AF"]).all()
    read_all_routes(paths, want, None, reader)


@pytest.mark.parametrize("n_samp", [1, 7, 8, 9, 63, 65, 2504])
def test_synthetic_all_widths_and_routes(n_samp, tmp_path):
    """About 60 records of mixed FORMATs, ploidies, missing alleles and hundreds of alt alleles.  The small batch is the
    smallest the context accepts (1 byte) up to 9 samples, for every width; 256 bytes up to 65 samples and 4 KiB at 2,504,
    where one-byte batches would take minutes: prefixes and records straddle batches, and most records are longer than
    a batch."""
    from utmos_amd import bcfio
    data = vcf_gen.make_vcf(n_samp * 7 + 3, 60, n_samp, big_alt=True, long_info=3000, long_cells=True)
    small = 1 if n_samp <= 9 else 256 if n_samp <= 65 else 4096
    for gt_width in ("auto", "int8", "int16", "int32"):
        stream = bcf_gen.make_bcf(data, raw=True, gt_width=gt_width, idx=gt_width == "int16")
        paths = write_forms(str(tmp_path), gt_width, stream)
        want = bcfio.read_bcf(paths["raw"])
        assert want["GT"].shape == (60, (n_samp + 7) // 8)
        for batch in (64 << 20, small) if gt_width in ("auto", "int32") else (small,):
            read_all_routes(paths, want, batch)


def test_hundred_thousand_samples(tmp_path, reader):
    from utmos_amd import bcfio
    data = vcf_gen.make_vcf(5, 3, 100_000, formats=("GT", "GT:AD:DP", "DP:GT"))
    paths = write_forms(str(tmp_path), "w", bcf_gen.make_bcf(data, raw=True), block=0xFF00)
    read_all_routes(paths, bcfio.read_bcf(paths["raw"]), None, reader)


def test_record_longer_than_a_batch(tmp_path):
    from utmos_amd import bcfio
    data = vcf_gen.make_vcf(9, 6, 300, long_info=(1 << 20) + 12345, long_cells=True)
    paths = write_forms(str(tmp_path), "l", bcf_gen.make_bcf(data, raw=True), block=0xFF00)
    read_all_routes(paths, bcfio.read_bcf(paths["raw"]), 64 << 10)


def test_empty_gt_and_empty_file_of_records(tmp_path, reader):
    import struct
    from utmos_amd import bcfio
    head, recs = bcf_gen.split_stream(bcf_gen.make_bcf(bcf_cases.good_vcf(), raw=True))
    l_shared = struct.unpack_from("<I", recs[0], 0)[0]
    empty = struct.pack("<II", l_shared, 3) + recs[0][8:8 + l_shared + 2] + b"\x01"      # GT: int8 x 0
    for name, stream in (("e", head + empty + recs[1]), ("none", head)):
        paths = write_forms(str(tmp_path), name, stream, block=100)
        read_all_routes(paths, bcfio.read_bcf(paths["raw"]), None, reader)


CASES = sorted(bcf_cases.RECORD_CASES) + sorted(bcf_cases.FILE_CASES)


@pytest.mark.parametrize("case", CASES)
def test_malformed_raises_and_context_survives(case, tmp_path, reader):
    from utmos_amd import bcfio
    from utmos_amd.vcfgpu import GpuVcfReader
    good = write_forms(str(tmp_path), "good", bcf_gen.make_bcf(bcf_cases.good_vcf(), raw=True), block=300)
    want = bcfio.read_bcf(good["raw"])
    if case in bcf_cases.RECORD_CASES:
        stream, named = bcf_cases.bad_stream(case)
        bad = write_forms(str(tmp_path), "bad", stream, block=300)
        expect = [f"record {named}:", bcf_cases.RECORD_CASES[case]]
    else:
        bad = {"file": str(tmp_path / "bad.bcf")}
        open(bad["file"], "wb").write(bcf_cases.bad_file(case))
        expect = [bcf_cases.FILE_CASES[case]]
    for batch in (None, 64):     # (64-byte batches: the failure lands in a later batch with another one queued)
        r = GpuVcfReader(device=0, batch_bytes=batch) if batch else reader
        try:
            for inflate in ("auto", "host"):
                r.inflate = inflate
                for path in bad.values():
                    with pytest.raises(ValueError) as err:
                        r.read(path)
                    assert os.path.basename(path) in str(err.value)
                    for text in expect:
                        assert text in str(err.value), str(err.value)
                    handle = r.handle.value if r.handle else None
                    assert_same(r.read(good["bgzf"]), want)
                    assert handle is None or r.handle.value == handle          # the same context
        finally:
            r.inflate = "auto"
            if batch:
                r.close()


def test_neither_bcf_nor_bgzf_names_the_file(tmp_path, reader):
    p = str(tmp_path / "text.bcf")
    open(p, "wb").write(b"##fileformat=VCFv4.2\n")
    with pytest.raises(ValueError, match="text.bcf: neither a BCF stream"):
        reader.read(p)


@pytest.mark.parametrize("case", ["short-l-shared", "no-gt"])
def test_bad_record_in_any_batch_is_the_error_reported(case, tmp_path):
    """The bad record placed at every position, with batches of a few records: whichever batch it lands in -- the last,
    the one before it with the last already queued -- the error names that record and its reason, on every route."""
    from utmos_amd.vcfgpu import GpuVcfReader
    with GpuVcfReader(device=0, batch_bytes=100) as r:
        for bad in range(bcf_cases.N_REC):
            stream, named = bcf_cases.bad_stream(case, bad)
            paths = write_forms(str(tmp_path), f"b{bad}", stream, block=100)
            for inflate in ("auto", "host"):
                r.inflate = inflate
                for path in paths.values():
                    with pytest.raises(ValueError) as err:
                        r.read(path)
                    assert f"record {named}: " in str(err.value) and bcf_cases.RECORD_CASES[case] in str(err.value), str(err.value)
