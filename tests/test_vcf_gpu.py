"""The GPU VCF reader (utmos_amd/vcfgpu.py, csrc/vcf.hip.h) against the CPU reference reader vcfio.read_vcf: GT bytes,
AF bit for bit and sample names, on the reference's VCF fixtures and on seeded synthetic call sets of every genotype
shape read_vcf accepts, in plain, gzip and BGZF form; malformed records raise ValueError and leave the context usable."""
import os

import numpy as np
import pytest

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


@pytest.fixture(scope="module")
def reader():
    from utmos_amd.vcfgpu import GpuVcfReader
    with GpuVcfReader(device=0) as r:
        yield r


@pytest.mark.parametrize("name", ["chunk0.vcf.gz", "chunk1.vcf.gz", "chunk_tiny.vcf", "build_tiny.vcf"])
def test_fixtures_equal_cpu_reader(name, reader):
    from utmos_amd.vcfio import read_vcf
    path = os.path.join(VCF, name)
    assert_same(reader.read(path), read_vcf(path))


@pytest.mark.parametrize("n_samp", [1, 7, 63, 65, 2504])
@pytest.mark.parametrize("variant", ["mixed", "crlf-no-final-newline"])
def test_synthetic_all_forms(n_samp, variant, tmp_path):
    from utmos_amd.vcfgpu import GpuVcfReader
    from utmos_amd.vcfio import read_vcf
    n_rec = 60 if n_samp < 2504 else 25
    data = vcf_gen.make_vcf(n_samp * 7 + len(variant), n_rec, n_samp, big_alt=True, meta_among=True,
                            crlf=variant != "mixed", final_newline=variant == "mixed")
    paths = vcf_gen.write_forms(str(tmp_path), "s", data)
    want = read_vcf(paths["plain"])
    assert want["GT"].shape[0] == n_rec
    for batch in (64 << 20, 4096):          # 4 KiB batches: records cross batch borders, long ones grow the staging
        with GpuVcfReader(device=0, batch_bytes=batch) as r:
            for form, path in paths.items():
                assert_same(r.read(path), want)


def test_hundred_thousand_samples(tmp_path, reader):
    from utmos_amd.vcfio import read_vcf
    data = vcf_gen.make_vcf(5, 3, 100_000, formats=("GT", "GT:AD:DP", "DP:GT"))
    paths = vcf_gen.write_forms(str(tmp_path), "w", data)
    want = read_vcf(paths["plain"])
    for path in paths.values():
        assert_same(reader.read(path), want)


def test_record_over_one_mib(tmp_path):
    from utmos_amd.vcfgpu import GpuVcfReader
    from utmos_amd.vcfio import read_vcf
    data = vcf_gen.make_vcf(9, 6, 300, long_info=(1 << 20) + 12345, long_cells=True)
    paths = vcf_gen.write_forms(str(tmp_path), "l", data)
    want = read_vcf(paths["plain"])
    for batch in (64 << 20, 64 << 10):
        with GpuVcfReader(device=0, batch_bytes=batch) as r:
            for path in paths.values():
                assert_same(r.read(path), want)


def test_stats_and_singletons_match_a_cpu_restatement(tmp_path, reader):
    """het / hom-alt cells and the singleton flag (convert.py:58-69), restated per cell here."""
    data = vcf_gen.make_vcf(11, 80, 40, big_alt=True)
    path = str(tmp_path / "st.vcf")
    open(path, "wb").write(data)
    got = reader.read(path)
    het, hom, sing = [], [], []
    for line in data.decode().splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        n_alt = len(f[4].split(","))
        gi = f[8].split(":").index("GT")
        h = o = 0
        counts = np.zeros(n_alt + 1, np.int64)
        for cell in f[9:]:
            al = [-1 if a == "." else int(a) for a in cell.split(":")[gi].replace("|", "/").split("/")]
            for a in al:
                if 0 <= a <= n_alt:
                    counts[a] += 1
            called = len(al) > 1 and all(a >= 0 for a in al)
            if called and any(a != al[0] for a in al[1:]):
                h += 1
            elif called and al[0] > 0:
                o += 1
        het.append(h)
        hom.append(o)
        sing.append(counts[1] == 1 or counts[0] == 1)
    assert got["het"].tolist() == het and got["hom"].tolist() == hom
    assert got["singleton"].tolist() == sing
    assert got["stats"] == {"num_het": sum(het), "num_hom": sum(hom)}


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\n"
GOOD = "c\t1\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1|1\n"
MALFORMED = {
    "few-columns": "c\t1\t.\tA\tC\t.\t.\t.\n",
    "too-many-cells": "c\t1\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1|1\t0|0\n",
    "too-few-cells": "c\t1\t.\tA\tC\t.\t.\t.\tGT:DP\t0|1:3\n",
    "no-gt-in-format": "c\t1\t.\tA\tC\t.\t.\t.\tDP:AD\t3:1\t4:2\n",
    "cell-without-gt": "c\t1\t.\tA\tC\t.\t.\t.\tDP:GT\t3:0|1\t4\n",
    "bad-allele": "c\t1\t.\tA\tC\t.\t.\t.\tGT:DP\t0|x:1\t0|0:1\n",
    "empty-allele": "c\t1\t.\tA\tC\t.\t.\t.\tGT:DP\t0|:1\t0|0:1\n",
    "chrom-among-records": "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\n",
    "too-many-alts": "c\t1\t.\tA\t" + ",".join(["C"] * 5000) + "\t.\t.\t.\tGT\t0|1\t1|1\n",
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_raises_and_context_survives(case, tmp_path, reader):
    from utmos_amd.vcfio import read_vcf
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write(HEAD + GOOD * 3 + MALFORMED[case] + GOOD)
    handle = None
    for batch in (None, 64):     # (64-byte batches: the failure lands in a later batch with another one queued)
        if batch:
            from utmos_amd.vcfgpu import GpuVcfReader
            r = GpuVcfReader(device=0, batch_bytes=batch)
        else:
            r = reader
        with pytest.raises(ValueError, match="bad.vcf"):
            r.read(bad)
        handle = r.handle.value
        good = str(tmp_path / "good.vcf")
        open(good, "w").write(HEAD + GOOD * 5 + "c\t2\t.\tA\tC,G\t.\t.\t.\tGT\t0|2\t2|2\n")
        assert_same(r.read(good), read_vcf(good))
        assert r.handle.value == handle          # the same context
        if batch:
            r.close()


def test_record_before_header_and_missing_header(tmp_path, reader):
    p = str(tmp_path / "h.vcf")
    open(p, "w").write(GOOD + HEAD)
    with pytest.raises(ValueError, match="h.vcf"):
        reader.read(p)
    open(p, "w").write("##x\n" + GOOD)
    with pytest.raises(ValueError, match="h.vcf"):
        reader.read(p)
