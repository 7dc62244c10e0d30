"""`python -m utmos_amd convert` (GPU parser) against the reference's own conversions of its VCF fixtures
(tests/golden/jl/chunkN.jl = utmos convert of tests/golden/vcf/chunkN.vcf.gz), and `select` on its outputs."""
import os

import numpy as np
import pytest

import oracle_util as ou

VCF = os.path.join(ou.GOLD, "vcf")
CASES = ou.golden_cases()
STATS = {0: (58258, 43479), 1: (47978, 27512)}
pytestmark = pytest.mark.gpu


def run(cmd, argv):
    from utmos_amd.__main__ import main
    assert main([cmd] + argv) == 0


@pytest.mark.parametrize("n", [0, 1])
def test_convert_matches_the_references_conversion(n, tmp_path):
    import joblib
    out = str(tmp_path / f"chunk{n}.jl")
    run("convert", [os.path.join(VCF, f"chunk{n}.vcf.gz"), out])
    got = joblib.load(out)
    want = joblib.load(os.path.join(ou.GOLD, "jl", f"chunk{n}.jl"))
    assert set(got) == {"samples", "GT", "AF", "stats"}
    assert got["GT"].dtype == np.uint8 and got["GT"].shape == want["GT"].shape and (got["GT"] == want["GT"]).all()
    assert [str(s) for s in got["samples"]] == [str(s) for s in want["samples"]]
    assert (int(got["stats"]["num_het"]), int(got["stats"]["num_hom"])) == STATS[n]
    assert (int(want["stats"]["num_het"]), int(want["stats"]["num_hom"])) == STATS[n]
    assert got["AF"].dtype == np.float64 and got["AF"].shape == want["AF"].shape
    differ = np.flatnonzero(got["AF"].reshape(-1) != want["AF"].reshape(-1))
    assert len(differ) == (5, 4)[n]          # the multi-allelic rows (test_vcf_fixtures.py, vcfio.py)


@pytest.mark.parametrize("n", [0, 1])
def test_convert_no_singleton(n, tmp_path):
    """--no-singleton drops rows with counts[1] == 1 or counts[0] == 1 before the stats (convert.py:57-70), restated
    here from the CPU reader's per-cell rule."""
    import joblib
    from utmos_amd import vcfio
    path = os.path.join(VCF, f"chunk{n}.vcf.gz")
    out = str(tmp_path / "ns.jl")
    run("convert", ["--no-singleton", "-c", "1", path, out])
    got = joblib.load(out)
    keep, het, hom = [], 0, 0
    with __import__("gzip").open(path, "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            f = line.rstrip("\n").split("\t")
            n_alt = len(f[4].split(","))
            pres, counts = vcfio._cells_slow(f[9:], f[8].split(":").index("GT"), n_alt)
            sing = counts[1] == 1 or counts[0] == 1
            keep.append(not sing)
            if not sing:
                for cell in f[9:]:
                    al = [-1 if a == "." else int(a) for a in cell.split(":")[0].replace("|", "/").split("/")]
                    called = len(al) > 1 and min(al) >= 0
                    het += called and any(a != al[0] for a in al)
                    hom += called and all(a == al[0] for a in al) and al[0] > 0
    full = vcfio.read_vcf(path)
    keep = np.array(keep)
    assert 0 < keep.sum() < len(keep)
    assert (got["GT"] == full["GT"][keep]).all() and (got["AF"] == full["AF"][keep]).all()
    assert (int(got["stats"]["num_het"]), int(got["stats"]["num_hom"])) == (het, hom)


def test_select_on_converted_parts_equals_select_on_the_vcfs(tmp_path):
    from utmos_amd.select import select_main
    parts = {}
    for n in (0, 1):
        for ext in ("jl", "npz"):
            out = str(tmp_path / f"chunk{n}.{ext}")
            run("convert", [os.path.join(VCF, f"chunk{n}.vcf.gz"), out])
            parts[n, ext] = out
    chunk2 = os.path.join(ou.GOLD, "chunk2.npz")
    for ext in ("jl", "npz"):
        o1, o2 = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
        select_main(["-o", o1, parts[1, ext]])
        select_main(["-o", o2, os.path.join(VCF, "chunk1.vcf.gz")])
        assert open(o1).read() == open(o2).read() == ou.golden_text(CASES["select_fileout"])
        select_main(["-o", o1, parts[0, ext], chunk2])
        select_main(["-o", o2, os.path.join(VCF, "chunk0.vcf.gz"), chunk2])
        assert open(o1).read() == open(o2).read() == ou.golden_text(CASES["select_multi"])
