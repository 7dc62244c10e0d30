"""The commands on .bcf inputs: `select` on BCF encodings (tests/bcf_gen.py) of the reference's chunk0.vcf.gz and
chunk1.vcf.gz reproduces the goldens tests/test_vcf_fixtures.py ties to those VCFs, alone and mixed with .npz parts;
`convert` and `select --variants-out` give what they give for the VCF."""
import os

import numpy as np
import pytest

import bcf_gen
import oracle_util as ou

VCF = os.path.join(ou.GOLD, "vcf")
CASES = ou.golden_cases()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bcf(tmp_path_factory):
    """chunkN.vcf.gz -> chunkN.bcf (BGZF; chunk1 with IDX= in its header)."""
    d = tmp_path_factory.mktemp("bcf")
    out = {}
    for n in (0, 1):
        out[n] = str(d / f"chunk{n}.bcf")
        open(out[n], "wb").write(bcf_gen.make_bcf(bcf_gen.vcf_bytes(os.path.join(VCF, f"chunk{n}.vcf.gz")), idx=n == 1, level=1))
    return out


@pytest.mark.parametrize("argv,golden", [
    (["BCF1"], "select_fileout"),
    (["BCF0", "GOLD/chunk2.npz"], "select_multi"),
    (["--inflate", "host", "BCF0", "GOLD/chunk2.npz"], "select_multi"),
    (["--maxmem", "0", "--buffer", "300", "BCF0", "GOLD/chunk2.npz"], "select_multi"),
], ids=["fileout", "multimix", "multimix-host-inflate", "multimix-chunked"])
def test_select_on_bcf_reproduces_the_references_goldens(argv, golden, bcf, tmp_path):
    from utmos_amd.select import select_main
    out = str(tmp_path / "out.txt")
    select_main(["-o", out] + [a.replace("BCF0", bcf[0]).replace("BCF1", bcf[1]).replace("GOLD", ou.GOLD) for a in argv])
    assert open(out).read() == ou.golden_text(CASES[golden])


def test_convert_bcf_equals_convert_vcf(bcf, tmp_path):
    from utmos_amd.convert import cvt_main
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    cvt_main([bcf[0], a])
    cvt_main([os.path.join(VCF, "chunk0.vcf.gz"), b])
    with np.load(a) as za, np.load(b) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and (za[k] == zb[k]).all()
    c, d = str(tmp_path / "c.npz"), str(tmp_path / "d.npz")
    cvt_main(["--no-singleton", bcf[0], c])
    cvt_main(["--no-singleton", os.path.join(VCF, "chunk0.vcf.gz"), d])
    with np.load(c) as zc, np.load(d) as zd, np.load(a) as za:
        assert zc["GT"].shape[0] < za["GT"].shape[0] and (zc["GT"] == zd["GT"]).all() and (zc["AF"] == zd["AF"]).all()


def test_variants_out_on_bcf_reports_the_same_part_and_row(bcf, tmp_path):
    from utmos_amd.select import select_main
    got = {}
    for name, first in (("bcf", bcf[0]), ("vcf", os.path.join(VCF, "chunk0.vcf.gz"))):
        tsv, npz = str(tmp_path / f"{name}.txt"), str(tmp_path / f"{name}.npz")
        select_main(["-c", "10", "-o", tsv, "--variants-out", npz, first, os.path.join(ou.GOLD, "chunk2.npz")])
        with np.load(npz) as z:
            got[name] = (open(tsv).read(), {k: z[k] for k in z.files})
    assert got["bcf"][0] == got["vcf"][0]
    assert sorted(got["bcf"][1]) == sorted(got["vcf"][1]) and {"part", "row"} <= set(got["bcf"][1])
    for k, v in got["vcf"][1].items():
        if v.dtype.kind in "US":           # file names differ by design
            continue
        assert (got["bcf"][1][k] == v).all(), k
