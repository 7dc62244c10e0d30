"""Seeded synthetic VCFs for the GPU reader's tests: every genotype shape vcfio.read_vcf accepts, in plain, gzip and BGZF
form."""
import gzip
import os

import numpy as np


def _gt(rng, n_alt, ploidy_mix, missing):
    ploidy = 2
    if ploidy_mix:
        ploidy = rng.choice([1, 2, 2, 2, 3])
    al = []
    for _ in range(ploidy):
        if missing and rng.random() < 0.08:
            al.append(".")
        else:
            a = 0 if rng.random() < 0.6 else int(rng.integers(1, n_alt + 1))
            al.append(str(a))
    if missing and rng.random() < 0.02:
        return "."
    sep = "|" if rng.random() < 0.7 else "/"
    out = al[0]
    for a in al[1:]:
        out += (sep if rng.random() < 0.9 else "/|"[sep == "/"]) + a
    return out


def make_vcf(seed, n_rec, n_samp, formats=("GT", "GT:AD:DP", "DP:GT"), big_alt=False, ploidy_mix=True, missing=True,
             crlf=False, final_newline=True, meta_among=False, long_info=0, long_cells=False):
    """-> VCF bytes.  formats: FORMAT strings the records cycle through (GT records with one-digit diploid calls take
    the fixed-width fast path).  big_alt: some records with hundreds of alt alleles (multi-digit alleles).
    long_info: bytes of INFO in record 1.  long_cells: record 2 carries a long AD subfield in every cell."""
    rng = np.random.default_rng(seed)
    nl = "\r\n" if crlf else "\n"
    lines = ["##fileformat=VCFv4.2", "##source=vcf_gen",
             "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] +
                       [f"S{i:06d}" for i in range(n_samp)])]
    for r in range(n_rec):
        fmt = formats[r % len(formats)]
        n_alt = 1
        if big_alt and r % 5 == 3:
            n_alt = int(rng.integers(100, 400))
        elif rng.random() < 0.3:
            n_alt = int(rng.integers(2, 13))
        alt = ",".join(["ACGT"[k % 4] * (1 + k // 4 % 3) for k in range(n_alt)])
        info = "AC=1;AN=2" if not (long_info and r == 1) else "X=" + "y" * long_info
        simple = fmt == "GT" and r % 3 == 0     # one-digit diploid calls only
        cells = []
        for _ in range(n_samp):
            if simple:
                a = [str(int(x)) if rng.random() > 0.05 or not missing else "." for x in rng.integers(0, min(n_alt, 9) + 1, 2)]
                g = a[0] + ("|" if rng.random() < 0.8 else "/") + a[1]
            else:
                g = _gt(rng, n_alt, ploidy_mix, missing)
            if fmt == "GT":
                cells.append(g)
            elif fmt == "GT:AD:DP":
                ad = ",".join(["7"] * (60 if long_cells and r == 2 else 2))
                cells.append(f"{g}:{ad}:14")
            else:
                cells.append(f"{int(rng.integers(0, 99))}:{g}")
        lines.append("\t".join(["chr1", str(1000 + r), ".", "A", alt, "50", "PASS", info, fmt] + cells))
        if meta_among and r % 7 == 2:
            lines.append("##among=records")
    text = nl.join(lines)
    if final_newline:
        text += nl
    return text.encode()


def write_forms(tmp_dir, name, data):
    """data written plain (.vcf), as one gzip stream and as BGZF (.vcf.gz) -> {form: path}."""
    from utmos_amd.vcfgpu import bgzf_compress
    paths = {"plain": os.path.join(tmp_dir, name + ".vcf"),
             "gzip": os.path.join(tmp_dir, name + ".gzip.vcf.gz"),
             "bgzf": os.path.join(tmp_dir, name + ".bgzf.vcf.gz")}
    with open(paths["plain"], "wb") as fh:
        fh.write(data)
    with open(paths["gzip"], "wb") as fh:
        fh.write(gzip.compress(data, 6))
    with open(paths["bgzf"], "wb") as fh:
        fh.write(bgzf_compress(data, block=4000))   # small members: many of them, and records across their borders
    return paths
