"""`python -m utmos_amd spectrum`: how many of the listed samples carry each variant.

One pass over the HBM-resident matrix (DeviceMatrix.carrier_counts -> utm_carrier_counts: a bit-sliced counter over the
listed columns) gives hist[c] = the number of variants that exactly c of the listed samples carry -- the site-frequency
spectrum of the list -- optionally counting only the variants that no sample of a `--given` panel carries.  From the
histogram alone follows, in closed form, the curve `select --mode random --seed S` only samples: a uniformly random panel
of k of the n listed samples misses a variant with c carriers with probability C(n - c, k) / C(n, k), so the expected
coverage for every k needs no seeds and carries no Monte-Carlo noise.  That is the baseline a greedy curve is plotted
against.  The reference has no such command.

    expected_curve(hist)                    E[0..n]: expected number of variants a random panel of k captures
    classes(hist, quorum)                   private / core / soft_core / absent / total
    write_spectrum, write_curve             the two TSVs: pure functions of the histogram
    spectrum_main(cmdargs)                  load (select.load_files), count, write
"""
import argparse
import logging
import math
import os
import sys

import numpy as np

from . import select
from .overlap import resolve_given

SPECTRUM_HEADER = "carriers\tvariants\tpct\n"
CLASSES_MAX = 16384                             # UTM_CLASSES_MAX
CURVE_HEADER = "k\texpected_captured\texpected_new\tpct_captured\n"


def expected_curve(hist):
    """float64 E[0..n] for a histogram over 0..n carriers: E[k] = sum over c >= 1 of hist[c] * (1 - r_c(k)), where
    r_c(k) = C(n - c, k) / C(n, k) is the chance that k of the n samples, drawn without replacement, miss all c carriers.
    r_c(0) = 1 and r_c(k + 1) = r_c(k) * max(n - c - k, 0) / (n - k): one vector operation over c per k, O(n^2) in all,
    no big numbers.  Every r_c(n) with c >= 1 is exactly 0, so E[n] is exactly hist[1:].sum()."""
    hist = np.asarray(hist)
    if hist.ndim != 1 or len(hist) == 0:
        raise ValueError("a histogram over 0..n carriers has n + 1 entries")
    n = len(hist) - 1
    weight = hist[1:].astype(np.float64)
    c = np.arange(1, n + 1, dtype=np.int64)
    r = np.ones(n, dtype=np.float64)
    out = np.zeros(n + 1, dtype=np.float64)
    for k in range(n):
        r *= np.maximum(n - c - k, 0) / float(n - k)
        out[k + 1] = (weight * (1.0 - r)).sum()
    return out


def classes(hist, quorum=0.95):
    """{"private": c == 1, "core": c == n, "soft_core": c >= ceil(quorum * n), "absent": c == 0, "total": all} of a
    histogram over 0..n carriers.  A variant nobody carries is in no core: the soft-core threshold is at least 1, and an
    empty list has no private and no core variants."""
    hist = np.asarray(hist, dtype=np.int64)
    n = len(hist) - 1
    if n < 0:
        raise ValueError("a histogram over 0..n carriers has n + 1 entries")
    if not 0.0 <= quorum <= 1.0:
        raise ValueError("quorum is a fraction of the listed samples")
    threshold = max(1, math.ceil(quorum * n))
    return {"private": int(hist[1]) if n >= 1 else 0, "core": int(hist[n]) if n >= 1 else 0,
            "soft_core": int(hist[threshold:].sum()), "absent": int(hist[0]), "total": int(hist.sum())}


def write_spectrum(fout, hist):
    """carriers, variants, pct = round(variants / total, 4) for every c in 0..n; total = the histogram's sum (pct 0.0 for
    an empty one)."""
    total = int(np.sum(hist))
    fout.write(SPECTRUM_HEADER)
    for c, variants in enumerate(hist):
        fout.write(f"{c}\t{int(variants)}\t{round(int(variants) / total, 4) if total else 0.0}\n")


def write_curve(fout, hist):
    """k, expected_captured = E[k], expected_new = E[k] - E[k - 1] (both %.2f) and pct_captured = round(E[k] / total, 4)
    for k in 1..n: the columns to lay over a `select` TSV's tot_captured, new_count and pct_captured."""
    total = int(np.sum(hist))
    curve = expected_curve(hist)
    fout.write(CURVE_HEADER)
    for k in range(1, len(curve)):
        fout.write("%d\t%.2f\t%.2f\t%s\n" % (k, curve[k], curve[k] - curve[k - 1], round(curve[k] / total, 4) if total else 0.0))


def _build_parser():
    parser = argparse.ArgumentParser(prog="spectrum", description="Carrier-count histogram of the listed samples and the exact "
                                                                  "expected coverage of a random panel (MI355X).")
    parser.add_argument("in_files", nargs="*", type=str, help="inputs: .vcf[.gz], .bcf, .jl, .npz parts, or one packed .utm or .hdf5 store")
    parser.add_argument("-o", "--out", type=str, default="/dev/stdout", metavar="FILE",
                        help="TSV of the histogram: carriers, variants, pct [stdout]")
    parser.add_argument("--curve-out", type=str, default=None, metavar="FILE",
                        help="TSV of the expected coverage of a random panel of k = 1..n listed samples")
    parser.add_argument("--counts-out", type=str, default=None, metavar="FILE.npz",
                        help="per variant: count (int32, -1 under --given), part, row; samples, given, files, hist (numpy .npz)")
    parser.add_argument("--by-sample", type=str, default=None, metavar="FILE.npz",
                        help="per listed sample: table[j, c] = the variants sample j carries that exactly c listed samples "
                             "carry (column 1: its singletons); samples, table (numpy .npz)")
    parser.add_argument("--quorum", type=float, default=0.95, help="soft core: carried by at least this share of the listed samples [%(default)s]")
    parser.add_argument("--debug", action="store_true", help="debug-level logging")
    samples = parser.add_argument_group("Sample Arguments")
    samples.add_argument("--subset", type=str, default=None, action="append",
                         help="only these samples (file or comma list; repeatable)")
    samples.add_argument("--exclude", type=str, default=None, action="append",
                         help="not these samples (file or comma list; repeatable)")
    samples.add_argument("--given", type=str, default=None, action="append",
                         help="leave out every variant one of these samples carries (file or comma list; repeatable)")
    samples.add_argument("--af", action="store_true", help=argparse.SUPPRESS)
    memory = parser.add_argument_group("Memory Arguments")
    memory.add_argument("--buffer", type=int, default=32768, help="variants per HBM chunk when chunking is on [%(default)s]")
    memory.add_argument("--maxmem", type=int, default=2, help="GB one chunk may take; 0 = always chunk [%(default)s]")
    gpu = parser.add_argument_group("GPU Arguments")
    gpu.add_argument("--device", type=int, default=0, help="GPU index [%(default)s]")
    gpu.add_argument("--inflate", choices=["auto", "gpu", "host"], default="auto",
                     help="where BGZF (.vcf.gz from bgzip, .bcf) input is inflated [%(default)s]")
    return parser


def parse_args(cmdargs):
    """Parse and validate; exits with status 1, before anything is loaded, on what the command refuses."""
    args = _build_parser().parse_args(cmdargs)
    select.setup_logging(args.debug)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("spectrum needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.af:
        logging.error("spectrum counts carriers, not allele frequency: remove --af (an AF store is read for its presence bits)")
        sys.exit(1)
    if not 0.0 <= args.quorum <= 1.0:
        logging.error("--quorum takes a share of the listed samples between 0 and 1")
        sys.exit(1)
    if not args.in_files:
        logging.error("Nothing to read: give input files or a matrix store")
        sys.exit(1)
    stores = [name for name in args.in_files if name.endswith((select.STORE_SUFFIX, select.H5_SUFFIX))]
    if stores and len(args.in_files) > 1:
        logging.error("A matrix store cannot be combined with other input files")
        sys.exit(1)
    missing = [path for path in args.in_files if not os.path.exists(path)]
    if missing:
        logging.error("Input %s does not exist", missing[0])
        sys.exit(1)
    args.lowmem = 1 if stores else None
    return args


def spectrum_main(cmdargs):
    args = parse_args(cmdargs)
    select.MAXMEM = args.maxmem
    data = select.load_files(args.in_files, args.lowmem, args.buffer, False, args.device, None, args.inflate,
                             **({"origin": True} if args.counts_out else {}))
    matrix = data["data"]
    try:
        names = np.asarray(data["samples"]).astype(str)
        states = select.sample_states(names, select.parse_sample_lists(args.subset), select.parse_sample_lists(args.exclude))
        listed = np.flatnonzero(states == select.SELECTABLE)
        given = resolve_given(names, select.parse_sample_lists(args.given))
        logging.info("%d of %d samples listed, %d given, %d variants", len(listed), len(names), len(given), matrix.shape[0])
        if args.by_sample and len(listed) + 1 > CLASSES_MAX:
            logging.error("--by-sample holds %d classes: %d listed samples need %d", CLASSES_MAX, len(listed), len(listed) + 1)
            sys.exit(1)
        if args.counts_out or args.by_sample:
            hist, counts = matrix.carrier_counts(listed, given, counts=True)
        else:
            hist, counts = matrix.carrier_counts(listed, given), None
        # the carrier count as class: -1 (a `given` sample carries the variant) stays -1 and is counted nowhere
        table = matrix.class_counts(counts, len(listed) + 1, listed) if args.by_sample else None
    finally:
        matrix.close()
    found = classes(hist, args.quorum)
    logging.info("%d variants beyond the given panel: %d absent, %d private, %d core, %d soft core (at least %d of %d samples)",
                 found["total"], found["absent"], found["private"], found["core"], found["soft_core"],
                 max(1, math.ceil(args.quorum * len(listed))), len(listed))
    if args.counts_out:
        origin = data["origin"]
        np.savez(args.counts_out, count=np.concatenate(counts) if counts else np.zeros(0, np.int32), part=origin["part"],
                 row=origin["row"], samples=names[listed], given=names[given],
                 files=np.asarray([str(name) for name in args.in_files], dtype=str), hist=hist)
        logging.info("%s: carrier counts of %d variants among %d samples", args.counts_out, matrix.shape[0], len(listed))
    if args.by_sample:
        np.savez(args.by_sample, samples=names[listed], table=table)
        logging.info("%s: frequency spectra of %d samples", args.by_sample, len(listed))
    with open(args.out, "w") as fout:
        write_spectrum(fout, hist)
    if args.curve_out:
        with open(args.curve_out, "w") as fout:
            write_curve(fout, hist)
    logging.info("utmos spectrum finished")
