"""`python -m utmos_amd overlap`: how many variants every two samples share.

One pass over the HBM-resident matrix (DeviceMatrix.pair_counts -> utm_pair_counts: a bit-matrix product of the listed
columns with themselves) gives shared[a, b] for every pair of the listed samples, optionally counting only the variants
that no sample of a `--given` panel carries.  Duplicates and close relatives have a Jaccard index near 1; with
`--given PANEL --sort joint` the first row is the pair that captures the most new variants together.  The reference has
no such command.

    pair_rows(shared, names, sort, top)     the TSV rows: a pure function of the matrix and the names
    overlap_main(cmdargs)                   load (select.load_files), count, write
"""
import argparse
import logging
import os
import sys

import numpy as np

from . import select

PAIRS_HEADER = "sample_a\tsample_b\tcount_a\tcount_b\tshared\tjaccard\tjoint\n"
SORT_KEYS = ("jaccard", "joint", "shared")


def pair_rows(shared, names, sort="jaccard", top=20):
    """[sample_a, sample_b, count_a, count_b, shared, jaccard, joint] for the pairs a < b (positions in `names`), highest
    `sort` first, ties to the smaller a and then the smaller b; at most `top` rows (-1: all).  count = the diagonal,
    joint = count_a + count_b - shared = the union, jaccard = round(shared / joint, 4) and 0 for an empty union."""
    if sort not in SORT_KEYS:
        raise ValueError(f"sort must be one of {SORT_KEYS}")
    shared = np.asarray(shared, dtype=np.int64)
    n = len(names)
    if shared.shape != (n, n):
        raise ValueError(f"a {n} x {n} matrix is needed for {n} names")
    a, b = np.triu_indices(n, k=1)                          # a < b, by a and then by b
    count = np.diagonal(shared)
    both = shared[a, b]
    joint = count[a] + count[b] - both
    jaccard = np.round(np.divide(both, joint, out=np.zeros(len(both), np.float64), where=joint != 0), 4)
    key = {"jaccard": jaccard, "joint": joint, "shared": both}[sort]
    order = np.argsort(-key, kind="stable")                 # stable: ties keep the (a, b) order
    if top >= 0:
        order = order[:top]
    return [[str(names[a[k]]), str(names[b[k]]), int(count[a[k]]), int(count[b[k]]), int(both[k]), float(jaccard[k]),
             int(joint[k])] for k in order]


def write_pairs(fout, rows):
    fout.write(PAIRS_HEADER)
    for row in rows:
        fout.write("\t".join(str(field) for field in row) + "\n")


def resolve_given(names, given):
    """--given names -> sample indices, later duplicates dropped.  Exits with status 1 on a name the input lacks."""
    position = {name: i for i, name in enumerate(names)}
    out = []
    for name in given or ():
        if name not in position:
            logging.error("--given: sample %s is not in the input", name)
            sys.exit(1)
        if position[name] not in out:
            out.append(position[name])
    return np.asarray(out, dtype=np.int64)


def _build_parser():
    parser = argparse.ArgumentParser(prog="overlap", description="Count the variants every two samples share (MI355X).")
    parser.add_argument("in_files", nargs="*", type=str, help="inputs: .vcf[.gz], .bcf, .jl, .npz parts, or one packed .utm or .hdf5 store")
    parser.add_argument("-o", "--out", type=str, default=None, metavar="FILE.npz",
                        help="write the whole matrix: shared (int64, n x n), samples, count, given, files (numpy .npz)")
    parser.add_argument("--pairs-out", type=str, default=None, metavar="FILE",
                        help="TSV of the pairs [stdout, unless -o is given]")
    parser.add_argument("--sort", choices=list(SORT_KEYS), default="jaccard", help="order of the pairs, descending [%(default)s]")
    parser.add_argument("--top", type=int, default=20, help="how many pairs to write; -1 = all [%(default)s]")
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
        logging.error("overlap needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.af:
        logging.error("overlap counts presence, not allele frequency: remove --af (an AF store is read for its presence bits)")
        sys.exit(1)
    if args.top < -1:
        logging.error("--top takes a number of pairs, or -1 for all")
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


def overlap_main(cmdargs):
    args = parse_args(cmdargs)
    select.MAXMEM = args.maxmem
    data = select.load_files(args.in_files, args.lowmem, args.buffer, False, args.device, None, args.inflate)
    matrix = data["data"]
    try:
        names = np.asarray(data["samples"]).astype(str)
        states = select.sample_states(names, select.parse_sample_lists(args.subset), select.parse_sample_lists(args.exclude))
        listed = np.flatnonzero(states == select.SELECTABLE)
        given = resolve_given(names, select.parse_sample_lists(args.given))
        logging.info("%d of %d samples listed, %d given, %d variants", len(listed), len(names), len(given), matrix.shape[0])
        shared = matrix.pair_counts(listed, given) if matrix.chunk_vars else np.zeros((len(listed), len(listed)), np.int64)
    finally:
        matrix.close()
    if args.out:
        np.savez(args.out, shared=shared, samples=names[listed], count=np.diagonal(shared).copy(), given=names[given],
                 files=np.asarray([str(name) for name in args.in_files], dtype=str))
        logging.info("%s: shared counts of %d samples", args.out, len(listed))
    pairs_out = args.pairs_out or (None if args.out else "/dev/stdout")
    if pairs_out:
        with open(pairs_out, "w") as fout:
            write_pairs(fout, pair_rows(shared, names[listed], args.sort, args.top))
    logging.info("utmos overlap finished")
