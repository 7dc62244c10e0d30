"""Variant filters: restrict a loaded matrix to some of its variants before anything runs on it.

The criteria (they combine with AND) become one boolean mask per HBM chunk on the host -- numpy over at most a few
million values -- and `DeviceMatrix.filter_variants` compacts every column on the GPU (utm_filter_variants).  What the
reference offers instead is filtering the VCF with bcftools and converting again.

    --min-af X / --max-af Y                 X <= AF <= Y, the AF as the loader holds it (float64 from part files, float32
                                            from stores), compared by its exact value with the bound as a float64
    --min-carriers A / --max-carriers B     A <= carriers <= B, counted over the run's cohort: the samples that are not
                                            excluded by --subset / --exclude
    --keep-variants / --drop-variants F.npz the arrays `part` and `row` of a `select --variants-out` file (or a selection
                                            of its entries): input file number and record number inside it

The invariant every detail follows: the output of a filtered run is byte for byte that of the same command on inputs
from which the dropped records had been removed beforehand.

`filter_main` is the `filter` command: load, filter, write the kept variants as a .utm store.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np


class FilterError(ValueError):
    """A criterion cannot be applied to this input (the message says why)."""


class Criteria:
    """The criteria of one run.  `active` is false when none was given."""

    def __init__(self, min_af=None, max_af=None, min_carriers=None, max_carriers=None, keep_variants=None, drop_variants=None):
        self.min_af, self.max_af = min_af, max_af
        self.min_carriers, self.max_carriers = min_carriers, max_carriers
        self.keep_variants, self.drop_variants = keep_variants, drop_variants

    @classmethod
    def from_args(cls, args):
        return cls(args.min_af, args.max_af, args.min_carriers, args.max_carriers, args.keep_variants, args.drop_variants)

    @property
    def needs_af(self):
        return self.min_af is not None or self.max_af is not None

    @property
    def needs_carriers(self):
        return self.min_carriers is not None or self.max_carriers is not None

    @property
    def needs_origin(self):
        return self.keep_variants is not None or self.drop_variants is not None

    @property
    def active(self):
        return self.needs_af or self.needs_carriers or self.needs_origin

    def flags(self):
        return [flag for flag, value in (("--min-af", self.min_af), ("--max-af", self.max_af), ("--min-carriers", self.min_carriers),
                                         ("--max-carriers", self.max_carriers), ("--keep-variants", self.keep_variants),
                                         ("--drop-variants", self.drop_variants)) if value is not None]


def add_arguments(parser):
    """The option group "variants", shared by `select` and `filter`."""
    group = parser.add_argument_group("Variant Arguments", "use only some of the variants (the criteria combine with AND)")
    group.add_argument("--min-af", type=float, default=None, metavar="X", help="keep variants with AF >= X")
    group.add_argument("--max-af", type=float, default=None, metavar="Y", help="keep variants with AF <= Y")
    group.add_argument("--min-carriers", type=int, default=None, metavar="A",
                       help="keep variants that at least A samples of the cohort (after --subset / --exclude) carry; 2 = no singletons")
    group.add_argument("--max-carriers", type=int, default=None, metavar="B", help="keep variants that at most B samples of the cohort carry")
    group.add_argument("--keep-variants", type=str, default=None, metavar="FILE.npz",
                       help="keep only the variants listed by the arrays part and row, as --variants-out writes them")
    group.add_argument("--drop-variants", type=str, default=None, metavar="FILE.npz", help="drop the variants listed that way")
    return group


# ---------------------------------------------------------------------------------------------- the criteria as masks
def af_mask(af, min_af=None, max_af=None):
    """min_af <= AF <= max_af, both bounds inclusive, every AF taken at its exact value (a float32 is widened)."""
    af = np.asarray(af).astype(np.float64)
    keep = np.ones(len(af), dtype=bool)
    if min_af is not None:
        keep &= af >= np.float64(min_af)
    if max_af is not None:
        keep &= af <= np.float64(max_af)
    return keep


def carrier_mask(counts, min_carriers=None, max_carriers=None):
    """min_carriers <= carriers <= max_carriers, both bounds inclusive."""
    counts = np.asarray(counts)
    keep = np.ones(len(counts), dtype=bool)
    if min_carriers is not None:
        keep &= counts >= int(min_carriers)
    if max_carriers is not None:
        keep &= counts <= int(max_carriers)
    return keep


def read_variant_list(path):
    """(part, row) int64 arrays of a --keep-variants / --drop-variants file."""
    try:
        with np.load(path, allow_pickle=False) as z:
            missing = [name for name in ("part", "row") if name not in z.files]
            if missing:
                raise FilterError(f"{path}: no array `{missing[0]}` (expected `part` and `row`, as --variants-out writes them)")
            part, row = np.asarray(z["part"]).astype(np.int64).reshape(-1), np.asarray(z["row"]).astype(np.int64).reshape(-1)
    except (OSError, ValueError) as err:
        if isinstance(err, FilterError):
            raise
        raise FilterError(f"{path}: cannot be read as a numpy .npz file ({err})") from err
    if len(part) != len(row):
        raise FilterError(f"{path}: `part` has {len(part)} entries and `row` {len(row)}")
    return part, row


def listed_mask(origin_part, origin_row, listed_part, listed_row, what="the list"):
    """True for the variants of the matrix -- (origin_part[i], origin_row[i]) each -- that the list names.  A listed
    variant the matrix does not have is an error."""
    origin = np.stack([np.asarray(origin_part, dtype=np.int64), np.asarray(origin_row, dtype=np.int64)], axis=1)
    listed = np.stack([np.asarray(listed_part, dtype=np.int64), np.asarray(listed_row, dtype=np.int64)], axis=1)
    pair = np.dtype([("part", np.int64), ("row", np.int64)])
    origin_keys = np.ascontiguousarray(origin).view(pair).reshape(-1)
    listed_keys = np.ascontiguousarray(listed).view(pair).reshape(-1)
    known = np.isin(listed_keys, origin_keys)
    if not known.all():
        first = listed[np.flatnonzero(~known)[0]]
        raise FilterError(f"{what}: variant (part {int(first[0])}, row {int(first[1])}) is not among the informative variants of the "
                          f"input ({int((~known).sum())} such entries)")
    return np.isin(origin_keys, listed_keys)


def cohort_indices(names, subset, exclude):
    """The samples carriers are counted over: everyone --subset / --exclude leave (an --include sample is one of them)."""
    names = np.asarray(names).astype(str)
    inside = np.ones(len(names), dtype=bool)
    if subset:
        inside &= np.isin(names, subset)
    if exclude:
        inside &= ~np.isin(names, exclude)
    return np.flatnonzero(inside).astype(np.int64)


def build_masks(criteria, chunk_vars, chunk_af=None, chunk_counts=None, origin=None):
    """One boolean mask per chunk.  chunk_af / chunk_counts: per-chunk arrays (needed by the AF / carrier criteria);
    origin: {"part", "row"} over all variants in matrix order (needed by the lists)."""
    total = int(sum(chunk_vars))
    keep = np.ones(total, dtype=bool)
    if criteria.needs_af:
        if chunk_af is None:
            raise FilterError("--min-af / --max-af need allele frequencies, and this input carries none (a store written without --af)")
        keep &= af_mask(np.concatenate([np.asarray(a) for a in chunk_af]) if len(chunk_af) else np.zeros(0), criteria.min_af, criteria.max_af)
    if criteria.needs_carriers:
        keep &= carrier_mask(np.concatenate(chunk_counts) if len(chunk_counts) else np.zeros(0, np.int32), criteria.min_carriers,
                             criteria.max_carriers)
    for path, wanted in ((criteria.keep_variants, True), (criteria.drop_variants, False)):
        if path is None:
            continue
        part, row = read_variant_list(path)
        listed = listed_mask(origin["part"], origin["row"], part, row, path)
        keep &= listed if wanted else ~listed
    bounds = np.cumsum([0] + [int(n) for n in chunk_vars])
    return [keep[bounds[k]:bounds[k + 1]] for k in range(len(chunk_vars))]


def apply(matrix, criteria, names, subset=None, exclude=None, chunk_af=None, origin=None):
    """Filter every chunk of `matrix` in place; returns the per-chunk masks.  FilterError when a criterion cannot be
    applied or no variant is left."""
    counts = None
    if criteria.needs_carriers:
        cohort = cohort_indices(names, subset, exclude)
        counts = matrix.carrier_counts(cohort, counts=True)[1]
    before = list(matrix.chunk_vars)
    masks = build_masks(criteria, before, chunk_af, counts, origin)
    kept = int(sum(int(m.sum()) for m in masks))
    if kept == 0:
        raise FilterError(f"no variants are left after {' '.join(criteria.flags())} (of {int(sum(before))})")
    for chunk, mask in enumerate(masks):
        matrix.filter_variants(chunk, mask)
    logging.info("variant filters %s: %d of %d variants kept", " ".join(criteria.flags()), kept, int(sum(before)))
    return masks


def refuse_several_processes(criteria):
    if criteria.active and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("%s need the whole sample axis on one GPU: run a single process", " / ".join(criteria.flags()))
        sys.exit(1)


# ---------------------------------------------------------------------------------------------- the filter command
def _build_parser():
    parser = argparse.ArgumentParser(prog="filter", description="Write the variants that pass the criteria, and all samples, as a .utm store (MI355X).")
    parser.add_argument("in_files", nargs="+", type=str, help="inputs: .vcf[.gz], .bcf, .jl, .npz parts, or one packed .utm or .hdf5 store")
    parser.add_argument("-o", "--out", type=str, required=True, metavar="OUT.utm", help="the store to write")
    parser.add_argument("--kept-out", type=str, default=None, metavar="FILE.npz",
                        help="also write part, row (and af) of the kept variants in store order: the store itself forgets where its rows came from")
    parser.add_argument("--af", action="store_true", help="keep the allele frequencies in the store (a later select --af needs them)")
    parser.add_argument("--subset", type=str, default=None, action="append", help="the cohort of --min/--max-carriers: only these samples (file or comma list; repeatable)")
    parser.add_argument("--exclude", type=str, default=None, action="append", help="... and none of these")
    parser.add_argument("--buffer", type=int, default=32768, help="variants per HBM chunk when chunking is on [%(default)s]")
    parser.add_argument("--maxmem", type=int, default=2, help="GB one chunk may take; 0 = always chunk [%(default)s]")
    parser.add_argument("--device", type=int, default=0, help="GPU index [%(default)s]")
    parser.add_argument("--debug", action="store_true", help="debug-level logging")
    add_arguments(parser)
    return parser


def filter_main(cmdargs):
    """`utmos filter`: load, filter on the GPU, write the kept variants (all samples) through StoreWriter."""
    from . import select
    from .store import SUFFIX, StoreWriter
    args = _build_parser().parse_args(cmdargs)
    select.setup_logging(args.debug)
    logging.info("options in effect: %s", json.dumps({k: v for k, v in vars(args).items() if v is not None}, sort_keys=True))
    criteria = Criteria.from_args(args)
    refuse_several_processes(criteria)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("filter writes one store: run a single process")
        sys.exit(1)
    if not args.out.endswith(SUFFIX):
        logging.error("-o takes a %s store", SUFFIX)
        sys.exit(1)
    stores = [name for name in args.in_files if name.endswith((SUFFIX, select.H5_SUFFIX))]
    if stores and len(args.in_files) > 1:
        logging.error("A matrix store cannot be combined with other input files")
        sys.exit(1)
    missing = [path for path in args.in_files if not os.path.exists(path)]
    if missing:
        logging.error("Input %s does not exist", missing[0])
        sys.exit(1)
    select.MAXMEM = args.maxmem
    data = select.load_files(args.in_files, 1 if stores else None, args.buffer, args.af, args.device, None, "auto", origin=True,
                             variants=(criteria, select.parse_sample_lists(args.subset), select.parse_sample_lists(args.exclude)))
    matrix = data["data"]
    try:
        if args.af and not data["has_af"]:
            logging.error("The input carries no allele frequencies: remove --af")
            sys.exit(1)
        keep_af = bool(data["has_af"])
        origin = data["origin"]
        bounds = np.cumsum([0] + list(matrix.chunk_vars))
        with StoreWriter(args.out, data["samples"], keep_af) as writer:
            for chunk, n_var in enumerate(matrix.chunk_vars):
                if n_var == 0:
                    continue
                af = np.asarray(origin["af"][bounds[chunk]:bounds[chunk + 1]], dtype=np.float32) if keep_af else None
                writer.add_chunk(n_var, matrix.download_columns(chunk), af)
            writer.finish(data["var_count"])
        if args.kept_out:
            arrays = {"part": origin["part"], "row": origin["row"]}
            if origin["af"] is not None:
                arrays["af"] = origin["af"]
            arrays["files"] = np.asarray([str(name) for name in args.in_files], dtype=str)
            np.savez(args.kept_out, **arrays)
        logging.info("%s: %d variants x %d samples", args.out, matrix.shape[0], matrix.shape[1])
    finally:
        matrix.close()
    logging.info("utmos filter finished")
