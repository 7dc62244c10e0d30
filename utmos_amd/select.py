"""`utmos select` on MI355X: the host side of the greedy maximum-coverage selection.

The entry points carry the names and argument meaning of the reference's module so that a caller of
utmos/select.py can switch over (what each one answers to is cited; the bodies are this build's own):

    calculate_scores(matrix, sample_mask, sample_weights)              utmos/select.py:24-53
    greedy_select(matrix, total_variant_count, select_count, ...)      utmos/select.py:69-137
    run_selection(data, select_count, subset, exclude, weights)        utmos/select.py:147-195
                  (+ include, mode, seed: a fixed prefix, and SVCollector's topN / random orders, utmos/select.py:140-142)
    refined_selection(data, select_count, ..., max_swaps)              (no counterpart: greedy + 1-swap local search)
    load_files(in_files, lowmem, buffer, calc_af)                      utmos/select.py:241-321
    parse_sample_lists / parse_weights / parse_args / select_main      utmos/select.py:327-448

`matrix` is a device.DeviceMatrix: bit-packed sample columns resident in HBM, scored by hand-written HIP kernels
behind libutmos_hip.so.  There is no CPU path: every scoring call goes through the C ABI and raises if the
library or a GPU is missing.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

from . import device
from .store import SUFFIX as STORE_SUFFIX
from .store import StoreReader, StoreWriter

MAXMEM = 2  # GB one HBM chunk of packed columns may take; 0 = smallest chunks (the reference's test hook, select.py:18-19)

HEADER = "sample\tvar_count\tnew_count\ttot_captured\tpct_captured\n"
MAX_PANEL = 16383   # --samples-out / --represent-out: UTM_CLASSES_MAX - 1 rows + the class of the never-captured variants
HEADER_DEPTH = HEADER[:-1] + "\tat_depth\n"   # --depth M > 1: + variants that M selected samples carry
MAX_DEPTH = 255

H5_SUFFIX = ".hdf5"                      # the reference's --lowmem store: read (h5store.py) and written (h5write.py)

SELECTABLE, USED, EXCLUDED = 1, 0, 2      # sample_mask values (select.py:168: "1 = can use, 0 = mask, 2 = exclude")


# ---------------------------------------------------------------------------------------------- scoring
def calculate_scores(matrix, sample_mask, sample_weights=None):
    """Best scoring sample for the given mask: (column index, new_variant_count) or (None, None).

    Stateless like the reference: covered variants are recomputed from sample_mask == 0.  Scoring, masking,
    weighting and the first-maximum argmax all run on the device (utm_local_best); nothing is selected.  The
    greedy driver below does not call this per iteration (it keeps the whole loop on the device); it is the
    drop-in for callers that do.
    """
    sample_mask = np.asarray(sample_mask)
    matrix.set_state(sample_mask)
    matrix.set_weights(sample_weights)
    matrix.reset()
    score, use_sample, new_variant_count = matrix.local_best()
    # np.argmax runs over every sample and masked ones hold 0 (select.py:43-48): a best of 0, or a negative best
    # while some sample is masked, means "nothing to select"
    if use_sample < 0 or score == 0 or (score < 0 and (sample_mask != SELECTABLE).any()):
        return None, None
    return np.int64(use_sample), np.int64(new_variant_count)


def is_memsafe(shape, with_af=False):
    """Would a (variants, samples) block fit one HBM chunk under --maxmem?  (The reference asks this of host RAM,
    select.py:56-63; here it only decides how the variant axis is cut into chunks and never changes results.)"""
    gigabytes = (shape[0] * shape[1] / 8 + (shape[0] * 8 if with_af else 0)) / 1e9
    logging.debug("packed block of %d x %d: %.2f GB", shape[0], shape[1], gigabytes)
    return gigabytes < MAXMEM


def _depth_rows(matrix, rows, depth):
    """With depth > 1 every row gets a sixth field: the variants whose support has reached the depth after it (the
    device keeps that count per row)."""
    if depth > 1 and rows:
        done = matrix.stats()["iterations"]
        for row, saturated in zip(rows, matrix.at_depth(done - len(rows), len(rows))):
            row.append(int(saturated))
    return rows


def greedy_select(matrix, total_variant_count, select_count, vcf_samples, sample_mask, sample_weights=None, batch=64,
                  captured=0, depth=1):
    """Generator of [sample, var_count, new_count, tot_captured, pct_captured], one per selected sample.

    matrix               device.DeviceMatrix; when it holds one shard of a multi-GPU run its exchange must be set up
                         (sharded.connect_shards) -- every rank then yields the same rows
    total_variant_count  per-sample totals (var_count column)
    select_count         how many samples to select at most
    vcf_samples          sample names, aligned with sample_mask
    sample_mask          1 selectable / 0 used / 2 excluded; winners are set to 0 in place, like select.py:100
    sample_weights       optional float64 per sample
    captured             tot_captured of rows already written (the used samples of sample_mask, e.g. an --include prefix):
                         tot_captured / pct_captured go on from there
    depth                M: every variant counts until M selected samples carry it.  With M > 1 new_count is the units
                         gained, tot_captured = F = sum of min(support, M), pct_captured = F / (M * variants), and a
                         sixth field says how many variants have support >= M

    The loop itself runs on the device, `batch` iterations per call; it ends by itself when the best score is 0
    (no row for that iteration) or right after the row that captures the last variant.
    """
    n_variants = matrix.shape[0]
    if n_variants == 0:                         # nothing informative was loaded: a first pass would find only zeros
        logging.warning("No informative variants: nothing to select")
        return
    matrix.set_state(np.asarray(sample_mask))
    matrix.set_weights(sample_weights)
    if depth != getattr(matrix, "coverage_depth", 1):     # (depth 1 on a matrix that never left it: nothing to say)
        matrix.set_depth(depth)
    matrix.reset()
    units = n_variants * depth                  # what tot_captured can reach
    wanted = int(select_count)
    while wanted > 0:
        asked = min(batch, wanted)
        winners, gains, _ = matrix.run(asked)   # up to `asked` iterations, no host round trip in between
        rows = []
        for winner, gain in zip(winners, gains):
            captured += gain                    # stays np.int64: the ratio below is then numpy's division and rounding
            sample_mask[winner] = USED
            rows.append([vcf_samples[winner], int(total_variant_count[winner]), int(gain), int(captured),
                         round(captured / units, 4)])
        yield from _depth_rows(matrix, rows, depth)
        wanted -= len(winners)
        if len(winners) < asked:                # the device loop stopped on its own
            if captured >= units:
                logging.warning("Every variant is captured: stopping early")
            else:
                logging.warning("No selectable sample adds a variant any more: stopping early")
            return


# ---------------------------------------------------------------------------------------------- fixed orders
MODES = ("greedy", "topN", "random")


def fixed_order_rows(matrix, total_variant_count, order, vcf_samples, sample_mask, captured=0, depth=1):
    """Generator of greedy_select's five-field rows for the samples of `order` (indices), taken in that order whatever
    they score: one pass over their columns on the device (utm_apply_order), no scoring of anyone else.  The matrix is
    reset already (states and weights set); the rows go on from `captured`.  A sample that adds nothing still gets its
    row; the rows end after the one that captures the last variant.  Sets sample_mask[i] = USED as it goes and returns
    the running total."""
    units = matrix.shape[0] * depth
    if len(order) == 0:
        return captured
    gains = matrix.apply_order(order)
    rows = []
    for sample, gain in zip(order, gains):
        captured += gain                        # np.int64, as in greedy_select
        sample_mask[sample] = USED
        rows.append([vcf_samples[sample], int(total_variant_count[sample]), int(gain), int(captured),
                     round(captured / units, 4)])
    yield from _depth_rows(matrix, rows, depth)
    if len(gains) < len(order):
        logging.warning("Every variant is captured: stopping early")
    return captured


def topn_order(scores, states):
    """SVCollector's topN: the selectable samples by score, highest first, ties to the lower index (np.argmax's first
    maximum), cut before the first score that is <= 0.  `scores` = the scores of greedy's next iteration
    (matrix.peek_scores()), so topN is that iteration taken over and over without rescoring."""
    scores = np.asarray(scores, dtype=np.float64)
    candidates = np.flatnonzero(np.asarray(states) == SELECTABLE)
    ranked = candidates[np.argsort(-scores[candidates], kind="stable")]
    return ranked[:int((scores[ranked] > 0).sum())]     # (descending: the positive scores come first)


def random_order(states, seed=0):
    """SVCollector's random: a seeded permutation of the selectable samples."""
    candidates = np.flatnonzero(np.asarray(states) == SELECTABLE)
    return np.random.default_rng(seed).permutation(candidates)


def resolve_include(names, include, exclude):
    """--include names -> sample indices in the order given, later duplicates dropped.  Exits with status 1 on a name
    the input does not have or one that is excluded as well."""
    position = {name: i for i, name in enumerate(names)}
    banned = set(exclude or ())
    order = []
    for name in include or ():
        if name not in position:
            logging.error("--include: sample %s is not in the input", name)
            sys.exit(1)
        if name in banned:
            logging.error("--include: sample %s is excluded as well", name)
            sys.exit(1)
        if position[name] not in order:
            order.append(position[name])
    return np.asarray(order, dtype=np.int64)


def _ordered_selection(matrix, total_variant_count, rounds, names, states, vector, included, mode, seed, depth=1):
    """Rows of a selection that starts from a fixed prefix and / or fills up in a fixed order: the prefix (all of it),
    then what is left of `rounds` by `mode`."""
    n_variants = matrix.shape[0]
    if n_variants == 0:
        logging.warning("No informative variants: nothing to select")
        return
    matrix.set_state(states)
    matrix.set_weights(vector)
    if depth != getattr(matrix, "coverage_depth", 1):     # (depth 1 on a matrix that never left it: nothing to say)
        matrix.set_depth(depth)
    matrix.reset()
    captured = yield from fixed_order_rows(matrix, total_variant_count, included, names, states, depth=depth)
    left = rounds - len(included)
    if left <= 0 or captured >= n_variants * depth:
        return
    if mode == "greedy":        # the prefix is used now: greedy restarts from the mask and covers it again
        yield from greedy_select(matrix, total_variant_count, left, names, states, vector, captured=captured, depth=depth)
        return
    order = topn_order(matrix.peek_scores()[1], states) if mode == "topN" else random_order(states, seed)
    if len(order) < left:
        logging.warning("Only %d samples left to take in %s order", len(order), mode)
    yield from fixed_order_rows(matrix, total_variant_count, order[:left], names, states, captured, depth)


def _quota_selection(matrix, total_variant_count, rounds, names, states, vector, included, mode, seed, group_of, quota):
    """Rows of a selection in which no group (group_of: an id per sample, -1 = none) gets more than `quota` samples, the
    --include prefix counted: the greedy over the samples whose group is not full (the partition-matroid greedy).  The
    device loop runs for as many iterations as no group can fill in (groups.quota_run_length); then the rest of every full
    group is marked excluded and the loop restarts from the mask, as after an include prefix.  topN / random: the fixed
    order with the samples of a full group skipped."""
    from . import groups
    n_variants = matrix.shape[0]
    if n_variants == 0:
        logging.warning("No informative variants: nothing to select")
        return
    taken = groups.group_taken(group_of, int(group_of.max()) + 1, included)
    captured = 0
    if len(included):
        matrix.set_state(states)
        matrix.set_weights(vector)
        if getattr(matrix, "coverage_depth", 1) != 1:
            matrix.set_depth(1)
        matrix.reset()
        captured = yield from fixed_order_rows(matrix, total_variant_count, included, names, states)
    left = rounds - len(included)
    if left <= 0 or captured >= n_variants:
        return
    if mode != "greedy":
        if not len(included):
            matrix.set_state(states)
            matrix.set_weights(vector)
            if getattr(matrix, "coverage_depth", 1) != 1:
                matrix.set_depth(1)
            matrix.reset()
        order = topn_order(matrix.peek_scores()[1], states) if mode == "topN" else random_order(states, seed)
        order = groups.quota_filter(order, group_of, taken, quota, left)
        if len(order) < left:
            logging.warning("Only %d samples left to take in %s order under --group-max", len(order), mode)
        yield from fixed_order_rows(matrix, total_variant_count, order, names, states, captured)
        return
    position = {name: i for i, name in enumerate(names)}
    while left > 0:
        groups.close_full_groups(states, group_of, taken, quota)
        run = groups.quota_run_length(states, group_of, taken, quota, left)
        made = 0
        for row in greedy_select(matrix, total_variant_count, run, names, states, vector, captured=captured):
            made += 1
            captured = row[3]
            g = group_of[position[row[0]]]
            if g >= 0:
                taken[g] += 1
            yield row
        left -= made
        if made < run:                          # the device loop stopped on its own (and said why)
            return


# ---------------------------------------------------------------------------------------------- set-up
def resolve_select_count(n_samples, requested):
    """--count: negative = every sample; below 1 = that fraction of the samples, at least one; else a number of
    samples (so 1 means one sample, not 100 %) -- select.py:157-159."""
    if requested < 0:
        return n_samples
    if requested < 1:
        return max(1, int(n_samples * requested))
    return max(1, int(requested))


def sample_states(names, subset, exclude):
    """uint8 state per sample: everything selectable; with a subset only its members; excluded names never."""
    states = np.full(len(names), SELECTABLE, dtype=np.uint8)
    if subset:
        states[~np.isin(names, subset)] = EXCLUDED
    if exclude:
        states[np.isin(names, exclude)] = EXCLUDED
    return states


def weight_vector(names, weights):
    """float64 weight per sample from a {name: weight} mapping (unlisted samples weigh 1), or None."""
    if weights is None:
        return None
    vector = np.ones(len(names), dtype=np.float64)
    for position, name in enumerate(names):
        weight = weights.get(name)
        if weight is not None:
            vector[position] = weight
    return vector


def run_selection(data, select_count=0.02, subset=None, exclude=None, weights=None, include=None, mode="greedy", seed=0,
                  depth=1, group_of=None, group_max=None):
    """Prepare a selection over `data` ({"data": DeviceMatrix, "samples", "var_count"}) and return its row generator.
    include: names that come first, in that order, whatever they score (they count towards select_count); mode: how
    the rest is chosen -- greedy, or the fixed orders topN / random (seed); depth: how many selected samples should
    carry every variant (rows get a sixth field when it is above 1); group_of + group_max: a group id per sample (-1 =
    none) and the most samples any one group may contribute (--include samples count; depth 1 only)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth must be in 1..{MAX_DEPTH}")
    depth = int(depth)
    n_variants, n_samples = data["data"].shape
    logging.info("%d samples x %d informative variants", n_samples, n_variants)
    rounds = resolve_select_count(n_samples, select_count)
    logging.info("up to %d samples will be selected", rounds)
    names = np.asarray(data["samples"]).astype(str)
    states = sample_states(names, subset, exclude)
    if subset or exclude:
        logging.info("subset of %d names, %d names excluded: %d samples remain selectable",
                     len(subset or ()), len(exclude or ()), int((states == SELECTABLE).sum()))
    vector = weight_vector(names, weights)
    if vector is not None:
        logging.info("%d sample weights given", len(weights))
    if group_max is not None:
        if group_of is None or int(group_max) < 1 or depth != 1:
            raise ValueError("group_max needs group_of, a quota of at least 1 and depth 1")
        from . import groups
        group_of = np.asarray(group_of, dtype=np.int32)
        included = resolve_include(names, include, exclude)
        if (groups.group_taken(group_of, int(group_of.max()) + 1, included) > int(group_max)).any():
            logging.error("--include already holds more than --group-max %d samples of one group", int(group_max))
            sys.exit(1)
        return _quota_selection(data["data"], np.asarray(data["var_count"]), rounds, names, states, vector, included, mode, seed,
                                group_of, int(group_max))
    if not include and mode == "greedy":
        return greedy_select(data["data"], np.asarray(data["var_count"]), rounds, names, states, vector, depth=depth)
    included = resolve_include(names, include, exclude)
    logging.info("%d samples included first; the rest in %s order", len(included), mode)
    return _ordered_selection(data["data"], np.asarray(data["var_count"]), rounds, names, states, vector, included, mode, seed,
                              depth)


def refined_selection(data, select_count=0.02, subset=None, exclude=None, include=None, max_swaps=None, log=None):
    """select --refine: the greedy panel of run_selection, improved by 1-swaps (refine.refine: samples that were
    selectable and are not in the panel come in, the --include samples never leave), then the rows of the greedy order
    WITHIN the refined panel -- what run_selection(subset=panel names, select_count=len(panel)) gives, still a coverage
    curve.  The plain count only: no AF, weights or depth.  max_swaps: None = until no swap helps.  `log`, a list,
    receives refine's (swap, out, in, gain, tot_captured) entries."""
    from .refine import refine
    matrix = data["data"]
    names = np.asarray(data["samples"]).astype(str)
    position = {name: i for i, name in enumerate(names)}
    first = list(run_selection(data, select_count, subset, exclude, None, include))
    panel = [position[row[0]] for row in first]
    if not panel:
        return
    pinned = resolve_include(names, include, exclude) if include else ()
    panel, swaps = refine(matrix, panel, sample_states(names, subset, exclude), pinned, max_swaps)
    logging.info("refine: %d swaps, %d -> %d variants captured", len(swaps), first[-1][3], swaps[-1][4] if swaps else first[-1][3])
    if log is not None:
        log.extend(swaps)
    states = np.full(len(names), EXCLUDED, dtype=np.uint8)
    states[panel] = SELECTABLE
    yield from greedy_select(matrix, np.asarray(data["var_count"]), len(panel), names, states)


# ---------------------------------------------------------------------------------------------- ingest
def _read_part(path, dev=0, inflate="auto"):
    """One input file -> {'GT': packbits rows, 'AF': per-variant float64, 'samples'} (the reference's part dict).
    VCFs and BCFs are parsed on the run's GPU (vcfgpu.py); `inflate` says where BGZF is inflated."""
    if path.endswith((".vcf.gz", ".vcf", ".bcf")):
        from .vcfgpu import read_vcf
        try:
            return read_vcf(path, device=dev, inflate=inflate)
        except ValueError as err:
            logging.error("%s", err)
            sys.exit(1)
    if path.endswith(".jl"):
        import joblib  # the reference's own container (utmos/convert.py:98)
        return joblib.load(path)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {"GT": z["GT"], "AF": z["AF"], "samples": z["samples"]}
    logging.error("%s: unknown file type (expected .vcf, .vcf.gz, .bcf, .jl, .npz or a %s store)", path, STORE_SUFFIX)
    sys.exit(1)


def _shard_matrix(n_samples, dev, shard):
    """shard = (rank, world) or None: this process holds a contiguous block of the sample axis."""
    if shard is None or shard[1] == 1:
        return device.DeviceMatrix(n_samples, device=dev)
    from .sharded import shard_bounds
    first, n_local = shard_bounds(n_samples, *shard)
    return device.DeviceMatrix(n_samples, device=dev, first_sample=first, n_local=n_local)


def filter_loaded(matrix, variants, names, chunk_af, origin):
    """Apply the run's variant filters (variants = (variant_filter.Criteria, subset names, exclude names)) to the loaded
    matrix, before var_count is taken and the AF is set: one mask per chunk on the host, every column compacted on the
    GPU.  Returns the per-chunk masks (None: no filter is active); exits with status 1 when a criterion cannot be applied
    to this input or nothing is left."""
    if not variants or not variants[0].active:
        return None
    from . import variant_filter
    try:
        return variant_filter.apply(matrix, variants[0], names, variants[1], variants[2], chunk_af, origin)
    except variant_filter.FilterError as err:
        if hasattr(matrix, "close"):
            matrix.close()
        logging.error("%s", err)
        sys.exit(1)


def _cut_origin(origin, masks):
    """A store's origin arrays under the per-chunk masks."""
    keep = np.concatenate(masks) if masks else np.zeros(0, bool)
    return {"part": origin["part"][keep], "row": origin["row"][keep], "af": None if origin["af"] is None else origin["af"][keep]}


def load_store(path, dev=0, shard=None, origin=False, variants=None):
    """Open a packed store and upload this process's columns, chunk by chunk, from a memory map.  origin: also return
    where every variant came from (store_origin).  variants: the run's variant filters (filter_loaded)."""
    try:
        reader = StoreReader(path)
    except (OSError, ValueError) as err:
        logging.error("%s", err)
        sys.exit(1)
    matrix = _shard_matrix(reader.n_samples, dev, shard)
    lo, n_local = matrix.first_sample, matrix.n_local
    for k, n_var in enumerate(reader.chunk_vars):
        chunk = matrix.add_chunk(n_var)
        matrix.upload_columns(chunk, reader.columns(k, lo, n_local))
    chunk_af = [np.asarray(reader.af(k)) for k in range(len(reader.chunk_vars))] if reader.has_af else None
    var_count = reader.var_count[lo:lo + n_local]
    where = store_origin(matrix.shape[0], chunk_af) if origin or variants else None
    masks = filter_loaded(matrix, variants, reader.samples, chunk_af, where)
    if masks is not None:               # the kept rows' var_count, taken like the store's own: before AF == 0 rows are cleared
        var_count = matrix.var_count()
        chunk_af = None if chunk_af is None else [af[mask] for af, mask in zip(chunk_af, masks)]
        where = _cut_origin(where, masks)
    if reader.has_af:
        for chunk, af in enumerate(chunk_af):
            matrix.set_af(chunk, af)
    data = {"samples": reader.samples, "data": matrix, "var_count": var_count, "has_af": reader.has_af}
    if origin:
        data["origin"] = where
    return data


class _ChunkBuilder:
    """Collects consecutive input parts until they make one HBM chunk (every chunk costs its own launches in every
    iteration, so a run over many input files should not end up with one small chunk per file), uploads it, and --
    with a store being written -- streams it to disk at once, so the host never holds more than one chunk."""

    def __init__(self, matrix, writer, calc_af, af_as_f32):
        self.matrix, self.writer, self.calc_af, self.af_as_f32 = matrix, writer, calc_af, af_as_f32
        self.rows, self.af = [], []
        self.chunk_af = []                       # per flushed chunk, kept only while no AF could be set yet
        self.origin, self.chunk_origin = [], []  # (part, row) of every variant held / flushed: only when asked for (add)

    def held_variants(self):
        return sum(len(r) for r in self.rows)

    def add(self, rows, af, origin=None):
        self.rows.append(rows)
        self.af.append(af)
        if origin is not None:
            self.origin.append(origin)

    def flush(self):
        if not self.rows:
            return
        rows = self.rows[0] if len(self.rows) == 1 else np.concatenate(self.rows)
        af = self.af[0] if len(self.af) == 1 else np.concatenate(self.af)
        self.rows, self.af = [], []
        if self.origin:
            self.chunk_origin.append(self.origin[0] if len(self.origin) == 1 else np.concatenate(self.origin))
            self.origin = []
        chunk = self.matrix.add_chunk(len(rows))
        self.matrix.upload_rows_packed(chunk, rows)          # bit transpose to columns happens on the GPU
        if self.writer is not None and hasattr(self.writer, "add_rows"):      # hdf5: the packed rows themselves
            self.writer.add_rows(rows, af.astype(np.float32) if self.calc_af else None)
        elif self.writer is not None:
            self.writer.add_chunk(len(rows), self.matrix.download_columns(chunk), af.astype(np.float32) if self.calc_af else None)
        self.chunk_af.append(af)


def _place_part(builder, rows, af, n_samples, calc_af, buffer, origin=None):
    """Hand one part's packed rows to the chunk builder: parts are merged while the chunk stays within --maxmem; a part
    too large for one chunk is cut into the largest pieces that fit; `buffer` variants per chunk only when chunking is
    forced (--maxmem 0): chunks are HBM allocations here, not the I/O granularity they are for the reference's hdf5
    appends.  origin: int64 (len(rows), 2), the (part, row) each variant came from; it is merged and cut with the rows."""
    if MAXMEM != 0 and is_memsafe((len(rows), n_samples), calc_af):
        if builder.held_variants() and not is_memsafe((builder.held_variants() + len(rows), n_samples), calc_af):
            builder.flush()
        builder.add(rows, af, origin)
        return
    builder.flush()
    if MAXMEM != 0:
        per_variant = n_samples / 8 + (8 if calc_af else 0)
        step = max(64, int(MAXMEM * 1e9 / per_variant) // 64 * 64 - 64)
    else:
        step = max(64, buffer // 64 * 64)
    for lo in range(0, len(rows), step):
        builder.add(rows[lo:lo + step], af[lo:lo + step], None if origin is None else origin[lo:lo + step])
        builder.flush()


def part_origin(part, informative):
    """int64 (k, 2): for the k informative records of input file number `part`, that number and the record's 0-based
    position in the file (before the records nobody carries were dropped)."""
    rows = np.flatnonzero(informative).astype(np.int64)
    return np.stack([np.full(len(rows), part, dtype=np.int64), rows], axis=1)


def chunks_origin(chunk_origin, chunk_af):
    """The builder's per-chunk origins and AF values -> {"part": int32, "row": int64, "af"} in matrix order."""
    pairs = np.concatenate(chunk_origin) if chunk_origin else np.zeros((0, 2), np.int64)
    af = np.concatenate(chunk_af) if chunk_af else np.zeros(0, np.float64)
    return {"part": pairs[:, 0].astype(np.int32), "row": pairs[:, 1].copy(), "af": af}


def store_origin(n_variants, chunk_af=None):
    """A .utm or .hdf5 store is one input whose rows are the matrix's: part 0, row = the position in the store."""
    af = None if chunk_af is None else (np.concatenate(chunk_af) if len(chunk_af) else np.zeros(0, np.float32))
    return {"part": np.zeros(n_variants, np.int32), "row": np.arange(n_variants, dtype=np.int64), "af": af}


def load_h5(path, dev=0, shard=None, buffer=32768, origin=False, variants=None):
    """Read the reference's `--lowmem` HDF5 store (h5store.py): its `data` chunks are LZF-decoded and packed on the GPU
    and go through the same chunk builder and upload as the rows of part files.  Unlike part files, all-zero rows stay
    (the reference's variant total is data.shape[0]) and var_count comes from the file (in an AF store a carrier whose
    AF is 0 holds 0)."""
    from .h5store import ChunkDecoder, H5Store
    try:
        store = H5Store(path)
    except (OSError, ValueError) as err:
        logging.error("%s", err)
        sys.exit(1)
    n_var, n_samples = store.data.shape
    has_af = store.data.kind == "float"
    logging.info("%s: hdf5 store of %d x %d %s cells in %d chunks", path, n_var, n_samples, store.data.dtype,
                 len(store.data.chunks))
    matrix = _shard_matrix(n_samples, dev, shard)
    builder = _ChunkBuilder(matrix, None, has_af, True)
    try:
        with ChunkDecoder(store, dev) as decoder:
            for _first, rows, af in decoder:
                _place_part(builder, rows, af if has_af else np.zeros(len(rows), np.float32), n_samples, has_af, buffer)
            builder.flush()
            logging.debug("hdf5 decode (ms): %s", decoder.timing())
    except ValueError as err:
        matrix.close()
        logging.error("%s", err)
        sys.exit(1)
    lo, n_local = matrix.first_sample, matrix.n_local
    var_count = store.var_count[lo:lo + n_local]
    chunk_af = [np.asarray(af, dtype=np.float32) for af in builder.chunk_af] if has_af else None
    where = store_origin(matrix.shape[0], chunk_af) if origin or variants else None
    masks = filter_loaded(matrix, variants, store.samples, chunk_af, where)
    if masks is not None:
        var_count = matrix.var_count()
        chunk_af = None if chunk_af is None else [af[mask] for af, mask in zip(chunk_af, masks)]
        where = _cut_origin(where, masks)
    if has_af:
        for chunk, af in enumerate(chunk_af):
            matrix.set_af(chunk, af)
    data = {"samples": store.samples, "data": matrix, "var_count": var_count, "has_af": has_af}
    if origin:
        data["origin"] = where
    return data


def load_files(in_files, lowmem=None, buffer=32768, calc_af=False, dev=0, shard=None, inflate="auto", origin=False, variants=None):
    """Load and concatenate the inputs into one HBM-resident matrix -> {"samples", "data", "var_count", "has_af"}.

    lowmem == 1: in_files[0] is an existing packed store.  lowmem == path: the store is (re)created there while
    loading (a .hdf5 path: the reference's own store, its chunks LZF-encoded on the GPU, h5write.py); like the reference's hdf5 it keeps AF as float32, so `--lowmem` + `--af` scores with float32 AF values
    (answer_key/select_af_h5.txt) and the plain path with float64 (select_af.txt).  `buffer` = variants per chunk
    when chunking is forced (--maxmem 0).  origin=True adds the key "origin": per informative variant, in matrix order,
    {"part": index into in_files, "row": record number inside that file, "af": its AF or None} (select --variants-out).
    variants = (variant_filter.Criteria, subset names, exclude names): the matrix is cut down to the variants that pass
    (filter_loaded) right after loading -- var_count, the AF and the origin arrays then describe the kept variants only.
    """
    logging.info("reading %d input file(s)", len(in_files))
    if lowmem == 1:
        if in_files[0].endswith(H5_SUFFIX):
            return load_h5(in_files[0], dev, shard, buffer, origin, variants)
        return load_store(in_files[0], dev, shard, origin, variants)
    if shard is not None and shard[1] > 1 and lowmem is not None:
        logging.error("Create the matrix store with a single process, then select from it with several")
        sys.exit(1)

    samples = matrix = builder = writer = None
    for number, path in enumerate(in_files, start=1):
        part = _read_part(path, dev, inflate)
        if samples is None:
            samples = np.asarray(part["samples"]).astype("U")
            matrix = _shard_matrix(len(samples), dev, shard)
            if lowmem is not None and lowmem.endswith(H5_SUFFIX):
                from .h5write import H5Writer
                writer = H5Writer(lowmem, samples, calc_af, "gpu", dev)
            elif lowmem is not None:
                writer = StoreWriter(lowmem, samples, calc_af)
            builder = _ChunkBuilder(matrix, writer, calc_af, lowmem is not None)
        rows = np.ascontiguousarray(part["GT"], dtype=np.uint8)
        informative = rows.any(axis=1)              # a variant nobody carries has no set bit in any byte (select.py:276-279)
        logging.debug("%s: %d of %d variants carried by nobody, dropped", path, int((~informative).sum()), len(rows))
        rows = rows[informative]
        af = np.asarray(part["AF"], dtype=np.float64).reshape(-1)[informative]
        if len(rows) == 0:
            continue
        _place_part(builder, rows, af, len(samples), calc_af, buffer,
                    part_origin(number - 1, informative) if origin or variants else None)
        logging.debug("%d of %d files read", number, len(in_files))
    if builder is not None:
        builder.flush()
    if matrix is None:
        logging.error("No input files")
        sys.exit(1)

    masks = filter_loaded(matrix, variants, samples, builder.chunk_af,
                          chunks_origin(builder.chunk_origin, builder.chunk_af) if variants else None)
    if masks is not None:
        builder.chunk_af = [af[mask] for af, mask in zip(builder.chunk_af, masks)]
        builder.chunk_origin = [where[mask] for where, mask in zip(builder.chunk_origin, masks)]
    # var_count before AF == 0 rows are cleared, like select.py:281-284.  (A shard counts its own samples;
    # select_main gathers the shards' parts.)
    var_count = matrix.var_count() if matrix.chunk_vars else np.zeros(matrix.n_local, dtype=np.int64)
    if calc_af:
        for chunk, af in enumerate(builder.chunk_af):
            matrix.set_af(chunk, af.astype(np.float32) if lowmem is not None else af)
    if writer is not None:
        writer.finish(var_count)
    data = {"samples": samples, "data": matrix, "var_count": var_count, "has_af": bool(calc_af)}
    if origin:
        data["origin"] = chunks_origin(builder.chunk_origin, builder.chunk_af)
    return data


# ---------------------------------------------------------------------------------------------- command line
def parse_sample_lists(argument):
    """--subset / --exclude values: each item is a file of names (one per line) or a comma separated list."""
    names = []
    for item in argument or []:
        if os.path.exists(item):
            with open(item, "r") as fh:
                names += [line.strip() for line in fh]
        else:
            names += item.split(",")
    return names


def parse_weights(argument):
    """Tab-delimited `sample<TAB>weight` -> {sample: weight}."""
    if not argument:
        return None
    table = {}
    with open(argument, "r") as fh:
        for line in fh:
            if not line.strip():
                continue
            name, weight = line.rstrip("\n").split("\t")[:2]
            table[name] = float(weight)
    return table


def setup_logging(debug=False):
    logging.basicConfig(stream=sys.stderr, level=logging.DEBUG if debug else logging.INFO,
                        format="%(asctime)s [%(levelname)s] %(message)s", force=True)


def _build_parser():
    """The option surface of the reference's `utmos select` (flags, defaults and meaning: utmos/select.py:355-398),
    plus this build's --device / --brute-force / --exchange."""
    parser = argparse.ArgumentParser(prog="select", description="Select the fewest samples that capture the most variants (MI355X).")
    parser.add_argument("in_files", nargs="*", type=str, help="inputs: .vcf[.gz], .bcf, .jl, .npz parts, or one packed .utm or .hdf5 store")
    parser.add_argument("-c", "--count", type=float, default=0.02,
                        help="how many samples: a fraction of all if < 1, a count if >= 1, every sample if -1 [%(default)s]")
    parser.add_argument("-o", "--out", type=str, default="/dev/stdout", help="TSV destination [stdout]")
    parser.add_argument("--debug", action="store_true", help="debug-level logging")
    parser.add_argument("--variants-out", type=str, default=None, metavar="FILE.npz",
                        help="also write, per informative variant, the row at which it was captured (-1: never), with "
                             "the input file and record it came from (numpy .npz)")
    parser.add_argument("--samples-out", type=str, default=None, metavar="FILE.npz",
                        help="also write, for EVERY sample of the inputs, how many of its own variants each row captured "
                             "(new, n x k), how many no row did (missed) and how many it carries (total), with samples and "
                             "panel (numpy .npz)")
    parser.add_argument("--represent-out", type=str, default=None, metavar="FILE.tsv",
                        help="also write, per row, how well the panel so far holds the samples outside it: n_outside, and "
                             "the mean, median and minimum share of a sample's own variants captured")
    scoring = parser.add_argument_group("Scoring Arguments")
    scoring.add_argument("--af", action="store_true", help="score variants by allele frequency instead of 1")
    scoring.add_argument("--weights", type=str, default=None, help="two-column TSV: sample, weight")
    scoring.add_argument("--subset", type=str, default=None, action="append",
                         help="only consider these samples (file or comma list; repeatable)")
    scoring.add_argument("--exclude", type=str, default=None, action="append",
                         help="never select these samples (file or comma list; repeatable)")
    scoring.add_argument("--include", type=str, default=None, action="append",
                         help="select these samples first, in the order given, whatever they score (file or comma "
                              "list; repeatable); they count towards --count")
    scoring.add_argument("--mode", choices=list(MODES), default="greedy",
                         help="how samples are chosen: greedy re-scores after every pick; topN takes the best first-"
                              "iteration scores in order; random takes a seeded permutation [%(default)s]")
    scoring.add_argument("--seed", type=int, default=0, help="seed of --mode random [%(default)s]")
    scoring.add_argument("--refine", type=int, default=0, metavar="N",
                         help="after the greedy selection, improve the panel by up to N 1-swaps (one selected sample "
                              "for one unselected, whenever that captures more variants); -1 = until no swap helps; "
                              "the TSV is then the greedy order within the refined panel [%(default)s: off]")
    scoring.add_argument("--refine-out", type=str, default=None, metavar="FILE.tsv",
                         help="with --refine: write the swaps made (swap, out, in, gain, tot_captured)")
    scoring.add_argument("--groups", type=str, default=None, metavar="FILE",
                         help="two-column TSV: sample, group (a population label; at most 64 groups)")
    scoring.add_argument("--groups-out", type=str, default=None, metavar="FILE.tsv",
                         help="with --groups: write, per row of the selection and group, what the row adds to the variants "
                              "that group carries and to those only that group carries")
    scoring.add_argument("--group-max", type=int, default=None, metavar="Q",
                         help="with --groups: select at most Q samples of any one group (--include samples count; "
                              "samples in no group are not limited)")
    scoring.add_argument("--depth", type=int, default=1,
                         help="every variant counts until this many selected samples carry it (1..255); above 1 "
                              "new_count / tot_captured count units of min(support, depth) and a column at_depth is "
                              "added [%(default)s]")
    stability = parser.add_argument_group("Stability Arguments")
    stability.add_argument("--replicates", type=int, default=None, metavar="B",
                           help="also run the greedy selection on B (1..256) random subsets of the variants, all at once, "
                                "with the run's count and --subset / --exclude (masks seeded by --seed)")
    stability.add_argument("--subsample", type=float, default=None, metavar="F",
                           help="with --replicates: the share of the variants every replicate keeps, 0 < F <= 1 [0.5]")
    stability.add_argument("--replicates-out", type=str, default=None, metavar="FILE.npz",
                           help="with --replicates: write every replicate's rows (order, new, kept, n_done), the band of the "
                                "coverage curves (pct_mean, pct_min, pct_max), samples, panel, seed and fraction (numpy .npz)")
    stability.add_argument("--stability-out", type=str, default=None, metavar="FILE.tsv",
                           help="with --replicates: write, per sample that a replicate or the run selected, in how many "
                                "replicates (selected, frequency), at which mean row (mean_rank) and whether the run did (in_panel)")
    quality = parser.add_argument_group("Bound Arguments")
    quality.add_argument("--bound-out", type=str, default=None, metavar="FILE.tsv",
                         help="also write a certified upper bound on what ANY panel of the same size can capture (k, captured, "
                              "bound_trivial, bound_online, bound_lagrange, bound, share): the panel captures at least `share` "
                              "of the best possible one.  --include samples are part of every panel compared with; with "
                              "--group-max the bound is for the problem without the quota, which is still a bound")
    quality.add_argument("--bound-iters", type=int, default=None, metavar="T",
                         help="with --bound-out: subgradient steps of the Lagrangian bound, 1..65535 [200]")
    quality.add_argument("--bound-at", type=str, default=None, metavar="K[,K...]",
                         help="with --bound-out: the panel sizes to bound [the number of rows the run produced]")
    from . import variant_filter
    variant_filter.add_arguments(parser)
    memory = parser.add_argument_group("Memory Arguments")
    memory.add_argument("--lowmem", type=str, default=None,
                        help="matrix store to write while loading the inputs (.utm, or the reference's .hdf5), or to "
                             "read when no inputs are given")
    memory.add_argument("--buffer", type=int, default=32768, help="variants per HBM chunk when chunking is on [%(default)s]")
    memory.add_argument("--maxmem", type=int, default=2, help="GB one chunk may take; 0 = always chunk [%(default)s]")
    gpu = parser.add_argument_group("GPU Arguments")
    gpu.add_argument("--device", type=int, default=None, help="GPU index [0; LOCAL_RANK when launched one process per GPU]")
    gpu.add_argument("--brute-force", action="store_true",
                     help="re-score every sample from scratch in every iteration (default: later iterations only "
                          "subtract what the last winner newly captured; identical output)")
    gpu.add_argument("--exchange", choices=["auto", "mailboxes", "rccl", "rccl-allreduce"], default="auto",
                     help="several processes: how the shards meet every iteration [auto: device mailboxes, else RCCL]")
    gpu.add_argument("--inflate", choices=["auto", "gpu", "host"], default="auto",
                     help="where BGZF (.vcf.gz from bgzip, .bcf) input is inflated: on the GPU (auto, gpu) or by host "
                          "threads (host); gpu refuses gzip that is not BGZF [%(default)s]")
    return parser


def parse_args(args):
    """Parse and validate the command line; exits with status 1 on unusable input combinations (select.py:401-415)."""
    args = _build_parser().parse_args(args)
    setup_logging(args.debug)
    stores = [name for name in args.in_files if name.endswith((STORE_SUFFIX, H5_SUFFIX))]
    if stores and len(args.in_files) > 1:
        logging.error("A matrix store cannot be combined with other input files")
        sys.exit(1)
    if not 1 <= args.depth <= MAX_DEPTH:
        logging.error("--depth must be between 1 and %d", MAX_DEPTH)
        sys.exit(1)
    if args.refine < -1:
        logging.error("--refine takes a number of swaps, or -1 for as many as help")
        sys.exit(1)
    if args.refine_out and not args.refine:
        logging.error("--refine-out needs --refine")
        sys.exit(1)
    if args.refine:                              # 1-swaps are judged by the plain count of captured variants
        clash = ("--af" if args.af else "--weights" if args.weights else "--depth above 1" if args.depth > 1 else
                 f"--mode {args.mode}" if args.mode != "greedy" else None)
        if clash:
            logging.error("--refine improves the plain number of captured variants and cannot be combined with %s", clash)
            sys.exit(1)
    from . import bound
    bound.refuse(args)
    if (args.groups_out or args.group_max is not None) and not args.groups:
        logging.error("--groups-out and --group-max need --groups")
        sys.exit(1)
    if args.group_max is not None and args.group_max < 1:
        logging.error("--group-max must be at least 1")
        sys.exit(1)
    if args.groups and (args.depth > 1 or args.refine):   # open: DESIGN.md section 15
        logging.error("--groups cannot be combined with %s", "--depth above 1" if args.depth > 1 else "--refine")
        sys.exit(1)
    if args.replicates is None:
        given = ("--replicates-out" if args.replicates_out else "--stability-out" if args.stability_out else
                 "--subsample" if args.subsample is not None else None)
        if given:
            logging.error("%s needs --replicates", given)
            sys.exit(1)
    else:                                        # the replicates restate the plain greedy run over fewer variants
        from .stability import MAX_REPLICATES
        if not 1 <= args.replicates <= MAX_REPLICATES:
            logging.error("--replicates must be between 1 and %d", MAX_REPLICATES)
            sys.exit(1)
        if args.subsample is not None and not 0.0 < args.subsample <= 1.0:
            logging.error("--subsample must be above 0 and at most 1")
            sys.exit(1)
        clash = ("--af" if args.af else "--weights" if args.weights else "--depth above 1" if args.depth > 1 else
                 f"--mode {args.mode}" if args.mode != "greedy" else "--refine" if args.refine else
                 "--groups" if args.groups else "--include" if args.include else None)
        if clash:
            logging.error("--replicates runs the plain greedy selection on subsets of the variants and cannot be combined with %s", clash)
            sys.exit(1)
    if (args.samples_out or args.represent_out) and args.count >= 1 and int(args.count) > MAX_PANEL:
        logging.error("--samples-out and --represent-out hold a panel of at most %d rows (-c %d asks for more)", MAX_PANEL, int(args.count))
        sys.exit(1)
    if not args.in_files and not args.lowmem:
        logging.error("Nothing to read: give input files, or --lowmem STORE to select from an existing store")
        sys.exit(1)
    if not args.in_files:                        # --lowmem STORE alone: select from the existing store
        args.in_files, args.lowmem = [args.lowmem], 1
    elif stores and not args.lowmem:
        logging.info("Input is a matrix store: reading it directly")
        args.lowmem = 1
    filters = ("min_af", "max_af", "min_carriers", "max_carriers", "keep_variants", "drop_variants")
    if args.lowmem not in (None, 1) and any(getattr(args, name) is not None for name in filters):
        logging.error("The variant filters cannot be combined with writing a --lowmem store: the store holds every variant. "
                      "Write the store first, or write a filtered one with `filter -o`")
        sys.exit(1)
    options = {name: value for name, value in vars(args).items()
               if (name not in ("variants_out", "samples_out", "represent_out", "groups", "groups_out", "group_max", "replicates", "subsample",
                                "replicates_out", "stability_out", "bound_out", "bound_iters", "bound_at") + filters or value is not None)
               and (name not in ("refine", "refine_out") or value)}
    logging.info("options in effect: %s", json.dumps(options, sort_keys=True))
    return args


def _gather_var_count(transport, local_counts, n_samples):
    """Every sample's var_count for the output rows: each shard popcounted its own columns on its GPU."""
    from .sharded import shard_bounds
    width = (n_samples + transport.world - 1) // transport.world      # shards differ by at most one sample
    padded = np.full(width, -1, dtype=np.int64)
    padded[:len(local_counts)] = local_counts
    parts = transport.allgather_bytes(padded.tobytes())
    return np.concatenate([np.frombuffer(blob, dtype=np.int64)[:shard_bounds(n_samples, rank, transport.world)[1]]
                           for rank, blob in enumerate(parts)])


def capture_ranks(matrix, order, depth=1):
    """int32 per variant of the whole matrix (chunks in order): the position in `order` at which `depth` of those samples
    carry it, -1 if never (utm_capture_rank, one pass per chunk)."""
    ranks = [matrix.capture_rank(chunk, order, depth) for chunk in range(len(matrix.chunk_vars))]
    return np.concatenate(ranks) if ranks else np.zeros(0, np.int32)


def selected_order(data, selected):
    """The global sample indices of the selected names, in row order."""
    position = {str(name): i for i, name in enumerate(data["samples"])}
    return np.asarray([position[name] for name in selected], dtype=np.int64)


def write_variants(path, data, selected, depth, in_files, ranks=None):
    """select --variants-out: the capture rank of every informative variant under the selected samples in row order, and
    where the variant came from (data["origin"], load_files(origin=True)); numpy.savez.  ranks: the per-chunk ranks at
    `depth`, when the caller has them already."""
    names = [str(name) for name in data["samples"]]
    position = {name: i for i, name in enumerate(names)}
    order = np.asarray([position[name] for name in selected], dtype=np.int64)
    origin = data["origin"]
    arrays = {"rank": capture_ranks(data["data"], order, depth) if ranks is None else
              (np.concatenate(ranks) if ranks else np.zeros(0, np.int32))}
    if depth > 1:
        arrays["first_rank"] = capture_ranks(data["data"], order, 1)
    arrays["part"], arrays["row"] = origin["part"], origin["row"]
    if origin["af"] is not None:
        arrays["af"] = origin["af"]
    arrays["samples"] = np.asarray(selected, dtype=str)
    arrays["files"] = np.asarray([str(name) for name in in_files], dtype=str)
    arrays["depth"] = np.int32(depth)
    np.savez(path, **arrays)
    logging.info("%s: capture ranks of %d variants under %d selected samples", path, len(arrays["rank"]), len(selected))


def refuse_af_store(args):
    """--replicates on a store made with --af: refused from the store's header, before anything is loaded."""
    if args.lowmem != 1 or not os.path.exists(args.in_files[0]):
        return
    try:
        if args.in_files[0].endswith(H5_SUFFIX):
            from .h5store import H5Store
            has_af = H5Store(args.in_files[0]).data.kind == "float"
        else:
            has_af = StoreReader(args.in_files[0]).has_af
    except (OSError, ValueError) as err:
        logging.error("%s", err)
        sys.exit(1)
    if has_af:
        logging.error("--replicates counts variants and cannot run on a store made with --af: recreate it without --af")
        sys.exit(1)


def select_main(cmdargs):
    """`utmos select`: load, select, write the TSV (header + one flushed line per selected sample, select.py:440-446)."""
    global MAXMEM
    args = parse_args(cmdargs)
    MAXMEM = args.maxmem
    ordered = bool(args.include) or args.mode != "greedy"
    if ordered and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--include and --mode %s need the whole sample axis on one GPU: run a single process", args.mode)
        sys.exit(1)
    if args.depth > 1 and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--depth above 1 needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.variants_out and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--variants-out needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if (args.samples_out or args.represent_out) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--samples-out and --represent-out need the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.refine and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--refine needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.groups and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        logging.error("--groups needs the whole sample axis on one GPU: run a single process")
        sys.exit(1)
    if args.replicates is not None:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            logging.error("--replicates needs the whole sample axis on one GPU: run a single process")
            sys.exit(1)
        refuse_af_store(args)
    from . import bound, variant_filter
    bound.refuse_several_processes(args)
    if args.bound_out:
        bound.refuse_small_sizes(bound.parse_bound_at(args.bound_at), len(dict.fromkeys(parse_sample_lists(args.include))))
    criteria = variant_filter.Criteria.from_args(args)
    variant_filter.refuse_several_processes(criteria)
    lists = [path for path in (args.keep_variants, args.drop_variants) if path]
    missing = [path for path in args.in_files + ([args.groups] if args.groups else []) + lists if not os.path.exists(path)]
    if missing:
        logging.error("Input %s does not exist", missing[0])
        sys.exit(1)

    # one process per GPU (torchrun-style RANK / WORLD_SIZE / LOCAL_RANK): each holds a block of the samples
    from .sharded import bootstrap, connect_shards, dist_env
    rank, world, local_rank = dist_env()
    if args.device is not None:
        dev = args.device
    else:   # one GPU per rank on a full node (ranks share devices only on smaller test boxes)
        dev = local_rank % device.nat.device_count() if world > 1 else 0
    subset = parse_sample_lists(args.subset)
    exclude = parse_sample_lists(args.exclude)
    data = load_files(args.in_files, args.lowmem, args.buffer, args.af, dev, (rank, world) if world > 1 else None,
                      args.inflate, **({"origin": True} if args.variants_out else {}),
                      **({"variants": (criteria, subset, exclude)} if criteria.active else {}))
    matrix = data["data"]
    per_sample = args.samples_out or args.represent_out
    if per_sample and args.count < 1 and len(data["samples"]) > MAX_PANEL:    # (a share of the samples, or all of them)
        wanted = len(data["samples"]) if args.count < 0 else int(len(data["samples"]) * args.count)
        if wanted > MAX_PANEL:
            logging.error("--samples-out and --represent-out hold a panel of at most %d rows (-c %s of %d samples asks for %d)",
                          MAX_PANEL, args.count, len(data["samples"]), wanted)
            matrix.close()
            sys.exit(1)
    if not args.brute_force:
        matrix.set_decremental(True)            # exact; same rows (DESIGN.md "Decremental scoring")
    matrix.set_af_exact_scores(False)           # the TSV has no score column: only ambiguous argmaxes need their chains
    if not data["has_af"] and args.af:
        logging.critical("The store was created without --af: remove --af or recreate it")
        sys.exit(1)
    if data["has_af"] and not args.af:
        logging.critical("The store was created with --af and scores by allele frequency: add --af or recreate it")
        if args.refine:
            logging.error("--refine improves the plain number of captured variants and cannot run on a store made with --af")
            sys.exit(1)
        if args.bound_out:
            logging.error("--bound-out bounds the plain number of captured variants and cannot run on a store made with --af")
            sys.exit(1)

    transport = None
    if world > 1:
        transport, uid = bootstrap(rank, world, device.DeviceMatrix.comm_unique_id)
        data["var_count"] = _gather_var_count(transport, data["var_count"], len(data["samples"]))
        try:
            how = connect_shards(matrix, transport, uid, os.environ.get("UTMOS_EXCHANGE", args.exchange))
        except RuntimeError as err:
            logging.critical("%s", err)
            sys.exit(1)
        logging.info("rank %d of %d: per-iteration exchange through %s", rank, world, how)
        if rank != 0:
            args.out = os.devnull

    weights = parse_weights(args.weights)
    group_of = group_names = None
    if args.groups:
        from . import groups
        group_of, group_names = groups.parse_groups(args.groups, data["samples"])
    try:
        with open(args.out, "w") as fout:
            fout.write(HEADER_DEPTH if args.depth > 1 else HEADER)
            swaps = []
            if args.refine:
                rows = refined_selection(data, args.count, subset, exclude, parse_sample_lists(args.include),
                                         None if args.refine < 0 else args.refine, swaps)
            elif args.group_max is not None:
                rows = run_selection(data, args.count, subset, exclude, weights, parse_sample_lists(args.include), args.mode,
                                     args.seed, group_of=group_of, group_max=args.group_max)
            elif ordered:
                rows = run_selection(data, args.count, subset, exclude, weights, parse_sample_lists(args.include), args.mode,
                                     args.seed, args.depth)
            else:
                rows = run_selection(data, args.count, subset, exclude, weights, depth=args.depth)
            selected = []
            for row in rows:
                logging.info("%s selected: %.1f%% of the variants captured", row[0], row[4] * 100)
                fout.write("\t".join(str(field) for field in row) + "\n")
                fout.flush()
                selected.append(row[0])
        if args.refine_out:
            from .refine import write_log
            write_log(args.refine_out, swaps, [str(name) for name in data["samples"]])
        if args.groups_out:
            groups.write_group_curve(args.groups_out, data, selected, group_of, group_names)
        if args.replicates is not None:          # stateless on the matrix as loaded (and filtered): the run's count and states
            from . import stability
            names = np.asarray(data["samples"]).astype(str)
            fraction = 0.5 if args.subsample is None else args.subsample
            result = stability.run_replicates(matrix, resolve_select_count(len(names), args.count), sample_states(names, subset, exclude),
                                              args.replicates, fraction, args.seed)
            panel = selected_order(data, selected)
            if args.replicates_out:
                stability.write_replicates(args.replicates_out, result, names, panel, args.seed, fraction)
            if args.stability_out:
                stability.write_table(args.stability_out, stability.selection_table(result[0], result[3], names, panel))
        if args.bound_out:                       # stateless on the matrix as loaded (and filtered)
            names = np.asarray(data["samples"]).astype(str)
            include = parse_sample_lists(args.include)
            bound.write_outputs(args.bound_out, data, selected, bound.parse_bound_at(args.bound_at), sample_states(names, subset, exclude),
                                resolve_include(names, include, exclude) if include else (), args.bound_iters or 200)
        ranks = None
        if args.variants_out and per_sample:     # both read the capture ranks of the printed order: one pass per chunk
            order = selected_order(data, selected)
            ranks = [matrix.capture_rank(chunk, order, args.depth) for chunk in range(len(matrix.chunk_vars))]
        if args.variants_out:
            write_variants(args.variants_out, data, selected, args.depth, args.in_files, ranks)
        if per_sample:
            from . import samples
            samples.write_outputs(args.samples_out, args.represent_out, data, selected, args.depth, ranks)
    finally:
        if transport is not None:
            # nobody unmaps or frees its columns while a peer's last launches may still read them
            try:
                transport.barrier()
            except OSError:
                pass
            transport.close()
        matrix.close()
    logging.info("utmos select finished")
