"""numpy restatement of the variant filters (what the filter tests compare with): the compaction by definition -- unpack
the columns to a dense boolean matrix, index its rows with the mask, pack again -- and the three criteria as masks."""
import numpy as np

from oracle_util import npo


def unpack_columns(cols, n_var):
    """uint64 (S, W) packed columns -> bool (n_var, S)."""
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    if cols.shape[1] == 0:
        return np.zeros((0, cols.shape[0]), dtype=bool)
    bits = np.unpackbits(cols.view(np.uint8), axis=1, bitorder="little")[:, :n_var]
    return bits.T.astype(bool)


def filter_columns(cols, n_var, keep, wp_out=None):
    """dense[keep] packed again with npo.pack_columns, zero padded to wp_out words per column -> (columns, kept count)."""
    keep = np.asarray(keep, dtype=bool)[:n_var]
    dense = unpack_columns(cols, n_var)[keep]
    kept = int(keep.sum())
    packed = npo.pack_columns(dense) if kept else np.zeros((cols.shape[0], 0), np.uint64)
    wp_out = packed.shape[1] if wp_out is None else int(wp_out)
    out = np.zeros((cols.shape[0], wp_out), dtype=np.uint64)
    out[:, :packed.shape[1]] = packed
    return out, kept


def pack_keep(keep, garbage=False):
    """bool per variant -> the keep words of the ABI; garbage: set every bit of the last word at or above n_var."""
    keep = np.asarray(keep, dtype=bool)
    words = np.zeros(max(1, (len(keep) + 63) // 64), dtype=np.uint64)
    packed = np.packbits(keep, bitorder="little")
    words.view(np.uint8)[:len(packed)] = packed
    if garbage and len(keep) % 64:
        words[-1] |= ~np.uint64(0) << np.uint64(len(keep) % 64)
    return words


# ----------------------------------------------------------------- the criteria
def af_keep(af, min_af=None, max_af=None):
    """X <= AF <= Y, every value taken exactly (python floats are float64; a float32 widens without rounding)."""
    lo = -np.inf if min_af is None else float(min_af)
    hi = np.inf if max_af is None else float(max_af)
    return np.array([lo <= float(a) <= hi for a in np.asarray(af)], dtype=bool)


def carrier_keep(dense, cohort, min_carriers=None, max_carriers=None):
    """A <= carriers among the cohort's columns <= B; dense: bool (N, S)."""
    counts = dense[:, np.asarray(cohort, dtype=np.int64)].sum(axis=1)
    lo = 0 if min_carriers is None else min_carriers
    hi = dense.shape[1] if max_carriers is None else max_carriers
    return (counts >= lo) & (counts <= hi)


def listed_keep(origin_part, origin_row, listed_part, listed_row):
    """True where (part, row) of a variant is in the list; KeyError for a listed pair the matrix does not have."""
    have = {(int(p), int(r)) for p, r in zip(origin_part, origin_row)}
    listed = {(int(p), int(r)) for p, r in zip(listed_part, listed_row)}
    if not listed <= have:
        raise KeyError(sorted(listed - have)[0])
    return np.array([(int(p), int(r)) in listed for p, r in zip(origin_part, origin_row)], dtype=bool)


# ----------------------------------------------------------------- the masks both compaction tests walk
SIZES = [1, 63, 64, 65, 8191, 8192, 8193, 32767, 32768, 32769, 100_003]   # one 1 KiB wave width and one 4 KiB tile +- 1 bit, several tiles


def mask_cases(n_var, seed=0):
    """{name: bool (n_var,)}: the masks the issue lists, those left out whose kept count the size cannot reach."""
    rng = np.random.default_rng(1000 + n_var + seed)
    cases = {"ones": np.ones(n_var, bool), "zeros": np.zeros(n_var, bool)}
    cases["first"] = np.arange(n_var) == 0
    cases["last"] = np.arange(n_var) == n_var - 1
    cases["alternating"] = np.arange(n_var) % 2 == 1
    for p in (0.03, 0.5, 0.97):
        cases[f"random{p}"] = rng.random(n_var) < p
    cases["alternating_words"] = (np.arange(n_var) // 64) % 2 == 1
    cases["every_shift"] = (np.arange(n_var) % 64) < ((np.arange(n_var) // 64) % 65)   # keep word k holds k mod 65 bits
    if n_var >= 200:
        exactly64 = np.zeros(n_var, bool)
        exactly64[rng.choice(n_var, 64, replace=False)] = True
        cases["kept64"] = exactly64
    if n_var > 8192:
        exactly = np.zeros(n_var, bool)
        exactly[rng.choice(n_var, 8192, replace=False)] = True
        cases["kept8192"] = exactly
    if n_var >= 8191:
        aligned = rng.random(n_var) < 0.5
        aligned[:5000] = False
        aligned[101:101 + 64 * 37] = True            # 2,368 kept bits end inside the first tile: the next piece starts a word
        cases["aligned_mid_tile"] = aligned
    return cases
