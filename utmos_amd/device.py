"""HBM-resident bit-packed presence matrix + the device-resident greedy loop (thin object layer
over the C ABI).  One DeviceMatrix = one GPU = one contiguous shard of the sample axis."""
import collections
import ctypes

import numpy as np

from . import _native as nat


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


BoundResult = collections.namedtuple("BoundResult", "hist bound best_iter n_live pass_ms lambdas")


class DeviceMatrix:
    """variants x samples presence matrix, column-major bitsets in HBM, split into chunks along
    the variant axis (the role the reference's row-chunked hdf5 plays, utmos/select.py:198-231)."""

    def __init__(self, n_samples, device=0, first_sample=0, n_local=None, profile_events=False,
                 af_sequential=False):
        self._h = ctypes.c_void_p()
        self.n_samples = int(n_samples)
        self.first_sample = int(first_sample)
        self.n_local = int(self.n_samples - self.first_sample if n_local is None else n_local)
        self.chunk_vars = []
        self.p2p = False
        self.fused = False      # run() is collective over the shards (mailboxes or RCCL)
        self.fused_mailboxes = False
        self.coverage_depth = 1
        flags = (nat.FLAG_PROFILE_EVENTS if profile_events else 0) | (nat.FLAG_AF_SEQUENTIAL if af_sequential else 0)
        code = nat.lib().utm_ctx_create(int(device), self.n_samples, self.first_sample, self.n_local, flags,
                                        ctypes.byref(self._h))
        if code != nat.UTM_OK:
            msg = nat.lib().utm_last_error().decode()
            if self._h:
                nat.lib().utm_ctx_destroy(self._h)
                self._h = ctypes.c_void_p()
            raise nat.NativeError(code, msg)

    # -- lifetime
    def close(self):
        if self._h:
            nat.lib().utm_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- shape, as the reference reads it (matrix.shape[0] / [1], select.py:89, :155)
    @property
    def shape(self):
        return (int(sum(self.chunk_vars)), self.n_samples)

    # -- matrix
    def add_chunk(self, n_var):
        idx = ctypes.c_int32(-1)
        nat.check(nat.lib().utm_add_chunk(self._h, int(n_var), ctypes.byref(idx)))
        self.chunk_vars.append(int(n_var))
        return idx.value

    def upload_columns(self, chunk, cols, first_col=0):
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        nat.check(nat.lib().utm_upload_columns(self._h, chunk, first_col, cols.shape[0], _ptr(cols), cols.shape[1]))

    def upload_rows_packed(self, chunk, rows, first_var=0):
        """rows: uint8 (n, >= ceil(S/8)), numpy.packbits(axis=1) order (utmos/convert.py:85)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        nat.check(nat.lib().utm_upload_rows_packed(self._h, chunk, int(first_var), rows.shape[0], _ptr(rows), rows.shape[1]))

    def download_columns(self, chunk, first_col=0, n_cols=None, out=None):
        """Columns [first_col, first_col + n_cols) of a chunk as uint64 (n_cols, ceil(n_var/64)); `out` = a C-contiguous
        array (or slice of whole rows of one) to fill instead of a new one -- large matrices come down in slices."""
        n_cols = self.n_local - first_col if n_cols is None else n_cols
        words = (self.chunk_vars[chunk] + 63) // 64
        if words == 0:                               # (a chunk filtered to nothing)
            return np.zeros((n_cols, 0), dtype=np.uint64) if out is None else out
        if out is None:
            out = np.empty((n_cols, words), dtype=np.uint64)
        elif out.dtype != np.uint64 or out.shape != (n_cols, words) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint64 array of shape (n_cols, words)")
        nat.check(nat.lib().utm_download_columns(self._h, chunk, first_col, n_cols, _ptr(out), words))
        return out

    def filter_variants(self, chunk, keep, pass_ms=False):
        """Keep only the variants of a chunk whose entry in `keep` (boolean, chunk_vars[chunk] entries) is true: every
        column is compacted on the device, the chunk's AF values with it, and the loop restarts (utm_filter_variants).
        Returns the kept count, which may be 0 (the chunk stays, empty); pass_ms: (count, HIP-event time) instead."""
        keep = np.asarray(keep)
        if keep.dtype != np.bool_ or keep.shape != (self.chunk_vars[chunk],):
            raise ValueError(f"keep must be a boolean array of {self.chunk_vars[chunk]} entries")
        words = np.zeros(max(1, (len(keep) + 63) // 64), dtype=np.uint64)
        packed = np.packbits(keep, bitorder="little")
        words.view(np.uint8)[:len(packed)] = packed
        kept, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
        nat.check(nat.lib().utm_filter_variants(self._h, int(chunk), _ptr(words), ctypes.byref(kept),
                                                ctypes.byref(ms) if pass_ms else None))
        self.chunk_vars[chunk] = int(kept.value)
        return (int(kept.value), ms.value) if pass_ms else int(kept.value)

    def var_count(self):
        out = np.zeros(self.n_local, dtype=np.int64)
        nat.check(nat.lib().utm_var_count(self._h, _ptr(out)))
        return out

    def synth_fill(self, chunk, seed=0, first_var_global=0):
        nat.check(nat.lib().utm_synth_fill(self._h, chunk, int(seed), int(first_var_global)))

    # -- options
    def set_state(self, state):
        st = np.ascontiguousarray(state, dtype=np.uint8)
        if st.shape != (self.n_samples,):
            raise ValueError(f"state must have {self.n_samples} entries")
        nat.check(nat.lib().utm_set_sample_state(self._h, _ptr(st)))

    def set_weights(self, weights):
        if weights is None:
            nat.check(nat.lib().utm_set_weights(self._h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (self.n_samples,):
            raise ValueError(f"weights must have {self.n_samples} entries")
        nat.check(nat.lib().utm_set_weights(self._h, _ptr(w)))

    def set_af(self, chunk, af):
        """af: float32 (hdf5 semantics) or float64 (in-memory semantics) per variant; None clears all."""
        if af is None:
            nat.check(nat.lib().utm_set_af(self._h, 0, nat.AF_NONE, None))
            return
        af = np.ascontiguousarray(af).reshape(-1)
        if af.dtype == np.float32:
            mode = nat.AF_F32
        elif af.dtype == np.float64:
            mode = nat.AF_F64
        else:
            raise TypeError("AF must be float32 or float64")
        if af.shape[0] != self.chunk_vars[chunk]:
            raise ValueError("AF length differs from the chunk's variant count")
        if af.shape[0] == 0:                         # (a chunk filtered to nothing: one value that is never read)
            af = np.zeros(1, dtype=af.dtype)
        nat.check(nat.lib().utm_set_af(self._h, chunk, mode, _ptr(af)))

    # -- loop
    def reset(self):
        nat.check(nat.lib().utm_reset(self._h))

    def step(self):
        """One greedy iteration.  (idx, new_count, score) or None for the reference's (None, None)."""
        i, n, s = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        nat.check(nat.lib().utm_step(self._h, ctypes.byref(i), ctypes.byref(n), ctypes.byref(s)))
        return None if i.value < 0 else (i.value, n.value, s.value)

    def run(self, k_max):
        k_max = int(k_max)
        idx = np.zeros(max(k_max, 1), dtype=np.int64)
        new = np.zeros(max(k_max, 1), dtype=np.int64)
        score = np.zeros(max(k_max, 1), dtype=np.float64)
        done = ctypes.c_int64(0)
        nat.check(nat.lib().utm_run(self._h, k_max, _ptr(idx), _ptr(new), _ptr(score), ctypes.byref(done)))
        n = done.value
        return idx[:n].copy(), new[:n].copy(), score[:n].copy()

    def apply_order(self, indices):
        """Select the given samples (global indices) in the given order in one pass over their columns; returns the
        new_count of each row made (fewer than listed when a row captured the last variant)."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        new = np.zeros(max(len(idx), 1), dtype=np.int64)
        done = ctypes.c_int64(0)
        nat.check(nat.lib().utm_apply_order(self._h, _ptr(idx), len(idx), _ptr(new), ctypes.byref(done)))
        return new[:done.value].copy()

    def capture_rank(self, chunk, indices, depth=1, pass_ms=False):
        """int32 per variant of a chunk: the position in `indices` (global sample indices, in order) at which `depth` of
        the listed samples carry the variant, -1 if that never happens.  Stateless: one pass over the listed columns,
        nothing of the selection is read or changed.  pass_ms: return (ranks, HIP-event time of the pass) instead."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        out = np.empty(self.chunk_vars[chunk], dtype=np.int32)
        ms = ctypes.c_double(0.0)
        nat.check(nat.lib().utm_capture_rank(self._h, int(chunk), _ptr(idx), len(idx), int(depth), _ptr(out),
                                             ctypes.byref(ms) if pass_ms else None))
        return (out, ms.value) if pass_ms else out

    def swap_gains(self, panel, pass_ms=False):
        """(gains, unique, new, base) of a panel (global sample indices): gains[i, t] = F(panel - panel[i] + t) - F(panel)
        for every sample t (int64, k x n_samples), unique[i] = the variants only member i carries, new[t] = the variants
        t carries and no member does, base = F(panel) = the variants some member carries.  Stateless: the columns are
        read, nothing of the selection is read or changed.  pass_ms: the HIP-event time of the launches as a fifth item."""
        idx = np.ascontiguousarray(panel, dtype=np.int64).reshape(-1)
        k = len(idx)
        gains = np.zeros((k, self.n_samples), dtype=np.int64)
        unique = np.zeros(k, dtype=np.int64)
        new = np.zeros(self.n_samples, dtype=np.int64)
        base, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        nat.check(nat.lib().utm_swap_gains(self._h, _ptr(idx), k, _ptr(gains), _ptr(unique), _ptr(new), ctypes.byref(base),
                                           ctypes.byref(ms) if pass_ms else None))
        return (gains, unique, new, base.value, ms.value) if pass_ms else (gains, unique, new, base.value)

    def multi_select(self, k, states, keep=None, seed=0, fraction=None, n_rep=None, pass_ms=False):
        """B greedy selections at once (utm_multi_select): replicate b runs over its own subset of the variants with its
        own sample states.  states: uint8 (B, n_samples), or (n_samples,) for every replicate alike (then n_rep says how
        many; default 1).  keep: a list with one boolean array (B, chunk_vars[chunk]) per chunk, or None for the hashed
        masks of `seed` that keep a share `fraction` of the variants (stability.keep_threshold; None = 1.0).  Returns
        (order int32 (B, k), -1 after a replicate's last row; new int64 (B, k); kept int64 (B,); n_done int64 (B,)), with
        pass_ms the HIP-event time of the launches as a fifth item.  Stateless: nothing of the selection is read or changed."""
        from .stability import keep_threshold
        k = int(k)
        states = np.ascontiguousarray(states, dtype=np.uint8)
        if states.ndim == 1:
            states = np.ascontiguousarray(np.broadcast_to(states, (1 if n_rep is None else int(n_rep), states.shape[0])))
        if states.ndim != 2 or states.shape[1] != self.n_samples or (n_rep is not None and states.shape[0] != int(n_rep)):
            raise ValueError(f"states must be (n_rep, {self.n_samples})")
        reps = states.shape[0]
        words, table = [], None
        if keep is not None:
            if len(keep) != len(self.chunk_vars):
                raise ValueError(f"keep needs one array per chunk ({len(self.chunk_vars)})")
            for n_var, mask in zip(self.chunk_vars, keep):
                mask = np.asarray(mask)
                if mask.dtype != np.bool_ or mask.shape != (reps, n_var):
                    raise ValueError(f"a keep mask must be a boolean array of shape ({reps}, {n_var})")
                packed = np.zeros((reps, max(1, (n_var + 63) // 64)), dtype=np.uint64)
                bits = np.packbits(mask, axis=1, bitorder="little")
                packed.view(np.uint8)[:, :bits.shape[1]] = bits
                words.append(packed)
            table = (ctypes.c_void_p * max(1, len(words)))(*[w.ctypes.data for w in words])
        order = np.full((reps, max(k, 0)), -1, dtype=np.int32)
        new = np.zeros((reps, max(k, 0)), dtype=np.int64)
        kept = np.zeros(reps, dtype=np.int64)
        done = np.zeros(reps, dtype=np.int64)
        ms = ctypes.c_double(0.0)
        nat.check(nat.lib().utm_multi_select(self._h, reps, _ptr(states), table, int(seed) & (2 ** 64 - 1),
                                             keep_threshold(1.0 if fraction is None else fraction), k, _ptr(order), _ptr(new),
                                             _ptr(kept), _ptr(done), ctypes.byref(ms) if pass_ms else None))
        return (order, new, kept, done, ms.value) if pass_ms else (order, new, kept, done)

    def coverage_bound(self, k, cand=None, given=None, iters=200, step0=0, period=0, want_lambda=False):
        """A certified upper bound on what any `k` of the samples `cand` (global sample indices; None: every sample) can
        capture beyond the samples `given`, by `iters` projected subgradient steps on the Lagrangian relaxation of maximum
        coverage (utm_coverage_bound; step0 / period 0: the defaults).  Returns a BoundResult: hist (int64 L_t per
        iteration, in units of 1/65,536 variant), bound = min(n_live, min_t hist[t] // 65,536), best_iter, n_live (the
        variants no `given` sample carries), pass_ms (HIP-event time of the launches) and lambdas (want_lambda: one uint32
        array per chunk, the multipliers after the last step; else None).  Stateless: the columns are read, nothing of the
        selection is read or changed."""
        c = None if cand is None else np.ascontiguousarray(cand, dtype=np.int64).reshape(-1)
        g = None if given is None else np.ascontiguousarray(given, dtype=np.int64).reshape(-1)
        iters = int(iters)
        hist = np.zeros(max(iters, 1), dtype=np.int64)
        lambdas = table = None
        if want_lambda:
            lambdas = [np.zeros(max(n_var, 1), dtype=np.uint32) for n_var in self.chunk_vars]
            table = (ctypes.c_void_p * max(1, len(lambdas)))(*[a.ctypes.data for a in lambdas])
        bound, best, n_live, ms = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_double(0.0)
        nat.check(nat.lib().utm_coverage_bound(self._h, _ptr(c) if c is not None and len(c) else None, 0 if c is None else len(c),
                                               _ptr(g) if g is not None and len(g) else None, 0 if g is None else len(g), int(k), iters,
                                               int(step0), int(period), _ptr(hist), ctypes.byref(bound), ctypes.byref(best),
                                               ctypes.byref(n_live), table, ctypes.byref(ms)))
        if want_lambda:
            lambdas = [a[:n_var] for a, n_var in zip(lambdas, self.chunk_vars)]
        return BoundResult(hist[:iters], bound.value, best.value, n_live.value, ms.value, lambdas)

    def coverage_bound_times(self):
        """(sums, pick, update): the summed HIP-event times in ms of the last coverage_bound call's three kernels; zeros
        unless the matrix was created with profile_events."""
        out = np.zeros(3, dtype=np.float64)
        nat.check(nat.lib().utm_coverage_bound_times(self._h, _ptr(out)))
        return tuple(out.tolist())

    def pair_counts(self, indices, given=(), tile_groups=0, pass_ms=False):
        """int64 (n, n): shared[i, j] = the variants the samples indices[i] and indices[j] (global sample indices) both
        carry and no sample of `given` carries; the diagonal is each sample's own count under that mask.  Stateless: the
        columns are read, nothing of the selection is read or changed.  tile_groups moves the launch shape only (0:
        automatic).  pass_ms: return (shared, HIP-event time of the launches) instead."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        panel = np.ascontiguousarray(given, dtype=np.int64).reshape(-1)
        n = len(idx)
        out = np.zeros((n, n), dtype=np.int64)
        ms = ctypes.c_double(0.0)
        nat.check(nat.lib().utm_pair_counts(self._h, _ptr(idx), n, _ptr(panel) if len(panel) else None, len(panel),
                                            int(tile_groups), _ptr(out), ctypes.byref(ms) if pass_ms else None))
        return (out, ms.value) if pass_ms else out

    def carrier_counts(self, indices, given=(), counts=False, hist_mode=0, pass_ms=False):
        """int64 (n + 1): hist[c] = the variants (summed over all chunks) that exactly c of the samples `indices` (global
        sample indices) carry and no sample of `given` carries.  counts: also the list of per-chunk int32 arrays, the
        count of every variant, -1 where a `given` sample carries it.  Stateless: the columns are read, nothing of the
        selection is read or changed.  hist_mode moves the launch shape only (0: automatic, 1: LDS bins, 2: global
        bins).  pass_ms: also the summed HIP-event time of the launches.  Returns hist, or (hist[, counts][, ms])."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        panel = np.ascontiguousarray(given, dtype=np.int64).reshape(-1)
        hist, per_chunk, total_ms = np.zeros(len(idx) + 1, dtype=np.int64), [], 0.0
        for chunk, n_var in enumerate(self.chunk_vars):
            part = np.zeros(len(idx) + 1, dtype=np.int64)
            count = np.empty(n_var, dtype=np.int32) if counts else None
            ms = ctypes.c_double(0.0)
            nat.check(nat.lib().utm_carrier_counts(self._h, chunk, _ptr(idx) if len(idx) else None, len(idx),
                                                   _ptr(panel) if len(panel) else None, len(panel), int(hist_mode), _ptr(part),
                                                   _ptr(count), ctypes.byref(ms) if pass_ms else None))
            hist += part
            total_ms += ms.value
            if counts:
                per_chunk.append(count)
        out = (hist,) + ((per_chunk,) if counts else ()) + ((total_ms,) if pass_ms else ())
        return out if len(out) > 1 else hist

    def group_curve(self, group_of, n_groups, order, private=True, bin_mode=0, pass_ms=False):
        """(new, priv, total, ptotal), summed over all chunks: new[g, j] = the variants some sample of group g carries
        whose first carrier in `order` (global sample indices) stands at position j, priv[g, j] the same over the variants
        no other group carries, total[g] / ptotal[g] = how many of either kind there are (int64; group_of: one id in
        0..n_groups-1 per sample, -1 = in no group).  private=False: priv and ptotal are None and are not computed.
        Stateless: the columns are read, nothing of the selection is read or changed.  bin_mode moves the launch shape
        only (0: automatic, 1: LDS head bins, 2: global bins).  pass_ms: the summed HIP-event time as a fifth item."""
        groups = np.ascontiguousarray(group_of, dtype=np.int32).reshape(-1)
        if groups.shape != (self.n_samples,):
            raise ValueError(f"group_of must have {self.n_samples} entries")
        idx = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
        n, G = len(idx), int(n_groups)
        shape = (max(G, 0), n)
        new, total = np.zeros(shape, np.int64), np.zeros(shape[0], np.int64)
        priv, ptotal = (np.zeros(shape, np.int64), np.zeros(shape[0], np.int64)) if private else (None, None)
        total_ms = 0.0
        for chunk in range(len(self.chunk_vars)):
            part = [np.zeros(shape, np.int64), np.zeros(shape, np.int64) if private else None,
                    np.zeros(shape[0], np.int64), np.zeros(shape[0], np.int64) if private else None]
            ms = ctypes.c_double(0.0)
            nat.check(nat.lib().utm_group_curve(self._h, chunk, _ptr(groups), G, _ptr(idx) if n else None, n, int(bin_mode),
                                                _ptr(part[0]), _ptr(part[1]), _ptr(part[2]), _ptr(part[3]),
                                                ctypes.byref(ms) if pass_ms else None))
            new += part[0]
            total += part[2]
            if private:
                priv += part[1]
                ptotal += part[3]
            total_ms += ms.value
        return (new, priv, total, ptotal) + ((total_ms,) if pass_ms else ())

    def class_counts(self, classes_per_chunk, n_classes, indices=None, tile_groups=0, mode=0, pass_ms=False):
        """int64 (n_rows, n_classes), summed over all chunks: table[j, c] = the variants of class c that sample indices[j]
        (global sample indices; None: every sample, in index order) carries.  classes_per_chunk: one int32 array per
        chunk, a label in 0..n_classes-1 per variant or -1 = counted nowhere.  Stateless: the columns are read, nothing
        of the selection is read or changed.  tile_groups and mode move the launch shape only (0: automatic).  pass_ms:
        return (table, summed HIP-event time of the launches) instead."""
        if len(classes_per_chunk) != len(self.chunk_vars):
            raise ValueError(f"{len(classes_per_chunk)} label arrays for {len(self.chunk_vars)} chunks")
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if idx is not None and len(idx) == 0:
            return (np.zeros((0, int(n_classes)), np.int64), 0.0) if pass_ms else np.zeros((0, int(n_classes)), np.int64)
        rows = self.n_samples if idx is None else len(idx)
        table, total_ms = np.zeros((rows, max(int(n_classes), 0)), dtype=np.int64), 0.0
        for chunk, n_var in enumerate(self.chunk_vars):
            labels = np.ascontiguousarray(classes_per_chunk[chunk], dtype=np.int32).reshape(-1)
            if len(labels) != n_var:
                raise ValueError(f"chunk {chunk}: {len(labels)} labels for {n_var} variants")
            if n_var == 0:                               # (a chunk filtered to nothing: one label that is never read)
                labels = np.full(1, -1, dtype=np.int32)
            part = np.zeros_like(table)
            ms = ctypes.c_double(0.0)
            nat.check(nat.lib().utm_class_counts(self._h, chunk, _ptr(labels), int(n_classes), _ptr(idx), 0 if idx is None else len(idx),
                                                 int(tile_groups), int(mode), _ptr(part), ctypes.byref(ms) if pass_ms else None))
            table += part
            total_ms += ms.value
        return (table, total_ms) if pass_ms else table

    def peek_scores(self):
        counts = np.zeros(self.n_local, dtype=np.int64)
        scores = np.zeros(self.n_local, dtype=np.float64)
        nat.check(nat.lib().utm_peek_scores(self._h, _ptr(counts), _ptr(scores)))
        return counts, scores

    def peek_estimates(self):
        """AF in fixed point: counts and scores of the next iteration from the parallel full pass (not the chains)."""
        counts = np.zeros(self.n_local, dtype=np.int64)
        scores = np.zeros(self.n_local, dtype=np.float64)
        nat.check(nat.lib().utm_peek_estimates(self._h, _ptr(counts), _ptr(scores)))
        return counts, scores

    def covered(self, chunk):
        out = np.zeros((self.chunk_vars[chunk] + 63) // 64, dtype=np.uint64)
        nat.check(nat.lib().utm_get_covered(self._h, chunk, _ptr(out)))
        return out

    def stats(self):
        st = nat.Stats()
        nat.check(nat.lib().utm_get_stats(self._h, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in nat.Stats._fields_}

    def set_decremental(self, on, threshold=0.0):
        """Allow decremental scoring for later iterations (exact; fewer bytes; reported separately)."""
        nat.check(nat.lib().utm_set_decremental(self._h, 1 if on else 0, float(threshold)))

    def set_depth(self, m):
        """Coverage depth: every variant counts until m selected samples carry it (1 = the plain selection).  Takes
        effect with the next reset."""
        nat.check(nat.lib().utm_set_depth(self._h, int(m)))
        self.coverage_depth = int(m)

    def depth(self):
        """{"depth", "apply_launches", "apply_ms"}: the depth in effect and what k_depth_apply has cost since the reset."""
        m, launches, ms = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_double(0.0)
        nat.check(nat.lib().utm_get_depth(self._h, ctypes.byref(m), ctypes.byref(launches), ctypes.byref(ms)))
        return {"depth": m.value, "apply_launches": launches.value, "apply_ms": ms.value}

    def at_depth(self, first_row, n_rows):
        """Variants with support >= depth after each of the rows [first_row, first_row + n_rows) (depth > 1)."""
        out = np.zeros(max(int(n_rows), 1), dtype=np.int64)
        nat.check(nat.lib().utm_get_at_depth(self._h, int(first_row), int(n_rows), _ptr(out)))
        return out[:int(n_rows)].copy()

    def support(self, chunk):
        """Per-variant support of a chunk: how many used samples carry it, saturating at the depth (uint8)."""
        out = np.zeros(self.chunk_vars[chunk], dtype=np.uint8)
        nat.check(nat.lib().utm_get_support(self._h, chunk, _ptr(out)))
        return out

    def set_af_exact_scores(self, on):
        """AF modes: off = skip the sequential chain of an unambiguous winner (same rows; scores become estimates)."""
        nat.check(nat.lib().utm_set_af_exact_scores(self._h, 1 if on else 0))

    def stream_calibration(self, launches=20):
        """GB/s of plain streaming reads over the resident columns (the scoring kernel's access shape, nothing else)."""
        out = ctypes.c_double(0.0)
        nat.check(nat.lib().utm_stream_calibration(self._h, int(launches), ctypes.byref(out)))
        return out.value

    def set_compaction(self, mode=1, min_vars=0, ratio=0.0):
        """Integer loop: score a compacted copy of the columns.  Both at 0 (the default): the library compacts by cost, while
        an iteration still streams more than the caches hold.  Otherwise: once at most `ratio` of a chunk's working variants
        are uncovered and it has at least `min_vars` of them (the one left at 0: 2^21 / 0.5).  mode 0 = off.  Same rows."""
        nat.check(nat.lib().utm_set_compaction(self._h, int(mode), int(min_vars), float(ratio)))

    def compaction_stats(self):
        """{"compactions", "working_vars", "pass_bytes", "pass_ms", "refused", ...} since the last reset; "passes" lists
        (rows out, variants kept, ms) of the first 16 compactions and "sources" what each read ("chunk" or "view")."""
        st = nat.CompactionStats()
        nat.check(nat.lib().utm_get_compaction_stats(self._h, ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in nat.CompactionStats._fields_ if not name.startswith("log_")}
        out["passes"] = [(st.log_iter[k], st.log_vars[k], st.log_ms[k]) for k in range(min(16, st.compactions))]
        out["sources"] = ["view" if st.log_src[k] else "chunk" for k in range(min(16, st.compactions))]
        return out

    def set_list_mode(self, mode=1, min_stream_bytes=0, ratio=0.0):
        """Integer loop: beside a freshly compacted view, score per-sample lists of set positions (4 bytes per carrier instead
        of one bit per variant) once 4 x last gain x `ratio` <= 8 x words per column and an iteration still streams more than
        `min_stream_bytes`.  Both at 0: the defaults (1 GiB, 2.0).  mode 0 = off.  Same rows."""
        nat.check(nat.lib().utm_set_list_mode(self._h, int(mode), int(min_stream_bytes), float(ratio)))

    def set_list_test(self, tile_log2=0, max_entries=0):
        """Test hook: fix the tile of every list build (13, 16, 18, 20; 0 = the rule) / refuse builds above `max_entries`."""
        nat.check(nat.lib().utm_set_list_test(self._h, int(tile_log2), int(max_entries)))

    def list_stats(self):
        """{"builds", "refused", "build_bytes", "build_ms", "mode", "valid", ...} since the last reset; "log" lists the
        first 16 builds as dicts (iter, tiles, t, entries, padded, ms, bytes)."""
        st = nat.ListStats()
        nat.check(nat.lib().utm_get_list_stats(self._h, ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in nat.ListStats._fields_ if not name.startswith("log_")}
        out["log"] = [dict(iter=st.log_iter[k], tiles=st.log_tiles[k], t=st.log_t[k], entries=st.log_entries[k],
                           padded=st.log_padded[k], ms=st.log_ms[k], bytes=st.log_bytes[k]) for k in range(min(16, st.builds))]
        return out

    def set_list_shape(self, lanes=0, target_wgs=0):
        """Lanes of a wave that share one list segment (16 or 64; 0 = by the build's mean segment) from the next build on,
        and the workgroup target of the 16-lane launches (1 .. 65536; 0 = the library's) from the next launch.  Same rows."""
        nat.check(nat.lib().utm_set_list_shape(self._h, int(lanes), int(target_wgs)))

    def list_shape(self):
        """[{"lanes", "wgs"}] of the first 16 list builds since the last reset, in the order of list_stats()["log"]: the lanes
        per segment and the scoring workgroups of the build's first launch."""
        lanes, wgs, n = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)(), ctypes.c_int32(0)
        nat.check(nat.lib().utm_get_list_shape(self._h, lanes, wgs, ctypes.byref(n)))
        return [dict(lanes=lanes[k], wgs=wgs[k]) for k in range(n.value)]

    def set_profile(self, on):
        nat.check(nat.lib().utm_set_profile(self._h, 1 if on else 0))

    # -- sharded building blocks
    def local_best(self):
        rec = nat.Record()
        nat.check(nat.lib().utm_local_best(self._h, ctypes.byref(rec)))
        return (rec.score, rec.idx, rec.new_count)

    def column_words(self):
        n = ctypes.c_uint64()
        nat.check(nat.lib().utm_column_words(self._h, ctypes.byref(n)))
        return n.value

    def get_column(self, global_idx):
        out = np.zeros(self.column_words(), dtype=np.uint64)
        nat.check(nat.lib().utm_get_column(self._h, int(global_idx), _ptr(out)))
        return out

    def apply_records(self, records, winner_col=None):
        """records: [(score, idx, new_count)] of every shard in rank order."""
        arr = (nat.Record * len(records))()
        for r, (score, idx, new) in zip(arr, records):
            r.score, r.idx, r.new_count = float(score), int(idx), int(new)
        col = None if winner_col is None else np.ascontiguousarray(winner_col, dtype=np.uint64)
        i, n, s = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        nat.check(nat.lib().utm_apply_records(self._h, arr, len(records), _ptr(col), ctypes.byref(i),
                                              ctypes.byref(n), ctypes.byref(s)))
        return None if i.value < 0 else (i.value, n.value, s.value)

    # -- P2P column access between shards (hipIpc)
    def p2p_export(self):
        n = ctypes.c_uint64()
        nat.check(nat.lib().utm_p2p_blob_bytes(self._h, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        nat.check(nat.lib().utm_p2p_export(self._h, buf))
        return buf.raw

    def p2p_import(self, rank, blobs):
        """blobs: every shard's p2p_export() in rank order.  Remote winners are then read in place."""
        joined = b"".join(blobs)
        buf = ctypes.create_string_buffer(joined, len(joined))
        nat.check(nat.lib().utm_p2p_import(self._h, int(rank), len(blobs), buf))
        self.p2p = True

    def p2p_selftest(self):
        """Collective over the shards: can this shard see every peer's mailbox stores?"""
        ok = ctypes.c_int32(0)
        nat.check(nat.lib().utm_p2p_selftest(self._h, ctypes.byref(ok)))
        return bool(ok.value)

    def p2p_use_mailboxes(self, on=True):
        """After every shard's self-test passed: run() becomes collective, records travel through the mailboxes."""
        nat.check(nat.lib().utm_p2p_use_mailboxes(self._h, 2 if on == "single" else 1 if on else 0))
        self.fused_mailboxes = bool(on)
        self.fused = bool(on) or getattr(self, "has_comm", False)

    def exchange(self):
        """How run() meets the other shards right now: 'none', 'mailboxes', 'rccl' or 'caller-driven'."""
        return nat.EXCHANGE_NAMES[self.stats()["exchange"]]

    # -- RCCL
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(nat.UNIQUE_ID_BYTES)
        nat.check(nat.lib().utm_comm_get_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, n_ranks, unique_id):
        """One RCCL communicator over the shards.  Unless the mailboxes are switched on, run() then exchanges through
        it: ncclAllGather of the records, ncclBroadcast of the winner's column from its owner."""
        buf = ctypes.create_string_buffer(bytes(unique_id), nat.UNIQUE_ID_BYTES)
        # RCCL announces itself ("RCCL version : ...") on stdout when its first communicator comes up; stdout belongs to
        # the caller (the TSV of `select`, bench.py's one JSON line): that banner goes to stderr instead
        import os
        import sys
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            code = nat.lib().utm_comm_init(self._h, int(rank), int(n_ranks), buf)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        nat.check(code)
        self.fused = True
        self.has_comm = True

    def comm_column_by_allreduce(self, on=True):
        """RCCL exchange: winner column by a root-free ncclAllReduce(sum) instead of an ncclBroadcast from its owner
        (no host sync per iteration; about twice the bytes on the links).  Same rows."""
        nat.check(nat.lib().utm_comm_column_by_allreduce(self._h, 1 if on else 0))

    def allreduce_max(self, value):
        v = ctypes.c_double(float(value))
        nat.check(nat.lib().utm_comm_allreduce_max(self._h, ctypes.byref(v)))
        return v.value


def synth_host(seed, n_var, n_samples, first_sample=0, n_samp=None, first_var_global=0, want_cols=True, want_af=True):
    """The device generator's host twin (bit-identical; no GPU call)."""
    n_samp = n_samples - first_sample if n_samp is None else n_samp
    words = (n_var + 63) // 64
    cols = np.zeros((n_samp, words), dtype=np.uint64) if want_cols else None
    af = np.zeros(n_var, dtype=np.float32) if want_af else None
    nat.check(nat.lib().utm_synth_host(int(seed), int(first_var_global), int(n_var), int(n_samples), int(first_sample),
                                       int(n_samp), _ptr(cols), words, _ptr(af)))
    return cols, af
