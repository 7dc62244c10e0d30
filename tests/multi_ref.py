"""Restatement of the replicated selection (utm_multi_select) in numpy, independent of the packed code: dense boolean rows,
replicate by replicate through the oracle's own greedy loop on the kept rows, and the hashed masks in uint64 arithmetic.

select()          the definition: per replicate npo.greedy (oracle/utmos_oracle.py) on dense[keep_b].
select_batched()  the same selection for all replicates at once as one float32 matrix product per row (every count is an
                  integer below 2^24, so the products are exact): what the GPU tests use at sizes where B passes of the
                  oracle's row loop would take minutes.  tests/test_multi_host.py holds it against select().
"""
import ctypes

import numpy as np

import oracle_util as ou

npo = ou.npo

M64 = (1 << 64) - 1
C_VAR, C_REP = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
C_MIX1, C_MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def hash_one(seed, v, b):
    """Plain Python integers, one (variant, replicate) at a time: the issue's four lines."""
    z = (seed + C_VAR * (v + 1) + C_REP * (b + 1)) & M64
    z = ((z ^ (z >> 30)) * C_MIX1) & M64
    z = ((z ^ (z >> 27)) * C_MIX2) & M64
    return z ^ (z >> 31)


def hashed_keep(seed, n_rep, n_var, threshold, first_var=0):
    """bool (n_rep, n_var): variant first_var + i belongs to replicate b iff (z >> 32) < threshold; uint64 arithmetic wraps."""
    with np.errstate(over="ignore"):
        v = (np.arange(n_var, dtype=np.uint64) + np.uint64(first_var) + np.uint64(1)) * np.uint64(C_VAR)
        b = (np.arange(n_rep, dtype=np.uint64) + np.uint64(1)) * np.uint64(C_REP)
        z = np.uint64(seed & M64) + v[None, :] + b[:, None]
        z = (z ^ (z >> np.uint64(30))) * np.uint64(C_MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(C_MIX2)
        z = z ^ (z >> np.uint64(31))
    top = (z >> np.uint64(32)).astype(np.int64)
    return top < int(threshold)


def pack_keep(keep):
    """bool (n_rep, n_var) -> uint64 (n_rep, max(1, ceil(n_var / 64))), variant v = bit v & 63 of word v >> 6."""
    keep = np.asarray(keep, dtype=bool)
    words = np.zeros((keep.shape[0], max(1, (keep.shape[1] + 63) // 64)), dtype=np.uint64)
    bits = np.packbits(keep, axis=1, bitorder="little")
    words.view(np.uint8)[:, :bits.shape[1]] = bits
    return words


def _outputs(n_rep, k):
    return (np.full((n_rep, k), -1, dtype=np.int32), np.zeros((n_rep, k), dtype=np.int64), np.zeros(n_rep, dtype=np.int64),
            np.zeros(n_rep, dtype=np.int64))


def select(dense, states, keep, k):
    """dense bool (n_var, n_samp), states uint8 (n_rep, n_samp), keep bool (n_rep, n_var) -> (order, new, kept, n_done)."""
    dense = np.asarray(dense, dtype=bool)
    n_rep = len(states)
    order, new, kept, n_done = _outputs(n_rep, k)
    names = np.arange(dense.shape[1])
    for b in range(n_rep):
        rows = dense[np.asarray(keep[b], dtype=bool)]
        kept[b] = rows.shape[0]
        if rows.shape[0] == 0 or k == 0:
            continue
        state = np.array(states[b], dtype=np.uint8, copy=True)
        for i, row in enumerate(ou.npo.greedy(rows, np.zeros(dense.shape[1], np.int64), k, names, state)):
            order[b, i], new[b, i] = row[0], row[2]
            n_done[b] = i + 1
    return order, new, kept, n_done


def select_batched(dense, states, keep, k):
    """The same as select(), every replicate advanced together: counts = live (n_rep, n_var) @ dense (n_var, n_samp)."""
    dense = np.asarray(dense, dtype=bool)
    assert dense.shape[0] < (1 << 24)
    states = np.array(states, dtype=np.uint8, copy=True)
    keep = np.asarray(keep, dtype=bool)
    n_rep, n_samp = states.shape
    order, new, kept, n_done = _outputs(n_rep, k)
    kept[:] = keep.sum(axis=1)
    m32 = dense.astype(np.float32)
    live = keep.copy()
    for b in range(n_rep):
        used = np.flatnonzero(states[b] == ou.npo.USED)
        if len(used):
            live[b] &= ~dense[:, used].any(axis=1)
    running = np.ones(n_rep, dtype=bool)
    captured = np.zeros(n_rep, dtype=np.int64)
    for i in range(min(k, n_samp)):
        if not running.any():
            break
        at = np.flatnonzero(running)
        counts = (live[at].astype(np.float32) @ m32).astype(np.int64)
        counts[states[at] != ou.npo.USABLE] = 0
        best = counts.argmax(axis=1)                                  # first maximum
        gain = counts[np.arange(len(at)), best]
        for b, s, g in zip(at, best, gain):
            if g == 0:
                running[b] = False
                continue
            order[b, i], new[b, i], n_done[b] = s, g, i + 1
            captured[b] += g
            states[b, s] = ou.npo.USED
            live[b] &= ~dense[:, s]
            if captured[b] >= kept[b]:
                running[b] = False
    return order, new, kept, n_done


def mixed_states(rng, n_rep, n_samp):
    """States that differ per replicate: mostly selectable, some used, some excluded; replicate 0 all selectable."""
    states = rng.choice(np.array([1, 1, 1, 1, 0, 2], dtype=np.uint8), size=(n_rep, n_samp))
    states[0] = 1
    return states


# ----------------------------------------------------------------- shared by the host and the GPU tests
def host_select(dense, states, keep, k, wp=None):
    """utm_multi_select_host on the packed columns of `dense` (bool (n_var, n_samp))."""
    from utmos_amd import _native as nat
    n_var, n_samp = dense.shape
    cols = npo.pack_columns(dense)
    if wp is not None:                                               # a stride wider than the words in use
        wide = np.zeros((n_samp, wp), dtype=np.uint64)
        wide[:, :cols.shape[1]] = cols
        cols = wide
    states = np.ascontiguousarray(states, dtype=np.uint8)
    words = pack_keep(keep)[:, :max((n_var + 63) // 64, 0)] if n_var else np.zeros((len(states), 0), np.uint64)
    words = np.ascontiguousarray(words)
    n_rep = len(states)
    order = np.full((n_rep, k), 77, dtype=np.int32)
    new = np.full((n_rep, k), 77, dtype=np.int64)
    kept = np.full(n_rep, 77, dtype=np.int64)
    done = np.full(n_rep, 77, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_multi_select_host(p(cols), cols.shape[1], n_var, n_samp, n_rep, p(states), p(words), k, p(order), p(new),
                                              p(kept), p(done)))
    return order, new, kept, done


def same(got, want, tag=""):
    for g, w, what in zip(got, want, ("order", "new", "kept", "n_done")):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (tag, what)


def family_keep(rng, n_rep, n_var):
    """Replicate by replicate: all ones, all zero, a random half, one kept variant, in turn."""
    keep = np.zeros((n_rep, n_var), dtype=bool)
    for b in range(n_rep):
        kind = b % 4
        if kind == 0:
            keep[b] = True
        elif kind == 2:
            keep[b] = rng.random(n_var) < 0.5
        elif kind == 3:
            keep[b, rng.integers(0, n_var)] = True
    return keep
