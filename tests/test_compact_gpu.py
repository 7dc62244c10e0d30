"""Working views of the integer loop (utmos_amd/csrc/host_compact.hip.h): once enough of a chunk is covered the loop scores
a compacted copy of its columns.  Integer arithmetic: the rows, get_covered and peek_scores are the C oracle's with
compaction forced (`set_compaction(1, min_vars=1, ratio)`) over the shapes at which the pieces change: the compaction
kernel's wave covers 8,192 variants and its workgroup 32,768, k_score_intq needs a column of one 16 KiB tile (131,072
variants) and k_score_int takes over below."""
import numpy as np
import pytest

import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

VARIANTS = [1, 63, 64, 65, 8_191, 8_193, 32_769, 70_001, 131_073, 300_000]
SAMPLES = [1, 5, 37, 131]


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def covered_of(cols, state, idx):
    want = np.zeros(cols.shape[1], np.uint64)
    for s in list(np.flatnonzero(state == 0)) + list(idx):
        want |= cols[s]
    return want


def check_between_calls(m, cols, n_var, state, idx, bounds):
    """get_covered and peek_scores after the rows `idx`: the oracle's covered mask and its counts of the next iteration."""
    now = state.copy()
    now[idx] = 0
    want = covered_of(cols, state, idx)
    for c, (lo, hi) in enumerate(bounds):
        assert lo % 64 == 0
        assert (m.covered(c) == want[lo // 64:(hi + 63) // 64]).all(), c
    _, cnt, sc = ou.c_score(cols, n_var, now)
    got_cnt, got_sc = m.peek_scores()
    sel = now == 1
    assert (got_cnt[sel] == cnt[sel]).all() and (got_sc[sel] == sc[sel]).all()


def run_compacted(dev, dense, state=None, weights=None, ratio=0.5, pieces=None, chunk_sizes=None, between=False, setup=None,
                  compaction=True):
    """One selection with compaction forced, against the oracle: rows, scores, covered masks.  -> (stats, compaction stats)."""
    n_var, n_samp = dense.shape
    state = np.ones(n_samp, np.uint8) if state is None else state
    cols = npo.pack_columns(dense)
    exp = ou.c_greedy(cols, n_var, state, weights=weights)
    bounds, lo = [], 0
    for size in (chunk_sizes or [n_var]):
        bounds.append((lo, lo + size))
        lo += size
    assert lo == n_var
    with dev.DeviceMatrix(n_samp) as m:
        for a, b in bounds:
            c = m.add_chunk(b - a)
            m.upload_columns(c, npo.pack_columns(dense[a:b]))
        m.set_state(state)
        if weights is not None:
            m.set_weights(weights)
        if setup:
            setup(m)
        if compaction:
            m.set_compaction(1, min_vars=1, ratio=ratio)
        idx, new, score = [], [], []
        for piece in (pieces or [n_samp]):
            got = m.run(piece)
            idx += got[0].tolist()
            new += got[1].tolist()
            score += got[2].tolist()
            assert idx == exp[0][:len(idx)].tolist() and new == exp[1][:len(new)].tolist()
            if between:
                check_between_calls(m, cols, n_var, state, idx, bounds)
        st, cst = m.stats(), m.compaction_stats()
        covered = [m.covered(c) for c in range(len(bounds))]
    assert idx == exp[0].tolist() and new == exp[1].tolist() and score == exp[2].tolist()
    want = covered_of(cols, state, idx)
    for c, (a, b) in enumerate(bounds):
        assert (covered[c] == want[a // 64:(b + 63) // 64]).all(), c
    assert st["tot_captured"] == sum(new) and cst["refused"] == 0
    return st, cst


@pytest.mark.parametrize("ratio", [0.5, 0.99])
@pytest.mark.parametrize("n_var", VARIANTS)
def test_rows_over_the_kernels_shapes(dev, n_var, ratio):
    for n_samp in SAMPLES:
        rng = np.random.default_rng(n_var * 7 + n_samp)
        dense = ou.random_dense(rng, n_var, n_samp)
        # (one call: boundaries after 16 and 48 rows; cut into calls: one at the start of every call)
        _, cst = run_compacted(dev, dense, ratio=ratio)
        _, cut = run_compacted(dev, dense, ratio=ratio, pieces=[1, 2, 3, 255])
        if ratio == 0.99 and n_samp >= 37 and n_var >= 8_191:
            assert cst["compactions"] >= 1 and cut["compactions"] >= 2, (n_samp, cst, cut)
            assert cst["working_vars"] < n_var and cst["pass_bytes"] > 0 and cst["pass_ms"] > 0


def test_a_compaction_that_keeps_less_than_a_word_and_one_that_ends_the_run(dev):
    rng = np.random.default_rng(5)
    n_var, n_samp = 5_000, 40
    dense = np.zeros((n_var, n_samp), bool)
    rest = rng.choice(n_var, 50, replace=False)
    dense[:, 0] = True
    dense[rest, 0] = False
    for v in rest:                                   # the 50 variants sample 0 misses: one or two carriers each
        dense[v, rng.integers(1, n_samp, 2)] = True
    st, cst = run_compacted(dev, dense, pieces=[1, n_samp])
    assert cst["compactions"] >= 1 and cst["passes"][0][0] == 1 and cst["passes"][0][1] == 50 and st["iterations"] > 2
    # nobody carries what sample 0 misses: the pass after the compaction scores zero everywhere and ends the run
    dense[rest, :] = False
    st, cst = run_compacted(dev, dense, pieces=[1, n_samp])
    assert cst["compactions"] == 1 and cst["passes"][0][1] == 50 and st["iterations"] == 1


@pytest.mark.parametrize("ratio", [0.5, 0.99])
def test_ties_states_and_weights(dev, ratio):
    rng = np.random.default_rng(11)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp, density=0.02)
    dense[:, 7] = dense[:, 3]                          # exact ties: lowest index first
    dense[:, 100] = dense[:, 3]
    state = np.ones(n_samp, np.uint8)
    state[rng.choice(n_samp, 20, replace=False)] = 2   # excluded: never selected, never cover
    state[[5, 99, 120]] = 0                            # start out used: cover from the first iteration
    state[[3, 7, 100]] = 1
    _, cst = run_compacted(dev, dense, state, ratio=ratio, pieces=[20, 20, n_samp])
    assert cst["compactions"] >= 1
    weights = rng.integers(-2, 4, n_samp).astype(np.float64)   # signed and zero weights: float64 products of the counts
    weights[3] = weights[7] = weights[100] = 2.0
    _, cst = run_compacted(dev, dense, state, weights=weights, ratio=ratio, pieces=[20, 20, n_samp])
    assert cst["compactions"] >= 1


def test_three_uneven_chunks_one_of_which_is_never_compacted(dev):
    rng = np.random.default_rng(17)
    sizes = [40_000 - 40_000 % 64, 9_024, 33_000]
    n_var, n_samp = sum(sizes), 131
    dense = ou.random_dense(rng, n_var, n_samp)
    lo = sizes[0]
    dense[lo:lo + 8_000, :] = False                    # most of the middle chunk has no carriers: it stays uncovered
    st, cst = run_compacted(dev, dense, ratio=0.5, chunk_sizes=sizes, pieces=[16, 32, n_samp], between=True)
    assert cst["compactions"] >= 2 and st["n_chunks"] == 3
    assert sizes[1] <= cst["working_vars"] < sizes[1] + (sizes[0] + sizes[2]) // 2


@pytest.mark.parametrize("n_var,n_samp", [(8_193, 37), (131_073, 131)])
def test_runs_cut_into_calls_with_covered_and_scores_in_between(dev, n_var, n_samp):
    rng = np.random.default_rng(n_var)
    dense = ou.random_dense(rng, n_var, n_samp)
    _, cst = run_compacted(dev, dense, ratio=0.99, pieces=[1, 2, 3, 255], between=True)
    assert cst["compactions"] >= 3


def test_set_state_and_reset_in_mid_run(dev):
    rng = np.random.default_rng(23)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    state = np.ones(n_samp, np.uint8)
    state2 = state.copy()
    state2[[1, 50]] = 0
    state2[[2, 60, 61]] = 2
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        m.set_compaction(1, min_vars=1, ratio=0.99)
        m.run(40)
        assert m.compaction_stats()["compactions"] >= 1 and m.compaction_stats()["working_vars"] < n_var
        m.reset()                                      # the view goes, its buffer stays for the next run
        assert m.compaction_stats()["compactions"] == 0 and m.compaction_stats()["working_vars"] == n_var
        got = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
        m.reset()
        m.run(40)
        m.set_state(state2)                            # ... and so it does when the states change
        got = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state2)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
        assert m.compaction_stats()["compactions"] >= 1
        assert (m.covered(c) == covered_of(cols, state2, got[0])).all()
        m.set_compaction(0)                            # switched off in mid-run: the chunk itself is scored again
        m.reset()
        m.run(40)
        m.set_compaction(1, min_vars=1, ratio=0.99)
        first = m.run(30)
        m.set_compaction(0)
        rest = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state2)
        assert exp[0][40:].tolist() == first[0].tolist() + rest[0].tolist()


def test_launches_forced_and_the_persistent_loop_admitted_after_a_compaction(dev, monkeypatch):
    rng = np.random.default_rng(29)
    n_var, n_samp = 300_000, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    # 131 columns of 300,000 variants are 4.7 MiB: with the persistent loop's size limit at 3 MiB the run starts as launches
    # and the loop takes over on the view, once that is short enough
    monkeypatch.setenv("UTM_PERSIST_MAX_MB", "3")
    st, cst = run_compacted(dev, dense, ratio=0.5)
    assert cst["compactions"] > 0 and st["persist_iterations"] > 0 and st["persist_iterations"] < st["iterations"]
    monkeypatch.setenv("UTM_PERSISTENT", "0")
    st, cst = run_compacted(dev, dense, ratio=0.5)
    assert cst["compactions"] > 0 and st["persist_iterations"] == 0


def _one_rank_mailboxes(m):
    m.p2p_import(0, [m.p2p_export()])
    assert m.p2p_selftest()
    m.p2p_use_mailboxes("single")


@pytest.mark.parametrize("form", ["af", "depth2", "decremental", "mailboxes"])
def test_ineligible_contexts_do_not_compact(dev, form):
    rng = np.random.default_rng(31)
    n_var, n_samp = 32_769, 37
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    state = np.ones(n_samp, np.uint8)
    if form in ("decremental", "mailboxes"):
        setup = (lambda m: m.set_decremental(True)) if form == "decremental" else _one_rank_mailboxes
        _, cst = run_compacted(dev, dense, ratio=0.99, pieces=[16, 16, n_samp], setup=setup)
        assert cst["compactions"] == 0 and cst["working_vars"] == n_var
        return
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        m.set_compaction(1, min_vars=1, ratio=0.99)
        if form == "af":
            af = (rng.random(n_var) * 0.5 + 1e-3).astype(np.float32)
            m.set_af(c, af)
            exp = ou.c_greedy(cols, n_var, state, af=af)
        else:
            import depth_ref
            m.set_depth(2)
            rows, _ = depth_ref.packed_greedy(cols, n_var, state.copy(), n_samp, 2)
            exp = ([r[0] for r in rows], [r[1] for r in rows])
        got = [m.run(16), m.run(n_samp)]
        idx = got[0][0].tolist() + got[1][0].tolist()
        new = got[0][1].tolist() + got[1][1].tolist()
        assert idx == list(exp[0]) and new == list(exp[1])
        assert m.compaction_stats()["compactions"] == 0 and m.compaction_stats()["working_vars"] == n_var
