"""Working views made from working views (utmos_amd/csrc/host_compact.hip.h): after the first compaction of a run every
later pass reads the view before it and writes the chunk's other column block, moves only the columns of the samples that
are still selectable, and leaves the chunk's own covered mask to the flush before utm_run returns.  Integer arithmetic:
rows, get_covered and peek_scores are the packed C oracle's.  The shapes are those at which such a pass can go wrong: chains
long enough for the first block to be written again, views that end inside a word or are shorter than one, a pending
winner at every boundary, samples that start out used, several chunks, a reset after two passes -- and the library's own
policy on either side of its byte threshold."""
import numpy as np
import pytest

import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu


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


def check_between_calls(m, cols, n_var, state, idx, bounds, weights=None):
    """After the rows `idx`: the chunks' masks are the oracle's (the pending winner's bits included) and the counts of the
    next iteration are its counts (so the winner's bits are in no view)."""
    now = state.copy()
    now[idx] = 0
    want = covered_of(cols, state, idx)
    for c, (lo, hi) in enumerate(bounds):
        assert (m.covered(c) == want[lo // 64:(hi + 63) // 64]).all(), c
    _, cnt, sc = ou.c_score(cols, n_var, now, weights=weights)
    got_cnt, got_sc = m.peek_scores()
    sel = now == 1
    assert (got_cnt[sel] == cnt[sel]).all() and (got_sc[sel] == sc[sel]).all()


def run_chain(dev, dense, state=None, weights=None, ratio=0.99, pieces=None, chunk_sizes=None, between=False):
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
        m.set_compaction(1, min_vars=1, ratio=ratio)
        idx, new, score = [], [], []
        for piece in (pieces or [n_samp]):
            got = m.run(piece)
            idx += got[0].tolist()
            new += got[1].tolist()
            score += got[2].tolist()
            assert idx == exp[0][:len(idx)].tolist() and new == exp[1][:len(new)].tolist()
            if between:
                check_between_calls(m, cols, n_var, state, idx, bounds, weights)
        st, cst = m.stats(), m.compaction_stats()
        covered = [m.covered(c) for c in range(len(bounds))]
    assert idx == exp[0].tolist() and new == exp[1].tolist() and score == exp[2].tolist()
    want = covered_of(cols, state, idx)
    for c, (a, b) in enumerate(bounds):
        assert (covered[c] == want[a // 64:(b + 63) // 64]).all(), c
    assert st["tot_captured"] == sum(new) and cst["refused"] == 0 and cst["view_refused"] == 0
    assert cst["view_passes"] == cst["sources"].count("view") or cst["compactions"] > 16
    assert cst["sources"][:1] in ([], ["chunk"])       # the first pass of a run reads the chunk
    return st, cst


@pytest.mark.parametrize("n_samp", [37, 300])
@pytest.mark.parametrize("n_var", [200, 8_191, 8_193, 70_000])
def test_chains_of_passes_return_to_the_first_block(dev, n_var, n_samp):
    rng = np.random.default_rng(n_var * 3 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    # 300 samples in one call: boundaries after 16, 48, 112 and 240 rows; 37 samples: one at the start of every call
    pieces = None if n_samp == 300 else [1, 2, 3, 4, 6, n_samp]
    _, cst = run_chain(dev, dense, pieces=pieces)
    if n_var >= 8_191:     # (200 variants: the 1 % a pass must drop is two variants, and few rows are left to lose them)
        assert cst["compactions"] >= 3 and cst["view_passes"] >= 2, cst
        assert cst["sources"][:3] == ["chunk", "view", "view"]
        kept = [p[1] for p in cst["passes"]]
        assert all(b < a for a, b in zip(kept, kept[1:])) and cst["working_vars"] == kept[-1]


def test_views_that_end_inside_a_word_and_one_under_a_word(dev):
    rng = np.random.default_rng(41)
    n_var, n_samp = 6_000, 48
    dense = np.zeros((n_var, n_samp), bool)
    # three dense columns, picked first: sample 0 leaves 1,000 + 37 variants, sample 1 leaves 101 of them, sample 2 leaves 50
    left0 = rng.choice(n_var, 1_037, replace=False)
    dense[:, 0] = True
    dense[left0, 0] = False
    dense[left0[101:], 1] = True
    dense[left0[50:101], 2] = True
    for v in left0[:50]:                                # the last 50: one or two carriers each among the other samples
        dense[v, rng.integers(3, n_samp, 2)] = True
    for v in left0[50:]:                                # (... and a few more carriers, so that the dense columns keep their order)
        dense[v, rng.integers(3, n_samp)] |= rng.random() < 0.3
    _, cst = run_chain(dev, dense, pieces=[1, 1, 1, 2, n_samp], between=True)
    kept = [p[1] for p in cst["passes"]]
    assert kept[:3] == [1_037, 101, 50] and cst["sources"][:3] == ["chunk", "view", "view"], cst
    assert cst["compactions"] >= 4 and kept[3] < 50     # the view under a word was compacted again


@pytest.mark.parametrize("n_var,n_samp", [(8_193, 37), (131_073, 131)])
def test_a_pending_winner_at_every_boundary(dev, n_var, n_samp):
    rng = np.random.default_rng(n_var + 1)
    dense = ou.random_dense(rng, n_var, n_samp)
    _, cst = run_chain(dev, dense, pieces=[1, 2, 3, 255], between=True)
    assert cst["compactions"] >= 3 and cst["view_passes"] >= 2


@pytest.mark.parametrize("weighted", [False, True])
def test_samples_that_start_out_used_are_skipped(dev, weighted):
    rng = np.random.default_rng(43)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    first = int(ou.c_greedy(cols, n_var, np.ones(n_samp, np.uint8), k_max=1)[0][0])
    state = np.ones(n_samp, np.uint8)
    state[[first, 4, 77, 130]] = 0                      # used from the start, the sample that would win first among them
    state[[9, 10]] = 2
    weights = None
    if weighted:
        weights = rng.integers(1, 4, n_samp).astype(np.float64)
    _, cst = run_chain(dev, dense, state, weights=weights, pieces=[1, 2, 3, 10, 32, n_samp], between=True)
    assert cst["compactions"] >= 3 and cst["view_passes"] >= 2


def test_three_uneven_chunks_one_too_small_to_compact(dev):
    rng = np.random.default_rng(17)
    sizes = [40_000 - 40_000 % 64, 9_024, 33_000]
    n_var, n_samp = sum(sizes), 131
    dense = ou.random_dense(rng, n_var, n_samp)
    lo = sizes[0]
    dense[lo:lo + 8_000, :] = False                    # most of the middle chunk has no carriers: it stays uncovered
    st, cst = run_chain(dev, dense, ratio=0.5, chunk_sizes=sizes, pieces=[4, 12, 32, 64, n_samp], between=True)
    assert cst["compactions"] >= 3 and cst["view_passes"] >= 1 and st["n_chunks"] == 3
    assert sizes[1] <= cst["working_vars"] < sizes[1] + (sizes[0] + sizes[2]) // 2


def test_reset_and_set_state_after_two_passes(dev):
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
        m.run(50)                                       # passes after 16 and 48 rows: the view lives in the second block
        cst = m.compaction_stats()
        assert cst["compactions"] == 2 and cst["sources"] == ["chunk", "view"] and cst["working_vars"] < n_var
        m.reset()
        cst = m.compaction_stats()
        assert cst["compactions"] == 0 and cst["view_passes"] == 0 and cst["working_vars"] == n_var and cst["pass_bytes"] == 0
        got = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist()
        assert m.compaction_stats()["sources"][:2] == ["chunk", "view"]      # the next run starts from the chunk again
        assert (m.covered(c) == covered_of(cols, state, got[0])).all()
        m.reset()
        m.run(50)
        m.set_state(state2)                             # (takes effect with the next run, which resets the loop)
        got = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state2)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist()
        assert m.compaction_stats()["sources"][:2] == ["chunk", "view"]
        assert (m.covered(c) == covered_of(cols, state2, got[0])).all()


# The library's own policy leaves a view alone once an iteration streams no more than 256 MiB from it: selectable samples x
# words per column x 8.  Columns are whole KiB, so with 2,504 samples, 16 of them gone at the first boundary, 13,440 words
# (860,160 variants) are 267.5 MB there, just below the threshold, and one variant more makes 13,568 words, 270.1 MB, above.
STREAM_BYTES = 256 << 20
N_SAMP, N_BELOW, N_ABOVE, ROWS = 2504, 860_160, 860_161, 48     # (48 rows: a whole batch is still wanted at the boundary after 16)


@pytest.fixture(scope="module")
def straddle():
    # one matrix for both shapes, carrier density 1/8: about a tenth of the variants is left after 16 rows
    rng = np.random.default_rng(47)
    shape = (N_SAMP, (N_ABOVE + 63) // 64)
    cols = rng.integers(0, 2**64, shape, np.uint64)
    cols &= rng.integers(0, 2**64, shape, np.uint64)
    cols &= rng.integers(0, 2**64, shape, np.uint64)
    cols[:, -1] &= np.uint64(1)                        # (the longer shape ends one variant into its last word)
    return cols


@pytest.mark.parametrize("n_var", [N_BELOW, N_ABOVE])
def test_default_policy_on_either_side_of_the_byte_threshold(dev, straddle, n_var):
    w = (n_var + 63) // 64
    wp = (w + 127) // 128 * 128
    assert ((N_SAMP - 16) * wp * 8 > STREAM_BYTES) == (n_var == N_ABOVE) and N_SAMP * wp * 8 > STREAM_BYTES
    cols = np.ascontiguousarray(straddle[:, :w])
    if n_var == N_BELOW:
        assert w * 64 == n_var
    state = np.ones(N_SAMP, np.uint8)
    exp = ou.c_greedy(cols, n_var, state, k_max=ROWS, omp=True)
    with dev.DeviceMatrix(N_SAMP) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        got = m.run(ROWS)
        cst = m.compaction_stats()
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist()
        assert cst["min_vars"] == 0 and cst["ratio"] == 0 and cst["stream_bytes"] == STREAM_BYTES
        if n_var == N_ABOVE:
            assert cst["compactions"] > 0 and cst["passes"][0][0] == 16 and cst["working_vars"] < n_var, cst
        else:
            assert cst["compactions"] == 0 and cst["working_vars"] == n_var, cst
        assert (m.covered(c) == covered_of(cols, state, got[0])[:w]).all()


def test_default_policy_leaves_2m_by_500_alone(dev):
    n_var, n_samp = 2_000_000, 500
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=1)
        got = m.run(300)
        assert len(got[0]) == 300
        cst = m.compaction_stats()
        assert cst["compactions"] == 0 and cst["working_vars"] == n_var and cst["pass_bytes"] == 0, cst
