"""List views of the integer loop (utmos_amd/csrc/host_list.hip.h, list.hip.h): beside a freshly compacted working view
the loop scores per-sample lists of set positions instead of bitmap columns.  Integer arithmetic: rows, scores,
get_covered and peek_scores are the packed C oracle's.  The shapes are those at which a list can go wrong: views shorter
than one tile, ending inside a word, exactly at a tile edge and one bit past it (the smallest tile forced, so that several
tiles exist), segments of 0, 1, 3, 4 and 5 entries, a pending winner at every boundary, samples that start out used,
several chunks with a build refused for one of them, a reset after two builds, weights of either sign -- and the library's
own gate on the two shapes that must stay on the bitmap path launch for launch."""
import numpy as np
import pytest

import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

T_SMALL = 13            # 8,192 positions per tile: the test-only tile
FORCE = 1e-9            # list ratio that lets every pass build


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


def oracle_counts(cols, n_var, state, idx, weights=None):
    now = state.copy()
    now[idx] = 0
    _, cnt, sc = ou.c_score(cols, n_var, now, weights=weights)
    return now == 1, cnt, sc


def run_lists(dev, dense, state=None, weights=None, pieces=None, chunk_sizes=None, between=True, tile=T_SMALL, ratio=FORCE,
              max_entries=0, list_mode=1, compact_ratio=0.99):
    """One selection with compaction and list mode forced, against the oracle.  -> (stats, compaction stats, list stats)."""
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
        m.set_compaction(1, min_vars=1, ratio=compact_ratio)
        m.set_list_mode(list_mode, min_stream_bytes=1, ratio=ratio)
        m.set_list_test(tile, max_entries)
        idx, new, score = [], [], []
        builds_seen = 0
        for piece in (pieces or [n_samp]):
            got = m.run(piece)
            idx += got[0].tolist()
            new += got[1].tolist()
            score += got[2].tolist()
            assert idx == exp[0][:len(idx)].tolist() and new == exp[1][:len(new)].tolist()
            lst = m.list_stats()
            # a build's entries are the uncovered carriers of the samples selectable at its iteration
            for b in lst["log"][builds_seen:]:
                if len(bounds) == 1:
                    sel, cnt, _ = oracle_counts(cols, n_var, state, idx[:b["iter"]])
                    assert b["entries"] == int(cnt[sel].sum()), b
                assert b["entries"] <= b["padded"] < b["entries"] + 4 * b["tiles"] * n_samp and b["t"] == (tile or b["t"])
            builds_seen = min(16, lst["builds"])
            if between and len(got[0]) == piece:        # (a run that has stopped scores nothing any more)
                want = covered_of(cols, state, idx)
                for c, (a, b) in enumerate(bounds):
                    assert (m.covered(c) == want[a // 64:(b + 63) // 64]).all(), c
                sel, cnt, sc = oracle_counts(cols, n_var, state, idx, weights)
                got_cnt, got_sc = m.peek_scores()
                assert (got_cnt[sel] == cnt[sel]).all() and (got_sc[sel] == sc[sel]).all()
        st, cst, lst = m.stats(), m.compaction_stats(), m.list_stats()
        covered = [m.covered(c) for c in range(len(bounds))]
    assert idx == exp[0].tolist() and new == exp[1].tolist() and score == exp[2].tolist()
    want = covered_of(cols, state, idx)
    for c, (a, b) in enumerate(bounds):
        assert (covered[c] == want[a // 64:(b + 63) // 64]).all(), c
    assert st["tot_captured"] == sum(new)
    return st, cst, lst


SHAPES = [(200, 37), (200, 300), (8_191, 37), (8_191, 300), (8_193, 37), (8_193, 300), (70_000, 37), (70_000, 300),
          (2**16 + 1, 37), (3 * 2**16 + 65, 37)]


@pytest.mark.parametrize("n_var,n_samp", SHAPES)
def test_rows_scores_and_masks_are_the_oracles(dev, n_var, n_samp):
    rng = np.random.default_rng(n_var * 5 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    # a pending winner sits at every boundary; 300 samples: the last call has boundaries of its own after 48, 112, 240 rows
    _, cst, lst = run_lists(dev, dense, pieces=[1, 2, 17, n_samp])
    assert lst["builds"] >= 2 and lst["refused"] == 0 and cst["compactions"] >= lst["builds"], (cst, lst)
    if n_var >= 8_193 * 4:
        assert lst["log"][0]["tiles"] > 1, lst


def test_segments_of_every_padding_and_a_view_that_ends_at_a_tile_edge(dev):
    rng = np.random.default_rng(7)
    tile, n_samp = 1 << T_SMALL, 41
    region = 5 * tile                                   # what is left after the first pick: five whole tiles
    n_var = region + 6_000
    dense = np.zeros((n_var, n_samp), bool)
    dense[region:region + 3_000, :] = True              # rows everybody carries ...
    dense[region + 3_000:, 0] = True                    # ... and sample 0's own: it wins first and leaves the region
    for v in range(region):                             # sparse carriers among samples 2.., every row informative
        dense[v, rng.integers(2, n_samp, 1 + (v % 3 == 0))] = True
    for t, n in enumerate([0, 1, 3, 4, 5]):             # sample 1: segments of 0, 1, 3, 4 and 5 entries
        dense[t * tile + rng.choice(tile, n, replace=False), 1] = True
    _, cst, lst = run_lists(dev, dense, pieces=[1, 1, 3, n_samp])
    assert cst["passes"][0][:2] == (1, region) and lst["log"][0]["iter"] == 1 and lst["log"][0]["tiles"] == 5, (cst, lst)
    assert lst["log"][0]["padded"] > lst["log"][0]["entries"]


@pytest.mark.parametrize("weighted", [False, True])
def test_samples_that_start_out_used_and_signed_weights(dev, weighted):
    rng = np.random.default_rng(43)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    first = int(ou.c_greedy(cols, n_var, np.ones(n_samp, np.uint8), k_max=1)[0][0])
    state = np.ones(n_samp, np.uint8)
    state[[first, 4, 77, 130]] = 0
    state[[9, 10]] = 2
    weights = rng.integers(-2, 4, n_samp).astype(np.float64) if weighted else None
    _, _, lst = run_lists(dev, dense, state, weights=weights, pieces=[1, 2, 3, 10, 32, n_samp])
    assert lst["builds"] >= 3 and lst["refused"] == 0, lst


def test_three_chunks_and_a_build_refused_for_one_of_two(dev):
    rng = np.random.default_rng(17)
    sizes = [40_000 - 40_000 % 64, 9_024, 33_000]
    n_var, n_samp = sum(sizes), 131
    dense = ou.random_dense(rng, n_var, n_samp)
    _, cst, lst = run_lists(dev, dense, chunk_sizes=sizes, pieces=[4, 12, 32, 64, n_samp])
    assert lst["builds"] >= 6 and lst["refused"] == 0 and lst["log"][0]["iter"] == lst["log"][2]["iter"] == 4, lst
    # two chunks, the second half as long: a capacity between their first builds refuses the longer one for the run
    sizes = [64_000, 32_000]
    dense = ou.random_dense(rng, sum(sizes), n_samp)
    _, _, lst = run_lists(dev, dense, chunk_sizes=sizes, pieces=[4, n_samp], between=False)
    big, small = lst["log"][0]["padded"], lst["log"][1]["padded"]
    assert lst["log"][0]["iter"] == lst["log"][1]["iter"] == 4 and small < big
    _, cst, lst = run_lists(dev, dense, chunk_sizes=sizes, pieces=[4, 12, 32, n_samp], max_entries=(big + small) // 2)
    assert lst["refused"] == 1 and lst["builds"] >= 2 and all(b["padded"] <= (big + small) // 2 for b in lst["log"]), lst
    assert cst["compactions"] > lst["builds"]           # the refused chunk went on compacting its bitmap view


def test_a_refused_buffer_leaves_the_run_on_the_bitmap_view(dev):
    rng = np.random.default_rng(29)
    dense = ou.random_dense(rng, 70_000, 131)
    st, cst, lst = run_lists(dev, dense, pieces=[3, 20, 131], max_entries=1)
    assert lst["builds"] == 0 and lst["refused"] == 1 and lst["valid"] == 0 and cst["compactions"] >= 3, (cst, lst)


def test_reset_after_two_builds_then_a_full_run(dev):
    rng = np.random.default_rng(23)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    state = np.ones(n_samp, np.uint8)
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        m.set_compaction(1, min_vars=1, ratio=0.99)
        m.set_list_mode(1, min_stream_bytes=1, ratio=FORCE)
        m.set_list_test(T_SMALL, 0)
        m.run(50)                                       # passes and builds after 16 and 48 rows
        lst = m.list_stats()
        assert lst["builds"] == 2 and lst["valid"] == 1 and [b["iter"] for b in lst["log"]] == [16, 48], lst
        assert lst["log"][1]["entries"] < lst["log"][0]["entries"]
        m.reset()
        lst = m.list_stats()
        assert lst["builds"] == 0 and lst["valid"] == 0 and lst["build_bytes"] == 0
        got = m.run(n_samp)
        exp = ou.c_greedy(cols, n_var, state)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist()
        assert m.list_stats()["builds"] >= 3
        assert (m.covered(c) == covered_of(cols, state, got[0])).all()
        m.set_list_mode(0)                              # switching off drops the list, not the view
        assert m.list_stats()["valid"] == 0 and m.list_stats()["mode"] == 0


def test_lists_read_fewer_bytes_than_the_bitmap_view(dev):
    rng = np.random.default_rng(31)
    n_var, n_samp = 70_000, 300
    dense = ou.random_dense(rng, n_var, n_samp, density=0.002, sfs=False)   # a column: ~370 carriers in 8.75 KB of bitmap
    on, _, lst = run_lists(dev, dense, between=False, ratio=0.0)             # (the library's ratio; boundaries after 16, 48, 112, 240 rows)
    off, _, lst_off = run_lists(dev, dense, between=False, list_mode=0)
    assert lst["builds"] >= 3 and lst["ratio"] == 2.0 and lst_off["builds"] == 0, lst
    assert on["algo_bytes"] < off["algo_bytes"] and on["brute_force_bytes"] == off["brute_force_bytes"], (on, off)
    assert on["persist_launches"] == 0 or on["persist_iterations"] <= 16    # the list phase runs one launch per iteration


@pytest.mark.parametrize("n_var,n_samp", [(2_000_000, 500), (1_100_000, 2_504)])
def test_the_default_gate_keeps_small_matrices_on_the_parents_path(dev, n_var, n_samp):
    seen = []
    for mode in (1, 0):
        with dev.DeviceMatrix(n_samp) as m:
            c = m.add_chunk(n_var)
            m.synth_fill(c, seed=1)
            if mode == 0:
                m.set_list_mode(0)
            got = m.run(40)
            st, cst, lst = m.stats(), m.compaction_stats(), m.list_stats()
            assert lst["builds"] == 0 and lst["refused"] == 0 and lst["min_stream_bytes"] == 1 << 30, lst
            seen.append((got[0].tolist(), got[1].tolist(), st["score_launches"], st["persist_launches"], st["persist_iterations"],
                         st["algo_bytes"], cst["compactions"]))
    assert seen[0] == seen[1]
