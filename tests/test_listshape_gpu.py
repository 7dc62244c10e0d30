"""The 16-lane form of the list launches (utmos_amd/csrc/list.hip.h, list_score_rows): a wave scores four positions of
act[] at once, one per row of 16 lanes, when a build's segments are short -- and the rules that choose it (list_policy.h:
list_lanes, list_group) with utm_set_list_shape / utm_get_list_shape.  Integer arithmetic: rows, new counts, scores,
get_covered and peek_scores are the packed C oracle's, exactly.  The shapes are those at which the row form can go wrong:
fewer selectable samples than a wave has rows, exactly one round of 16, one more, an end inside a wave's four rows, several
groups; four rows of one wave with segments of 0, 1, 5 and 1,300 entries (the batch loop runs to the longest), once with
the long one in the last selectable position; segments of exactly 64 quads and one past it; a pending winner at every
boundary; samples that start out used; chunks with a build refused; forced workgroup targets at either extreme, one of
them one group per tile, so that a workgroup walks 19 rounds and the loop's own read-ahead is what it scores."""
import numpy as np
import pytest

import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

T_SMALL = 13            # 8,192 positions per tile: the test-only tile
FORCE = 1e-9            # list ratio that lets every pass build
ROW_QUADS = 64          # list_policy.h: UTM_LIST_ROW_QUADS


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


def rule_lanes(build, listed):
    """list_lanes by hand: the build's mean segment (quads over tiles x listed columns) against one batch of a row."""
    return 16 if build["padded"] // 4 <= ROW_QUADS * build["tiles"] * listed else 64


def run_shape(dev, dense, lanes, target=0, state=None, weights=None, pieces=None, chunk_sizes=None, between=True, max_entries=0,
              profile=False, exp=None):
    """One selection with compaction, list mode and the launch shape forced, against the oracle at every boundary.
    -> (rows, stats, compaction stats, list stats, list shape)."""
    n_var, n_samp = dense.shape
    state = np.ones(n_samp, np.uint8) if state is None else state
    cols = npo.pack_columns(dense)
    exp = ou.c_greedy(cols, n_var, state, weights=weights) if exp is None else exp
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
        m.set_compaction(1, min_vars=1, ratio=0.99)
        m.set_list_mode(1, min_stream_bytes=1, ratio=FORCE)
        m.set_list_test(T_SMALL, max_entries)
        m.set_list_shape(lanes, target)
        if profile:
            m.set_profile(True)
        idx, new, score = [], [], []
        for piece in (pieces or [n_samp]):
            got = m.run(piece)
            idx += got[0].tolist()
            new += got[1].tolist()
            score += got[2].tolist()
            assert idx == exp[0][:len(idx)].tolist() and new == exp[1][:len(new)].tolist() and score == exp[2][:len(score)].tolist()
            if between and len(got[0]) == piece:        # (a run that has stopped scores nothing any more)
                want = covered_of(cols, state, idx)
                for c, (a, b) in enumerate(bounds):
                    assert (m.covered(c) == want[a // 64:(b + 63) // 64]).all(), c
                sel, cnt, sc = oracle_counts(cols, n_var, state, idx, weights)
                got_cnt, got_sc = m.peek_scores()
                assert (got_cnt[sel] == cnt[sel]).all() and (got_sc[sel] == sc[sel]).all()
        st, cst, lst, shape = m.stats(), m.compaction_stats(), m.list_stats(), m.list_shape()
        covered = [m.covered(c) for c in range(len(bounds))]
    assert idx == exp[0].tolist() and new == exp[1].tolist() and score == exp[2].tolist()
    want = covered_of(cols, state, idx)
    for c, (a, b) in enumerate(bounds):
        assert (covered[c] == want[a // 64:(b + 63) // 64]).all(), c
    assert st["tot_captured"] == sum(new)
    assert len(shape) == min(16, lst["builds"]) and all(b["t"] == T_SMALL for b in lst["log"])
    if lanes:
        assert all(s["lanes"] == lanes for s in shape), shape
    return (idx, new, score), st, cst, lst, shape


@pytest.mark.parametrize("n_var", [8_193, 70_000])
@pytest.mark.parametrize("n_samp", [3, 15, 16, 17, 37, 300])
def test_rows_of_16_lanes_give_the_oracles_rows_scores_and_masks(dev, n_var, n_samp):
    rng = np.random.default_rng(n_var * 7 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    # a pending winner sits at every boundary, and n_active passes through every residue of 16 as the run goes on
    _, _, cst, lst, shape = run_shape(dev, dense, 16, pieces=[1, 2, 17, n_samp])
    assert lst["builds"] >= 1 and lst["refused"] == 0 and cst["compactions"] >= lst["builds"], (cst, lst)
    assert all(s["wgs"] >= 1 for s in shape[:-1]), shape
    if n_var == 70_000:
        assert lst["log"][0]["tiles"] > 1, lst


def uneven_rows_matrix():
    """41 samples; sample 0 wins first and leaves a region of three whole tiles (so position p of act[] holds sample p
    for p >= 1, the last sample having moved to position 0).  Tile 0: samples 4 .. 7, the four rows of one wave, hold 0, 1,
    5 and 1,300 entries (six batches of a row).  Tile 1: the same for samples 36 .. 39, the long one in the last
    selectable position.  Tile 2: samples 12 .. 15 hold 256, 257, 260 and 512 entries: exactly 64 quads, 65, 65 and 128."""
    rng = np.random.default_rng(11)
    tile, n_samp = 1 << T_SMALL, 41
    region = 3 * tile
    n_var = region + 7_000
    dense = np.zeros((n_var, n_samp), bool)
    dense[region:region + 3_000, :] = True              # rows everybody carries ...
    dense[region + 3_000:, 0] = True                    # ... and sample 0's own: it wins first and leaves the region
    for v in range(region):                             # sparse carriers among samples 16 .. 35, every row informative
        dense[v, rng.integers(16, 36, 1 + (v % 3 == 0))] = True
    for t, first, counts in [(0, 4, [0, 1, 5, 1_300]), (1, 36, [0, 1, 5, 1_300]), (2, 12, [256, 257, 260, 512])]:
        for k, n in enumerate(counts):
            dense[t * tile + rng.choice(tile, n, replace=False), first + k] = True
    dense[tile + rng.choice(tile, 3, replace=False), 4] = True      # (no column is empty throughout)
    dense[rng.choice(tile, 3, replace=False), 36] = True
    return dense, region


def test_four_rows_of_one_wave_with_segments_as_uneven_as_they_get(dev):
    dense, region = uneven_rows_matrix()
    for lanes in (16, 64):
        _, _, cst, lst, shape = run_shape(dev, dense, lanes, pieces=[1, 1, 3, dense.shape[1]])
        assert cst["passes"][0][:2] == (1, region) and lst["log"][0]["iter"] == 1 and lst["log"][0]["tiles"] == 3, (cst, lst)
        assert lst["log"][0]["padded"] > lst["log"][0]["entries"] and shape[0]["lanes"] == lanes


@pytest.mark.parametrize("weighted", [False, True])
def test_samples_that_start_out_used_and_signed_weights_in_rows(dev, weighted):
    rng = np.random.default_rng(43)
    n_var, n_samp = 70_001, 131
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    first = int(ou.c_greedy(cols, n_var, np.ones(n_samp, np.uint8), k_max=1)[0][0])
    state = np.ones(n_samp, np.uint8)
    state[[first, 4, 77, 130]] = 0
    state[[9, 10]] = 2
    weights = rng.integers(-2, 4, n_samp).astype(np.float64) if weighted else None
    _, _, _, lst, _ = run_shape(dev, dense, 16, state=state, weights=weights, pieces=[1, 2, 3, 10, 32, n_samp])
    assert lst["builds"] >= 3 and lst["refused"] == 0, lst


def test_three_chunks_and_the_build_of_one_refused_in_rows(dev):
    rng = np.random.default_rng(19)
    sizes, n_samp = [64_000, 32_000, 16_000], 131
    dense = ou.random_dense(rng, sum(sizes), n_samp)
    exp = ou.c_greedy(npo.pack_columns(dense), sum(sizes), np.ones(n_samp, np.uint8))
    _, _, _, lst, _ = run_shape(dev, dense, 16, chunk_sizes=sizes, pieces=[4, n_samp], between=False, exp=exp)
    big, mid, small = (lst["log"][k]["padded"] for k in range(3))
    assert [lst["log"][k]["iter"] for k in range(3)] == [4, 4, 4] and small < mid < big, lst
    cap = (big + mid) // 2                              # between the first builds of the two longer chunks
    _, _, cst, lst, _ = run_shape(dev, dense, 16, chunk_sizes=sizes, pieces=[4, 12, 32, n_samp], max_entries=cap, exp=exp)
    assert lst["refused"] == 1 and lst["builds"] >= 4 and all(b["padded"] <= cap for b in lst["log"]), lst
    assert cst["compactions"] > lst["builds"]           # the refused chunk went on compacting its bitmap view


def test_both_forms_read_the_same_bytes_and_report_their_shape(dev):
    rng = np.random.default_rng(37)
    dense = ou.random_dense(rng, 70_000, 131)
    exp = ou.c_greedy(npo.pack_columns(dense), 70_000, np.ones(131, np.uint8))
    seen = {}
    for lanes in (64, 16):
        rows, st, _, lst, shape = run_shape(dev, dense, lanes, between=False, profile=True, exp=exp)
        assert lst["builds"] >= 3 and [s["lanes"] for s in shape] == [lanes] * len(shape), (lst, shape)
        seen[lanes] = (rows, st["algo_bytes"], st["score_launches"], [b["padded"] for b in lst["log"]])
    assert seen[64] == seen[16]


@pytest.mark.parametrize("density,first", [(0.002, 16), (0.5, 64)])
def test_the_rule_goes_by_the_mean_segment_of_the_build(dev, density, first):
    rng = np.random.default_rng(53)
    n_var, n_samp = 70_000, 300
    dense = ou.random_dense(rng, n_var, n_samp, density=density, sfs=False)
    # density 0.002: ~16 carriers of a column in a tile, 4 quads (a first pick covers too little for a pass: the first build
    # comes at the batch boundary); 0.5: the view after the first pick keeps ~35,000 variants, ~1,000 quads a segment
    _, _, _, lst, shape = run_shape(dev, dense, 0, pieces=[1, n_samp], between=False)
    # (at density 0.5 seventeen picks cover everything: the run may end before a second pass)
    assert lst["builds"] >= (1 if density == 0.5 else 2) and shape[0]["lanes"] == first, (lst, shape)
    if density == 0.5:
        assert lst["log"][0]["iter"] == 1 and lst["log"][0]["padded"] // 4 > 500 * lst["log"][0]["tiles"] * (n_samp - 1), lst
    for b, s in zip(lst["log"], shape):
        assert s["lanes"] == rule_lanes(b, n_samp - b["iter"]), (b, s)


@pytest.mark.parametrize("target", [64, 4_096])
def test_forced_workgroup_targets(dev, target):
    rng = np.random.default_rng(61)
    n_var, n_samp = 70_000, 300
    dense = ou.random_dense(rng, n_var, n_samp)
    _, _, _, lst, shape = run_shape(dev, dense, 16, target=target, pieces=[1, n_samp], between=False)
    assert lst["builds"] >= 2 and lst["log"][0]["iter"] == 1
    tiles, a = lst["log"][0]["tiles"], n_samp - 1
    rounds = -(-a // 16)
    # whole groups per tile; within the target plus rounding, or one round per group (more groups than the target asks for)
    assert shape[0]["wgs"] % tiles == 0 and tiles <= shape[0]["wgs"] <= tiles * rounds, (lst["log"][0], shape[0])
    assert shape[0]["wgs"] <= target + tiles or shape[0]["wgs"] == tiles * rounds, (lst["log"][0], shape[0])
    if target == 4_096:
        assert shape[0]["wgs"] == tiles * rounds        # at most 9 tiles x 19 rounds: below the target, so one round per group


@pytest.mark.parametrize("weighted", [False, True])
def test_one_group_per_tile_walks_many_rounds(dev, weighted):
    """A target at or below the tile count: one workgroup per tile walks all of act[], 19 rounds at 299 positions.  From its
    fourth round on a row scores a segment whose index the loop itself read ahead (the kernel's head loads only the first
    three), so this is the run that checks the steady state of the loop: rows at every piece, the masks and -- through
    peek_scores -- the counts by sample of the launch without a pick, plain and with signed weights."""
    rng = np.random.default_rng(71)
    n_var, n_samp = 70_000, 300
    dense = ou.random_dense(rng, n_var, n_samp)
    weights = rng.integers(-2, 4, n_samp).astype(np.float64) if weighted else None
    _, _, _, lst, shape = run_shape(dev, dense, 16, target=1, weights=weights, pieces=[1, 2, 17, 100, n_samp])
    assert lst["builds"] >= 3 and lst["refused"] == 0 and lst["log"][0]["iter"] == 1 and lst["log"][0]["tiles"] > 1, lst
    for b, sh in zip(lst["log"], shape):
        assert sh["wgs"] in (0, b["tiles"]), (b, sh)    # (0: a build at the run's last boundary has had no launch)
    assert shape[0]["wgs"] == lst["log"][0]["tiles"] and n_samp - 1 > 4 * 16


def test_values_out_of_range_are_refused_and_change_nothing(dev):
    rng = np.random.default_rng(67)
    dense = ou.random_dense(rng, 8_193, 37)
    cols = npo.pack_columns(dense)
    exp = ou.c_greedy(cols, 8_193, np.ones(37, np.uint8))
    bad = [(7, 0), (32, 0), (-16, 0), (16, -1), (16, 65_537), (0, 1 << 20), (64, 65_537), (7, 4_096)]
    with dev.DeviceMatrix(37) as m:
        c = m.add_chunk(8_193)
        m.upload_columns(c, cols)
        m.set_compaction(1, min_vars=1, ratio=0.99)
        m.set_list_mode(1, min_stream_bytes=1, ratio=FORCE)
        m.set_list_test(T_SMALL, 0)
        seen = []
        for lanes, target in [(64, 0), (16, 1), (16, 65_536)]:    # (the ends of the target's range are taken)
            m.set_list_shape(lanes, target)
            for refused in (False, True):
                if refused:                             # neither the lanes nor the target may move
                    for args in bad:
                        with pytest.raises(Exception):
                            m.set_list_shape(*args)
                m.reset()
                got = m.run(37)
                assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist() and got[2].tolist() == exp[2].tolist()
                seen.append(m.list_shape())
            assert seen[-1] == seen[-2] and len(seen[-1]) >= 1 and all(sh["lanes"] == lanes for sh in seen[-1]), seen[-2:]
        # one tile, 21 positions at the build after 16 rows: one group at target 1, one per round of 16 at 65,536
        assert seen[3][0]["wgs"] == 1 and seen[5][0]["wgs"] > 1, seen
