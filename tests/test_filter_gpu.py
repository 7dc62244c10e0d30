"""GPU: variant filters (utm_filter_variants: k_filter_prefix + k_filter_compact).

The compacted columns have to equal the numpy restatement (tests/filter_ref.py: dense[keep], packed again) and the CPU
build of the same word arithmetic bit for bit, and everything that runs afterwards has to equal its oracle on dense[keep]:
the greedy rows and float64 scores, the first iteration's score vector, depth planes, capture ranks, var_count."""
import ctypes

import numpy as np
import pytest

import depth_ref
import filter_ref
import oracle_util as ou
import rank_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


_MATRIX = {}


def matrix(n_var, n_samp):
    if (n_var, n_samp) not in _MATRIX:
        dense = ou.random_dense(np.random.default_rng(7 * n_var + n_samp), n_var, n_samp, density=0.4, sfs=n_var % 2 == 0)
        _MATRIX[(n_var, n_samp)] = (dense, npo.pack_columns(dense))
    return _MATRIX[(n_var, n_samp)]


def host_filter(cols, n_var, keep):
    from utmos_amd import _native as nat
    wp_out = (int(keep.sum()) + 63) // 64
    out = np.zeros((cols.shape[0], wp_out), dtype=np.uint64)
    words = filter_ref.pack_keep(keep)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_filter_columns_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(words), p(out), wp_out, None))
    return out


def context(dev, dense, chunk_vars=None, af=None):
    n_var, n_samp = dense.shape
    m = dev.DeviceMatrix(n_samp)
    lo = 0
    for n in chunk_vars or [n_var]:
        c = m.add_chunk(n)
        m.upload_columns(c, npo.pack_columns(dense[lo:lo + n]))
        if af is not None:
            m.set_af(c, af[lo:lo + n])
        lo += n
    return m


@pytest.mark.parametrize("n_samp", [70, 300])
@pytest.mark.parametrize("n_var", filter_ref.SIZES)
def test_compacted_columns_equal_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    dense, cols = matrix(n_var, n_samp)
    for name, keep in filter_ref.mask_cases(n_var).items():
        with dev.DeviceMatrix(n_samp) as m:
            c = m.add_chunk(n_var)
            m.upload_columns(c, cols)
            kept = m.filter_variants(c, keep)
            assert kept == int(keep.sum()) and m.chunk_vars == [kept] and m.shape == (kept, n_samp), name
            got = m.download_columns(c)
            want, _ = filter_ref.filter_columns(cols, n_var, keep)
            assert got.shape == want.shape and (got == want).all(), name      # (the last word's padding bits included)
            assert (got == host_filter(cols, n_var, keep)).all(), name
            assert (m.var_count() == dense[keep].sum(axis=0)).all(), name
            if name == "ones":
                assert (got == cols).all()


def test_garbage_above_n_var_and_pass_ms(dev):
    from utmos_amd import _native as nat
    n_var, n_samp = 8191, 70
    dense, cols = matrix(n_var, n_samp)
    keep = filter_ref.mask_cases(n_var)["random0.5"]
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        words = filter_ref.pack_keep(keep, garbage=True)
        kept, ms = ctypes.c_uint64(0), ctypes.c_double(-1.0)
        nat.check(nat.lib().utm_filter_variants(m._h, c, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(kept), ctypes.byref(ms)))
        assert kept.value == int(keep.sum()) and ms.value > 0
        m.chunk_vars[c] = int(kept.value)
        assert (m.download_columns(c) == filter_ref.filter_columns(cols, n_var, keep)[0]).all()


def test_three_chunks_with_masks_of_their_own_one_emptied_then_filtered_again(dev):
    n_samp, chunk_vars = 70, [8193, 700, 32769]
    dense, _ = matrix(sum(chunk_vars), n_samp)
    rng = np.random.default_rng(5)
    masks = [rng.random(chunk_vars[0]) < 0.5, np.zeros(chunk_vars[1], bool), rng.random(chunk_vars[2]) < 0.08]
    bounds = np.cumsum([0] + chunk_vars)
    with context(dev, dense, chunk_vars) as m:
        for c, mask in enumerate(masks):
            assert m.filter_variants(c, mask) == int(mask.sum())
        assert m.chunk_vars == [int(mask.sum()) for mask in masks] and m.chunk_vars[1] == 0
        parts = [dense[bounds[c]:bounds[c + 1]][masks[c]] for c in range(3)]
        for c in range(3):
            assert (m.download_columns(c) == (npo.pack_columns(parts[c]) if len(parts[c]) else np.zeros((n_samp, 0), np.uint64))).all()
        left = np.concatenate(parts)
        state = np.ones(n_samp, np.uint8)
        want = depth_ref.greedy(left, state.copy(), n_samp)
        idx, new, _ = m.run(n_samp)
        assert idx.tolist() == [r[0] for r in want] and new.tolist() == [r[1] for r in want]
        assert (m.var_count() == left.sum(axis=0)).all()
        # filtering twice equals filtering once with the composed mask; the emptied chunk takes an empty mask
        again = [rng.random(len(parts[0])) < 0.6, np.zeros(0, bool), rng.random(len(parts[2])) < 0.5]
        for c, mask in enumerate(again):
            assert m.filter_variants(c, mask) == int(mask.sum())
        for c in (0, 2):
            composed = masks[c].copy()
            composed[np.flatnonzero(masks[c])[~again[c]]] = False
            once, _ = filter_ref.filter_columns(npo.pack_columns(dense[bounds[c]:bounds[c + 1]]), chunk_vars[c], composed)
            assert (m.download_columns(c) == once).all()
        left = np.concatenate([parts[0][again[0]], parts[2][again[2]]])
        want = depth_ref.greedy(left, state.copy(), n_samp)
        idx, new, _ = m.run(n_samp)
        assert idx.tolist() == [r[0] for r in want] and new.tolist() == [r[1] for r in want]


def hexes(values):
    return [float(v).hex() for v in values]


@pytest.mark.parametrize("kind", [None, "f32", "f64w"])
def test_everything_downstream_equals_its_oracle_on_the_kept_rows(dev, kind):
    n_samp, chunk_vars = 70, [8193, 5000]
    n_var = sum(chunk_vars)
    dense, _ = matrix(n_var, n_samp)
    rng = np.random.default_rng(11)
    af = np.round(rng.random(n_var) * 0.5, 4) + 1e-4
    af[rng.choice(n_var, 50, replace=False)] = 0.0                # AF == 0 rows are cleared: among the kept and the dropped
    af = af.astype(np.float32) if kind == "f32" else af
    keep = rng.random(n_var) < 0.4
    weights = rng.uniform(0.5, 2.0, n_samp) if kind == "f64w" else None
    state = np.ones(n_samp, np.uint8)
    state[[3, 40]] = 2
    state[7] = 0
    left = dense[keep]
    scored = left if kind is None else left * af[keep][:, None]
    with context(dev, dense, chunk_vars) as m:
        m.filter_variants(0, keep[:chunk_vars[0]])
        m.filter_variants(1, keep[chunk_vars[0]:])
        assert (m.var_count() == left.sum(axis=0)).all()
        if kind is not None:
            lo = 0
            for c, n in enumerate(m.chunk_vars):
                m.set_af(c, af[keep][lo:lo + n])
                lo += n
        m.set_state(state)
        m.set_weights(weights)
        m.reset()
        _, _, want_scores = depth_ref.calculate_scores(scored, state, weights)
        counts, scores = m.peek_scores()
        assert scores.tolist() == want_scores.tolist()            # the AF values went with their rows
        want = depth_ref.greedy(scored, state.copy(), n_samp, weights)
        idx, new, score = m.run(n_samp)
        assert idx.tolist() == [r[0] for r in want] and new.tolist() == [r[1] for r in want]
        assert hexes(score) == hexes(r[2] for r in want)
        m.set_decremental(True)
        m.reset()
        idx2, new2, _ = m.run(n_samp)
        assert idx2.tolist() == idx.tolist() and new2.tolist() == new.tolist()
        m.set_decremental(False)
        # depth 2, and the capture ranks of that order
        m.set_depth(2)
        m.reset()
        want2 = depth_ref.greedy(scored, state.copy(), n_samp, weights, 2)
        idx3, new3, score3 = m.run(n_samp)
        assert idx3.tolist() == [r[0] for r in want2] and new3.tolist() == [r[1] for r in want2] and hexes(score3) == hexes(r[2] for r in want2)
        assert m.at_depth(0, len(idx3)).tolist() == [r[3] for r in want2]
        ranks = np.concatenate([m.capture_rank(c, idx3, 2) for c in range(2)])
        assert (ranks == rank_ref.capture_rank(npo.pack_columns(scored != 0), idx3, 2, len(scored))).all()


def test_af_set_before_the_filter_is_gathered_with_the_rows(dev):
    n_samp, n_var = 70, 8193
    dense, _ = matrix(n_var, n_samp)
    rng = np.random.default_rng(13)
    for dtype in (np.float32, np.float64):
        af = (rng.random(n_var) * 0.5 + 1e-3).astype(dtype)
        keep = rng.random(n_var) < 0.3
        state = np.ones(n_samp, np.uint8)
        with context(dev, dense, af=af) as m:
            m.run(3)
            m.filter_variants(0, keep)
            scored = dense[keep] * af[keep][:, None]
            _, _, want_scores = depth_ref.calculate_scores(scored, state)
            assert m.peek_scores()[1].tolist() == want_scores.tolist()
            want = depth_ref.greedy(scored, state.copy(), n_samp)
            idx, new, score = m.run(n_samp)
            assert idx.tolist() == [r[0] for r in want] and hexes(score) == hexes(r[2] for r in want)


def test_a_filter_in_the_middle_of_a_run_restarts_it(dev):
    n_samp, n_var = 70, 32769
    dense, _ = matrix(n_var, n_samp)
    keep = filter_ref.mask_cases(n_var)["random0.5"]
    state = np.ones(n_samp, np.uint8)
    state[[1, 2]] = 2
    state[10] = 0
    with context(dev, dense) as m:
        m.set_state(state)
        m.reset()
        for _ in range(5):
            assert m.step() is not None
        m.filter_variants(0, keep)
        want = depth_ref.greedy(dense[keep], state.copy(), n_samp)
        idx, new, _ = m.run(n_samp)
        assert idx.tolist() == [r[0] for r in want] and new.tolist() == [r[1] for r in want]
        assert m.stats()["iterations"] == len(want)


def test_refusals(dev):
    from utmos_amd import _native as nat
    dense, cols = matrix(65, 70)
    keep = np.ones(65, bool)
    with dev.DeviceMatrix(70) as m:
        c = m.add_chunk(65)
        m.upload_columns(c, cols)
        words = filter_ref.pack_keep(keep)
        p = words.ctypes.data_as(ctypes.c_void_p)
        assert nat.lib().utm_filter_variants(m._h, 1, p, None, None) == EINVAL
        assert nat.lib().utm_filter_variants(m._h, -1, p, None, None) == EINVAL
        assert nat.lib().utm_filter_variants(m._h, 0, None, None, None) == EINVAL
        assert nat.lib().utm_filter_variants(None, 0, p, None, None) == EINVAL
        with pytest.raises(ValueError):
            m.filter_variants(0, np.ones(64, bool))
        with pytest.raises(ValueError):
            m.filter_variants(0, np.ones(65, np.uint8))
        assert m.filter_variants(0, keep) == 65 and (m.download_columns(0) == cols).all()
    # a shard before its exchange is set up may be filtered; afterwards the peers have mapped the old column bases
    with dev.DeviceMatrix(70, first_sample=10, n_local=30) as m:
        c = m.add_chunk(65)
        m.upload_columns(c, cols[10:40])
        half = np.arange(65) % 2 == 0
        assert m.filter_variants(0, half) == 33
        assert (m.download_columns(0) == filter_ref.filter_columns(cols[10:40], 65, half)[0]).all()
    with dev.DeviceMatrix(70) as m:
        c = m.add_chunk(65)
        m.upload_columns(c, cols)
        m.p2p_import(0, [m.p2p_export()])
        with pytest.raises(nat.NativeError) as e:
            m.filter_variants(0, np.arange(65) % 2 == 0)
        assert e.value.code == ESTATE and m.chunk_vars == [65]
        assert (m.download_columns(0) == cols).all()
