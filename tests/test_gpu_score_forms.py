"""The two forms of the integer scoring launch at 32 and 16 KiB tiles (UTM_SCORE_FORM): 0 = k_score_int (the tile's
~covered words staged in LDS), 1 = k_score_intq (each wave keeps a quarter of the tile in registers).  Both against the
OpenMP C oracle and against each other: short last tiles, groups of 4 and of many samples (several rounds of partials,
a last group that ends part-way), every fused form of the launch (pick inside: 1, one-rank mailboxes: 2, k_pick behind:
0 -- weights, decremental full passes by sample, the earlier chunks of a multi-chunk matrix), the bounded wait for a
withheld partial, and the production shape."""
import numpy as np
import pytest

import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

KIB_VARS = 8192  # variants per KiB of a column


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def _launch_env(monkeypatch, form, steps, target_wgs=None):
    monkeypatch.setenv("UTM_SCORE_FORM", str(form))
    monkeypatch.setenv("UTM_TILE_STEPS", str(steps))
    monkeypatch.setenv("UTM_PERSISTENT", "0")
    if target_wgs is None:
        monkeypatch.delenv("UTM_TARGET_WGS", raising=False)
    else:
        monkeypatch.setenv("UTM_TARGET_WGS", str(target_wgs))


def _run(dev, dense, state, k, weights=None, chunks=None, decremental=None, mailboxes=False):
    n_var, n_samp = dense.shape
    bounds = [0, n_var] if chunks is None else chunks
    with dev.DeviceMatrix(n_samp) as m:
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            c = m.add_chunk(hi - lo)
            m.upload_columns(c, npo.pack_columns(dense[lo:hi]))
        m.set_state(state)
        m.set_weights(weights)
        if decremental is not None:
            m.set_decremental(True, decremental)
        if mailboxes:  # the only shard exchanging through its own mailbox (bench.py --force-mailboxes): FUSED = 2
            m.p2p_import(0, [m.p2p_export()])
            assert m.p2p_selftest()
            m.p2p_use_mailboxes("single")
        got = m.run(k)
    return got[0].tolist(), got[1].tolist(), got[2].tolist()


@pytest.mark.parametrize("steps", [32, 16])
@pytest.mark.parametrize("tail_kib", [1, 5, "full"])
def test_both_forms_match_the_oracle(dev, monkeypatch, steps, tail_kib):
    """Three tiles' worth of columns whose last tile holds 1 KiB, 5 KiB or all of its steps (minus a few variants of
    padding); 301 samples, some used.  Every launch form, both scoring forms, the oracle's rows."""
    tile_vars = steps * KIB_VARS
    n_var = 3 * tile_vars - 29 if tail_kib == "full" else 2 * tile_vars + tail_kib * KIB_VARS - 29
    n_samp, k = 301, 40
    rng = np.random.default_rng(steps * 10 + (0 if tail_kib == "full" else tail_kib))
    dense = ou.random_dense(rng, n_var, n_samp, density=0.02)
    state = np.ones(n_samp, np.uint8)
    state[rng.choice(n_samp, 12, replace=False)] = 2
    weights = rng.choice([0.5, 1.0, 1.0, 2.0], n_samp)
    cols = npo.pack_columns(dense)
    exp = ou.c_greedy(cols, n_var, state, k_max=k, omp=True)
    exp_w = ou.c_greedy(cols, n_var, state, weights, k_max=k, omp=True)
    exp_rows = (exp[0].tolist(), exp[1].tolist())
    exp_w_rows = (exp_w[0].tolist(), exp_w[1].tolist(), exp_w[2].tolist())
    split = tile_vars + 2 * KIB_VARS  # first chunk: a tile and a short one (FUSED = 0); the rest: the pick's chunk
    results = {}
    for form in (0, 1):
        for target in (None, 8):  # groups of 4 samples; groups of ~116 (two rounds of partials, a ragged last group)
            _launch_env(monkeypatch, form, steps, target)
            plain = _run(dev, dense, state, k)
            assert plain[:2] == exp_rows, (form, target, "plain")
            mbox = _run(dev, dense, state, k, mailboxes=True)
            assert mbox[:2] == exp_rows, (form, target, "mailboxes")
            chunked = _run(dev, dense, state, k, chunks=[0, split, n_var])
            assert chunked[:2] == exp_rows, (form, target, "chunks")
            decr = _run(dev, dense, state, k, decremental=0.0)  # full passes count by sample (by_pos = 0)
            assert decr[:2] == exp_rows, (form, target, "decremental")
            wtd = _run(dev, dense, state, k, weights=weights)
            assert wtd == exp_w_rows, (form, target, "weights")
            results[form, target] = (plain, mbox, chunked, decr, wtd)
    assert results[0, None] == results[1, None] and results[0, 8] == results[1, 8]


def test_withheld_partial_ends_in_an_error_under_register_quarters(dev, monkeypatch):
    """UTM_TEST_DROP_ARRIVAL under the register-quarter form: one (sample, tile) partial of block 0 is withheld, the
    fused pick's bounded wait runs out, the loop ends with UTM_EHIP, and after utm_reset the same context produces the
    oracle's rows."""
    rng = np.random.default_rng(18)
    n_var, n_samp = 2 * 16 * KIB_VARS + 3 * KIB_VARS, 120
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    exp = ou.c_greedy(cols, n_var, np.ones(n_samp, np.uint8))
    _launch_env(monkeypatch, 1, 16)
    monkeypatch.setenv("UTM_TEST_DROP_ARRIVAL", "5")
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.run(n_samp)
        assert e.value.code == -2 and "did not all arrive" in str(e.value)
        monkeypatch.setenv("UTM_TEST_DROP_ARRIVAL", "0")
        m.reset()
        got = m.run(n_samp)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()


def test_full_size_register_quarters(dev, monkeypatch):
    """10M variants x 2,504 samples (the flagship shape: 32 KiB tiles, groups of 4) under the register-quarter form:
    the first 24 rows from scratch, then the state after 1,252 selections (every selectable sample's count, the
    winner and the rows that follow), against the OpenMP C oracle on the matrix downloaded from the device."""
    from test_gpu_fullsize import check_late_state, download
    n_var, n_samp, k = 10_000_000, 2504, 1252
    monkeypatch.setenv("UTM_SCORE_FORM", "1")
    monkeypatch.setenv("UTM_PERSISTENT", "0")
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=5)
        cols = download(m, c)
        rows = m.run(k + 3)
        exp = ou.c_greedy(cols, n_var, np.ones(n_samp, np.uint8), k_max=24, omp=True)
        assert rows[0][:24].tolist() == exp[0].tolist() and rows[1][:24].tolist() == exp[1].tolist()
        check_late_state(m, cols, n_var, rows, k)
