"""Replicated selection without a GPU: the CPU build of the kernels' arithmetic (utm_multi_select_host, utm_multi_keep_host)
against the numpy restatement (multi_ref.py), the reference's traces, stability.py's pure functions and the command's refusals."""
import ctypes
import os

import numpy as np
import pytest

import multi_ref
import oracle_util as ou
from multi_ref import family_keep, host_select, same

npo = ou.npo


@pytest.mark.parametrize("n_samp", [1, 17, 70])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 1000])
def test_cpu_build_equals_the_restatement(n_var, n_samp):
    rng = np.random.default_rng(n_var * 131 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    for n_rep in (1, 2, 63, 64, 65):
        states = multi_ref.mixed_states(rng, n_rep, n_samp)
        keep = family_keep(rng, n_rep, n_var)
        if n_rep >= 4:
            keep[0] = rng.random(n_var) < 0.5                        # (a half with every sample selectable too)
        k = n_samp + 2                                               # above the number of selectable samples
        want = multi_ref.select(dense, states, keep, k)
        same(host_select(dense, states, keep, k), want, n_rep)
        same(multi_ref.select_batched(dense, states, keep, k), want, ("batched", n_rep))
        assert (want[2] == keep.sum(axis=1)).all()
        short = max(1, n_samp // 3)
        same(host_select(dense, states, keep, short), multi_ref.select(dense, states, keep, short), ("short", n_rep))


def test_k_zero_and_bits_above_n_var_and_a_wide_stride():
    rng = np.random.default_rng(5)
    dense = ou.random_dense(rng, 100, 9)
    states = multi_ref.mixed_states(rng, 3, 9)
    keep = rng.random((3, 100)) < 0.5
    order, new, kept, done = host_select(dense, states, keep, 0)
    assert order.shape == (3, 0) and kept.tolist() == keep.sum(axis=1).tolist() and done.tolist() == [0, 0, 0]
    # garbage above n_var in the last keep word is ignored; the column stride may exceed the words in use
    from utmos_amd import _native as nat
    cols = np.zeros((9, 5), dtype=np.uint64)
    cols[:, :2] = npo.pack_columns(dense)
    words = multi_ref.pack_keep(keep)
    words[:, 1] |= np.uint64(0xFFFFFFF000000000)
    outs = [np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_multi_select_host(p(cols), 5, 100, 9, 3, p(states), p(words), 4, *[p(o) for o in outs]))
    same(outs, multi_ref.select(dense, states, keep, 4))


def test_duplicate_columns_the_smaller_index_wins():
    rng = np.random.default_rng(11)
    dense = ou.random_dense(rng, 200, 12)
    dense[:, 9] = dense[:, 3]
    dense[:, 5] = dense[:, 3]
    dense[:, 3] |= rng.random(200) < 0.6                             # make the triple the best columns
    dense[:, 5] = dense[:, 9] = dense[:, 3]
    states = np.ones((2, 12), dtype=np.uint8)
    states[1, 3] = 2                                                 # without the first of them: the next smaller index
    keep = np.ones((2, 200), dtype=bool)
    order, new, kept, done = host_select(dense, states, keep, 3)
    assert order[0, 0] == 3 and order[1, 0] == 5
    same((order, new, kept, done), multi_ref.select(dense, states, keep, 3))


def test_replicates_stop_at_different_rows():
    # sample s alone carries the variants of block s; replicate b keeps the blocks below b: it stops after b rows
    n_samp = 6
    dense = np.zeros((n_samp * 10, n_samp), dtype=bool)
    for s in range(n_samp):
        dense[s * 10:(s + 1) * 10, s] = True
    dense[:, 0] |= np.arange(n_samp * 10) % 10 == 0                  # sample 0 also carries one variant of every block
    keep = np.zeros((n_samp + 1, n_samp * 10), dtype=bool)
    for b in range(n_samp + 1):
        keep[b, :b * 10] = True
    states = np.ones((n_samp + 1, n_samp), dtype=np.uint8)
    got = host_select(dense, states, keep, n_samp)
    want = multi_ref.select(dense, states, keep, n_samp)
    same(got, want)
    assert got[3].tolist() == list(range(n_samp + 1))                # the capture of the last kept variant ends a replicate
    states[:, 2] = 2                                                 # block 2 can never be captured: best score 0 ends it
    got = host_select(dense, states, keep, n_samp)
    same(got, multi_ref.select(dense, states, keep, n_samp))
    assert got[3].tolist() == [0, 1, 2, 2, 3, 4, 5]
    assert (got[0][3, 2:] == -1).all() and (got[1][3, 2:] == 0).all()


def test_hashed_masks_on_the_host():
    from utmos_amd import _native as nat
    from utmos_amd.stability import keep_threshold
    lib = nat.lib()
    for seed, first, n_var, fraction in ((0, 0, 1, 0.5), (7, 0, 64, 0.5), (7, 0, 65, 0.25), (2 ** 64 - 3, 12345, 1000, 0.5),
                                         (99, 2 ** 33 + 5, 130, 0.9), (3, 77, 500, 1.0)):
        thr = keep_threshold(fraction)
        want = multi_ref.hashed_keep(seed, 5, n_var, thr, first)
        for b in (0, 1, 4):
            words = np.full((n_var + 63) // 64, 0x5555555555555555, dtype=np.uint64)
            assert lib.utm_multi_keep_host(seed, b, first, n_var, thr, words.ctypes.data_as(ctypes.c_void_p)) == 0
            assert np.array_equal(words, multi_ref.pack_keep(want[b:b + 1])[0][:len(words)]), (seed, first, n_var, b)
        for v in (0, n_var - 1):
            assert bool(want[3, v]) == ((multi_ref.hash_one(seed, first + v, 3) >> 32) < thr)
        if fraction == 1.0:
            assert thr == 2 ** 32 and want.all()                     # a threshold of 2^32 keeps everything
    # a chunk that starts at a non-zero global index continues the mask of the chunk before it
    whole = multi_ref.hashed_keep(1, 3, 300, keep_threshold(0.5))
    assert np.array_equal(whole[:, 100:], multi_ref.hashed_keep(1, 3, 200, keep_threshold(0.5), 100))
    share = multi_ref.hashed_keep(4, 8, 20000, keep_threshold(0.5)).mean()
    assert 0.49 < share < 0.51
    assert lib.utm_multi_keep_host(0, 0, 0, 10, 1, None) == -1


def test_argument_errors_leave_the_outputs_untouched():
    from utmos_amd import _native as nat
    lib = nat.lib()
    dense = ou.random_dense(np.random.default_rng(1), 70, 5)
    cols = npo.pack_columns(dense)
    words = np.full((2, 2), 2 ** 64 - 1, dtype=np.uint64)
    states = np.ones((2, 5), dtype=np.uint8)
    outs = [np.full((2, 3), 9, np.int32), np.full((2, 3), 9, np.int64), np.full(2, 9, np.int64), np.full(2, 9, np.int64)]
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    call = lambda n_rep, st, kw, k, o: lib.utm_multi_select_host(p(cols), 2, 70, 5, n_rep, p(st), p(kw), k, *[p(x) for x in o])
    bad_state = states.copy()
    bad_state[1, 4] = 3
    assert call(0, states, words, 3, outs) == -1 and call(257, states, words, 3, outs) == -1
    assert call(2, states, words, -1, outs) == -1
    assert call(2, bad_state, words, 3, outs) == -1 and b"state" in lib.utm_last_error()
    assert call(2, None, words, 3, outs) == -1 and call(2, states, None, 3, outs) == -1
    for i in range(4):
        assert call(2, states, words, 3, outs[:i] + [None] + outs[i + 1:]) == -1
    assert all((o == 9).all() for o in outs)
    assert call(2, states, words, 3, outs) == 0 and outs[2].tolist() == [70, 70]
    assert lib.utm_multi_select(None, 1, None, None, 0, 0, 1, None, None, None, None, None) == -1


def integer_traces():
    names = []
    for name in ou.trace_names():
        t = ou.load_trace(name)
        if "idx" not in t or "tsv" not in t or "weight_vector_hex" in t:
            continue
        kw = ou.trace_options(t)
        if kw.get("af") or kw.get("weights"):
            continue
        names.append(name)
    return names


@pytest.mark.parametrize("name", integer_traces())
def test_every_replicate_with_all_variants_reproduces_the_reference_trace(name):
    t = ou.load_trace(name)
    kw = ou.trace_options(t)
    dense, _, samples = npo.build_matrix(t["part_list"])
    state = np.array(t["state"], dtype=np.uint8) if "state" in t else npo.initial_state(samples, kw.get("subset"), kw.get("exclude"))
    k = npo.resolve_count(len(samples), kw.get("count", 0.02))
    want_new = [int(ln.split("\t")[2]) for ln in t["tsv"].splitlines()[1:]]
    assert len(want_new) == len(t["idx"])
    n_rep = 3
    order, new, kept, done = host_select(dense, np.tile(state, (n_rep, 1)), np.ones((n_rep, dense.shape[0]), dtype=bool), k)
    for b in range(n_rep):
        assert done[b] == len(t["idx"]) and kept[b] == dense.shape[0]
        assert order[b, :done[b]].tolist() == t["idx"] and new[b, :done[b]].tolist() == want_new
        assert (order[b, done[b]:] == -1).all() and (new[b, done[b]:] == 0).all()


def test_the_integer_traces_are_found():
    names = integer_traces()
    assert {"ties_int", "tiny_all", "initial_used_int", "mid_int", "zero_score_stop", "all_excluded"} <= set(names)


# ----------------------------------------------------------------- stability.py
def test_keep_threshold():
    from utmos_amd.stability import keep_threshold
    assert keep_threshold(0.5) == 2 ** 31 and keep_threshold(1.0) == 2 ** 32 and keep_threshold(1e-10) == 0
    assert keep_threshold(0.3) == int(np.floor(0.3 * 2 ** 32))
    for bad in (0.0, -0.1, 1.0001):
        with pytest.raises(ValueError):
            keep_threshold(bad)


def test_selection_table_by_hand():
    from utmos_amd.stability import selection_table
    names = ["a", "b", "c", "d", "e"]
    order = np.array([[2, 0, 3], [0, 2, -1], [2, 3, 0]], dtype=np.int32)
    n_done = [3, 2, 3]
    # c: 3 replicates, rows 1, 2, 1; a: 3 replicates, rows 2, 1, 3; d: 2 replicates, rows 3, 2; e: the panel only
    table = selection_table(order, n_done, names, [2, 4])
    assert table[:3] == [["c", 3, 1.0, 1.33, 1], ["a", 3, 1.0, 2.0, 0], ["d", 2, 0.6667, 2.5, 0]]
    assert table[3][:3] == ["e", 0, 0.0] and np.isnan(table[3][3]) and table[3][4] == 1 and len(table) == 4
    # equal counts and equal mean ranks: the sample index decides
    tie = selection_table(np.array([[1, 0], [0, 1]]), [2, 2], names, [])
    assert [r[0] for r in tie] == ["a", "b"] and tie[0][1:] == [2, 1.0, 1.5, 0]
    # the unrounded mean decides before the rounded one would call it a tie
    order = np.full((300, 2), -1, dtype=np.int32)
    order[:, 0], order[:, 1] = 0, 1
    order[0] = [1, 0]
    order[1] = [1, 0]
    order[2, 1] = -1                                                 # b: 299 times, a: 300 times
    table = selection_table(order, [2, 2, 1] + [2] * 297, names, [])
    assert [r[0] for r in table] == ["a", "b"]


def test_curve_band_by_hand():
    from utmos_amd.stability import curve_band
    new = np.array([[2, 1, 1], [4, 0, 0], [0, 0, 0]])
    mean, low, high = curve_band(new, [4, 8, 0])
    assert np.allclose(mean, [(0.5 + 0.5 + 0) / 3, (0.75 + 0.5 + 0) / 3, (1.0 + 0.5 + 0) / 3])
    assert low.tolist() == [0.0, 0.0, 0.0] and high.tolist() == [0.5, 0.75, 1.0]
    mean, low, high = curve_band(new[:2], [4, 8])
    assert low.tolist() == [0.5, 0.5, 0.5]                           # the replicate that stopped early carries its last value
    assert [len(x) for x in curve_band(np.zeros((2, 0)), [1, 1])] == [0, 0, 0]


def test_writers(tmp_path):
    from utmos_amd import stability
    order = np.array([[1, 0], [1, -1]], dtype=np.int32)
    new = np.array([[3, 1], [2, 0]])
    result = (order, new, np.array([4, 2]), np.array([2, 1]))
    stability.write_table(str(tmp_path / "s.tsv"), stability.selection_table(order, result[3], ["x", "y"], [1]))
    assert open(tmp_path / "s.tsv").read() == "sample\tselected\tfrequency\tmean_rank\tin_panel\ny\t2\t1.0\t1.0\t1\nx\t1\t0.5\t2.0\t0\n"
    stability.write_replicates(str(tmp_path / "r.npz"), result, ["x", "y"], [1], 5, 0.5)
    z = np.load(tmp_path / "r.npz")
    assert sorted(z.files) == sorted(["order", "new", "kept", "n_done", "pct_mean", "pct_min", "pct_max", "samples", "panel", "seed",
                                      "fraction"])
    assert z["pct_min"].tolist() == [0.75, 1.0] and z["pct_max"].tolist() == [1.0, 1.0] and int(z["seed"]) == 5
    assert z["samples"].tolist() == ["x", "y"] and z["panel"].tolist() == [1] and float(z["fraction"]) == 0.5


# ----------------------------------------------------------------- the command's refusals
PART = os.path.join(ou.GOLD, "chunk0.npz")


def refused(capsys, argv):
    from utmos_amd.select import parse_args
    with pytest.raises(SystemExit) as err:
        parse_args(argv)
    assert err.value.code == 1
    return capsys.readouterr().err


@pytest.mark.parametrize("flags, named", [
    (["--af"], "--af"), (["--weights", "w.tsv"], "--weights"), (["--depth", "2"], "--depth"), (["--mode", "topN"], "--mode topN"),
    (["--mode", "random"], "--mode random"), (["--refine", "3"], "--refine"), (["--groups", "g.tsv"], "--groups"),
    (["--include", "a,b"], "--include")])
def test_replicates_refuse_what_they_do_not_restate(capsys, flags, named):
    text = refused(capsys, ["--replicates", "8", PART] + flags)
    line = [ln for ln in text.splitlines() if "ERROR" in ln][-1]
    assert "--replicates" in line and named in line


@pytest.mark.parametrize("flags, named", [(["--replicates-out", "r.npz"], "--replicates-out"), (["--stability-out", "s.tsv"], "--stability-out"),
                                          (["--subsample", "0.3"], "--subsample")])
def test_the_out_flags_need_replicates(capsys, flags, named):
    line = [ln for ln in refused(capsys, [PART] + flags).splitlines() if "ERROR" in ln][-1]
    assert "--replicates" in line and named in line


@pytest.mark.parametrize("flags", [["--replicates", "0"], ["--replicates", "257"], ["--replicates", "4", "--subsample", "0"],
                                   ["--replicates", "4", "--subsample", "1.5"]])
def test_values_out_of_range(capsys, flags):
    assert "ERROR" in refused(capsys, [PART] + flags)


def options_line(capsys, argv):
    from utmos_amd.select import parse_args
    parse_args(argv)
    return [ln for ln in capsys.readouterr().err.splitlines() if "options in effect" in ln][-1]


def test_options_line(capsys):
    line = options_line(capsys, [PART])
    for name in ("replicates", "subsample", "replicates_out", "stability_out"):
        assert name not in line
    line = options_line(capsys, [PART, "--replicates", "16", "--subsample", "0.25", "--replicates-out", "r.npz", "--stability-out", "s.tsv"])
    assert '"replicates": 16' in line and '"subsample": 0.25' in line and '"replicates_out": "r.npz"' in line and '"stability_out": "s.tsv"' in line
    line = options_line(capsys, [PART, "--replicates", "16"])
    assert '"replicates": 16' in line and "subsample" not in line and "replicates_out" not in line


def test_several_processes_and_af_stores_are_refused_before_loading(capsys, tmp_path, monkeypatch):
    from utmos_amd.select import select_main
    from utmos_amd.store import SUFFIX, StoreWriter
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as err:
        select_main(["--replicates", "4", PART])
    assert err.value.code == 1 and "--replicates" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "1")
    path = str(tmp_path / ("af" + SUFFIX))
    writer = StoreWriter(path, np.array(["a", "b"]), True)
    writer.add_chunk(3, np.array([[5], [3]], dtype=np.uint64), np.array([0.1, 0.2, 0.3], dtype=np.float32))
    writer.finish(np.array([2, 2], dtype=np.int64))
    with pytest.raises(SystemExit) as err:
        select_main(["--replicates", "4", path])
    text = capsys.readouterr().err
    assert err.value.code == 1 and "--replicates" in text and "--af" in text
