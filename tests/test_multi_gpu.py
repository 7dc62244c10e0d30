"""GPU: the replicated selection (utm_multi_select: k_multi_keep, k_multi_init, k_multi_score, k_multi_pick, k_multi_apply).

Every replicate has to equal, bit for bit, the numpy restatement (tests/multi_ref.py) and the CPU build of the same
arithmetic; with all variants kept it has to equal utm_run on the same context, with a random mask a fresh matrix cut by
utm_filter_variants; and the call leaves nothing behind in the context."""
import ctypes
import os

import numpy as np
import pytest

import multi_ref
import oracle_util as ou
from oracle_util import npo
from multi_ref import family_keep, host_select, same

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
REPS = (1, 2, 63, 64, 65, 130)
SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def context(dev, dense, chunk_vars=None):
    n_var, n_samp = dense.shape
    m = dev.DeviceMatrix(n_samp)
    lo = 0
    for n in chunk_vars or [n_var]:
        c = m.add_chunk(n)
        m.upload_columns(c, npo.pack_columns(dense[lo:lo + n]))
        lo += n
    return m


def split(keep, chunk_vars):
    out, lo = [], 0
    for n in chunk_vars:
        out.append(np.ascontiguousarray(keep[:, lo:lo + n]))
        lo += n
    return out


# 32768 variants = one tile group boundary of nothing in particular but 64 tiles of 4 KiB; 32769 and 3 x 32768 + 5 leave a last
# tile with one wave at work; 8191 a last word with one bit missing; 1 and 65 a single KiB
@pytest.mark.parametrize("n_samp", [17, 70, 200])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 32768, 32769, 3 * 32768 + 5])
def test_abi_equals_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    from utmos_amd.stability import keep_threshold
    rng = np.random.default_rng(n_var * 7 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    top = max(REPS)
    states = multi_ref.mixed_states(rng, top, n_samp)
    k = min(n_samp, 12) if n_var <= 8191 else 4 if n_var <= 32769 else 3         # (rows enough for two k_multi_apply passes)
    masks = {"explicit": family_keep(rng, top, n_var), "hashed": multi_ref.hashed_keep(SEED, top, n_var, keep_threshold(0.5))}
    masks["explicit"][0] = rng.random(n_var) < 0.5
    # the restatement and the CPU build once for the largest B: replicate b is the same in every smaller B
    want = {mode: multi_ref.select_batched(dense, states, keep, k) for mode, keep in masks.items()}
    for mode, keep in masks.items():
        same(host_select(dense, states, keep, k), want[mode], ("cpu build", mode))
    with context(dev, dense) as m:
        for n_rep in REPS:
            cut = lambda outs: tuple(o[:n_rep] for o in outs)
            same(m.multi_select(k, states[:n_rep], keep=[masks["explicit"][:n_rep]]), cut(want["explicit"]), ("explicit", n_rep))
            same(m.multi_select(k, states[:n_rep], seed=SEED, fraction=0.5), cut(want["hashed"]), ("hashed", n_rep))
    assert want["hashed"][3].max() > 0 or n_var == 1


def test_two_chunks_the_hash_index_runs_across_them(dev):
    from utmos_amd.stability import keep_threshold
    rng = np.random.default_rng(21)
    chunk_vars = [4101, 5904]
    dense = ou.random_dense(rng, sum(chunk_vars), 40)
    states = multi_ref.mixed_states(rng, 5, 40)
    with context(dev, dense, chunk_vars) as m:
        for fraction in (0.5, 0.1, 1.0):
            keep = multi_ref.hashed_keep(9, 5, dense.shape[0], keep_threshold(fraction))
            want = multi_ref.select(dense, states, keep, 15)
            same(m.multi_select(15, states, seed=9, fraction=fraction), want, fraction)
            same(m.multi_select(15, states, keep=split(keep, chunk_vars)), want, ("explicit", fraction))
        keep = rng.random((5, dense.shape[0])) < 0.3
        keep[2, :chunk_vars[0]] = False                              # a replicate without a variant in the first chunk
        same(m.multi_select(15, states, keep=split(keep, chunk_vars)), multi_ref.select(dense, states, keep, 15), "random")


def test_all_variants_kept_equals_run_on_the_same_context(dev):
    rng = np.random.default_rng(22)
    dense = ou.random_dense(rng, 20000, 90)
    state = np.ones(90, dtype=np.uint8)
    state[[3, 50]] = 0                                               # used: cover from the start
    state[[7, 8, 60]] = 2                                            # excluded
    with context(dev, dense) as m:
        m.set_state(state)
        idx, new, _ = m.run(30)
        order, gains, kept, done = m.multi_select(30, state, keep=[np.ones((3, 20000), dtype=bool)], n_rep=3)
        threshold_all = m.multi_select(30, state, seed=5, fraction=1.0, n_rep=2)
    assert len(idx) == 30 and not set(idx.tolist()) & {3, 50, 7, 8, 60}
    for b in range(3):
        assert done[b] == 30 and kept[b] == 20000
        assert order[b].tolist() == idx.tolist() and gains[b].tolist() == new.tolist()
    assert threshold_all[0][1].tolist() == idx.tolist() and threshold_all[2].tolist() == [20000, 20000]


def test_a_random_mask_equals_a_fresh_filtered_matrix(dev):
    rng = np.random.default_rng(23)
    dense = ou.random_dense(rng, 30000, 64)
    states = multi_ref.mixed_states(rng, 4, 64)
    keep = rng.random((4, 30000)) < np.array([0.5, 0.5, 0.05, 0.9])[:, None]
    with context(dev, dense) as m:
        order, gains, kept, done = m.multi_select(20, states, keep=[keep])
    for b in range(4):
        with context(dev, dense) as fresh:
            assert fresh.filter_variants(0, keep[b]) == kept[b]
            fresh.set_state(states[b])
            idx, new, _ = fresh.run(20)
        assert done[b] == len(idx) and order[b, :done[b]].tolist() == idx.tolist() and gains[b, :done[b]].tolist() == new.tolist()


def test_staggered_early_stops(dev):
    n_samp = 70
    dense = np.zeros((n_samp * 10, n_samp), dtype=bool)
    for s in range(n_samp):
        dense[s * 10:(s + 1) * 10, s] = True
    dense[:, 0] |= np.arange(n_samp * 10) % 10 == 0
    keep = np.zeros((n_samp + 1, n_samp * 10), dtype=bool)
    for b in range(n_samp + 1):
        keep[b, :b * 10] = True                                      # replicate b ends after b rows: its last variant captured
    states = np.ones((n_samp + 1, n_samp), dtype=np.uint8)
    states[1::2, 2] = 2                                              # every other one cannot capture block 2: a best score of 0
    want = multi_ref.select(dense, states, keep, n_samp)
    assert len(set(want[3].tolist())) > 30
    with context(dev, dense) as m:
        got = m.multi_select(n_samp, states, keep=[keep])
        same(got, want)
        same(m.multi_select(n_samp + 50, states, keep=[keep]), multi_ref.select(dense, states, keep, n_samp + 50), "k above the samples")
        order, gains, kept, done = m.multi_select(0, states, keep=[keep])
        assert order.shape == (n_samp + 1, 0) and kept.tolist() == want[2].tolist() and not done.any()
    same(host_select(dense, states, keep, n_samp), want)


def test_the_call_leaves_the_context_as_it_was(dev):
    rng = np.random.default_rng(24)
    dense = ou.random_dense(rng, 40000, 120)
    state = np.ones(120, dtype=np.uint8)
    state[[4, 9]] = 0
    state[[11]] = 2
    with context(dev, dense) as m:
        m.set_state(state)
        whole = m.run(20)
        m.reset()
        first = m.run(10)
        covered, stats = m.covered(0).copy(), m.stats()
        other = multi_ref.mixed_states(rng, 66, 120)
        got = m.multi_select(15, other, seed=1, fraction=0.5)
        assert (m.covered(0) == covered).all()
        after = m.stats()
        for key in ("iterations", "tot_captured", "score_launches", "persist_launches", "persist_iterations"):
            assert after[key] == stats[key], key
        second = m.run(10)
        again = m.multi_select(15, other, seed=1, fraction=0.5)
    assert np.concatenate([first[0], second[0]]).tolist() == whole[0].tolist()
    assert np.concatenate([first[1], second[1]]).tolist() == whole[1].tolist()
    same(got, again)
    assert got[3].min() > 0


def test_refusals_leave_the_outputs_untouched(dev):
    from utmos_amd import _native as nat
    lib = nat.lib()
    dense = ou.random_dense(np.random.default_rng(25), 500, 20)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    outs = [np.full((2, 3), 9, np.int32), np.full((2, 3), 9, np.int64), np.full(2, 9, np.int64), np.full(2, 9, np.int64)]
    states = np.ones((2, 20), dtype=np.uint8)
    words = np.full((2, 8), 2 ** 64 - 1, dtype=np.uint64)
    table = (ctypes.c_void_p * 1)(words.ctypes.data)
    null_entry = (ctypes.c_void_p * 1)(None)
    with context(dev, dense) as m:
        call = lambda n_rep, st, kp, k, o: lib.utm_multi_select(m._h, n_rep, p(st), kp, 0, 2 ** 31, k, *[p(x) for x in o], None)
        bad = states.copy()
        bad[1, 19] = 3
        assert call(0, states, table, 3, outs) == EINVAL and call(257, np.ones((257, 20), np.uint8), None, 3, outs) == EINVAL
        assert call(2, states, table, -1, outs) == EINVAL
        assert call(2, bad, table, 3, outs) == EINVAL and b"state" in lib.utm_last_error()
        assert call(2, states, null_entry, 3, outs) == EINVAL and b"keep[0]" in lib.utm_last_error()
        assert call(2, None, table, 3, outs) == EINVAL
        for i in range(4):
            assert call(2, states, table, 3, outs[:i] + [None] + outs[i + 1:]) == EINVAL
        assert all((o == 9).all() for o in outs)
        assert call(2, states, table, 3, outs) == 0 and outs[2].tolist() == [500, 500] and outs[3].tolist() == [3, 3]
        with pytest.raises(ValueError):
            m.multi_select(3, states, keep=[np.ones((2, 499), dtype=bool)])
        with pytest.raises(ValueError):
            m.multi_select(3, states, fraction=0.0)
    outs = [np.full((2, 3), 9, np.int32), np.full((2, 3), 9, np.int64), np.full(2, 9, np.int64), np.full(2, 9, np.int64)]
    with dev.DeviceMatrix(20, first_sample=0, n_local=10) as shard:  # a shard of the sample axis
        c = shard.add_chunk(500)
        shard.upload_columns(c, npo.pack_columns(dense)[:10])
        rc = lib.utm_multi_select(shard._h, 2, p(states), table, 0, 2 ** 31, 3, *[p(x) for x in outs], None)
        assert rc == ESTATE and all((o == 9).all() for o in outs)


def test_the_command_on_two_parts_in_64_variant_chunks(tmp_path):
    from utmos_amd import stability
    from utmos_amd.select import select_main
    parts = [os.path.join(ou.GOLD, name + ".npz") for name in ("chunk0", "chunk1")]
    exclude = ou.read_list(os.path.join(ou.GOLD, "exclude.txt"))
    common = ["-c", "6", "--maxmem", "0", "--buffer", "64", "--exclude", os.path.join(ou.GOLD, "exclude.txt"), "--seed", "17"]
    plain, with_flags = str(tmp_path / "plain.tsv"), str(tmp_path / "flags.tsv")
    npz, tsv = str(tmp_path / "rep.npz"), str(tmp_path / "stab.tsv")
    select_main(common + ["-o", plain] + parts)
    select_main(common + ["-o", with_flags, "--replicates", "9", "--subsample", "0.4", "--replicates-out", npz, "--stability-out", tsv] + parts)
    text = open(plain).read()
    assert text == open(with_flags).read() and len(text.splitlines()) > 2
    dense, _, samples = npo.build_matrix([ou.load_part("chunk0"), ou.load_part("chunk1")])
    assert dense.shape[0] > 3 * 64                                   # several chunks
    state = npo.initial_state(samples, None, exclude)
    assert (state == 2).any()
    k = npo.resolve_count(len(samples), 6)
    keep = multi_ref.hashed_keep(17, 9, dense.shape[0], stability.keep_threshold(0.4))
    order, new, kept, done = multi_ref.select(dense, np.tile(state, (9, 1)), keep, k)
    names = [str(s) for s in samples]
    panel = [names.index(line.split("\t")[0]) for line in text.splitlines()[1:]]
    z = np.load(npz)
    for key, want in (("order", order), ("new", new), ("kept", kept), ("n_done", done), ("panel", panel)):
        assert z[key].tolist() == np.asarray(want).tolist(), key
    mean, low, high = stability.curve_band(new, kept)
    assert z["pct_mean"].tolist() == mean.tolist() and z["pct_min"].tolist() == low.tolist() and z["pct_max"].tolist() == high.tolist()
    assert z["samples"].tolist() == names and int(z["seed"]) == 17 and float(z["fraction"]) == 0.4
    stability.write_table(str(tmp_path / "want.tsv"), stability.selection_table(order, done, names, panel))
    assert open(tsv).read() == open(tmp_path / "want.tsv").read()
    assert len(open(tsv).read().splitlines()) > 2
