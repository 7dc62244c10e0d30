"""GPU: fixed orders through the C ABI (utm_apply_order / k_order_curve) and the command line (--include, --mode).

Gains and covered masks are held against the numpy restatement (tests/order_ref.py), the loop's continuation against a
fresh context that starts with the same samples used, and the command line against what the reference's own code
answered for a forced order (tests/golden/order, tools/make_order_traces.py)."""
import os

import numpy as np
import pytest

import oracle_util as ou
import order_ref

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def synth_matrix(dev, n_samp, chunk_vars, seed, af=None):
    """A context over the synthetic matrix cut into chunks, and the same columns on the host (chunks side by side: every
    chunk's words are zero padded, so popcounts over the joined words are popcounts over the variants)."""
    m = dev.DeviceMatrix(n_samp)
    host, first = [], 0
    for n_var in chunk_vars:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=seed, first_var_global=first)
        cols, af32 = dev.synth_host(seed, n_var, n_samp, first_var_global=first)
        if af == "f32":
            m.set_af(c, af32)
        elif af == "f64":
            m.set_af(c, af32.astype(np.float64) / 3.0)      # not representable in float32
        host.append(cols)
        first += n_var
    return m, np.concatenate(host, axis=1)


def covered_of(m):
    return np.concatenate([m.covered(c) for c in range(len(m.chunk_vars))])


def orders_for(rng, n_samp):
    orders = {"one": np.array([n_samp - 1]), "all": rng.permutation(n_samp)}
    if n_samp > 64:
        orders["64"] = rng.permutation(n_samp)[:64]
    return orders


# ----------------------------------------------------------------- gains and covered
@pytest.mark.parametrize("n_samp,chunk_vars", [(1, [1]), (1, [63]), (65, [63]), (65, [4097]), (65, [70_000]), (2504, [4097]),
                                               (2504, [70_000]), (65, [1_100_000]), (65, [1, 63, 4097]),
                                               (2504, [20_000, 30_000, 20_000]), (65, [400_000, 300_001, 399_999])])
def test_gains_and_covered_equal_the_restatement(dev, n_samp, chunk_vars):
    rng = np.random.default_rng(n_samp * 7 + sum(chunk_vars))
    m, cols = synth_matrix(dev, n_samp, chunk_vars, seed=3)
    with m:
        state = np.ones(n_samp, np.uint8)
        if n_samp > 2:
            state[rng.choice(n_samp, n_samp // 4, replace=False)] = 2          # excluded samples are accepted
        for order in orders_for(rng, n_samp).values():
            m.set_state(state)
            m.reset()
            want, covered = order_ref.order_curve(cols, order, n_var=sum(chunk_vars))
            got = m.apply_order(order)
            assert got.tolist() == want.tolist()
            assert (covered_of(m) == covered).all()
            st = m.stats()
            assert st["iterations"] == len(want) and st["tot_captured"] == int(want.sum())


def test_prefix_that_captures_everything_stops_and_leaves_the_rest_selectable(dev):
    n_var, n_samp = 5000, 40
    rng = np.random.default_rng(1)
    dense = ou.random_dense(rng, n_var, n_samp)
    dense[:, 9] = True                                               # sample 9 carries every variant
    cols = ou.npo.pack_columns(dense)
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        order = [4, 9, 20, 21]
        want, covered = order_ref.order_curve(cols, order, n_var=n_var)
        got = m.apply_order(order)
        assert len(got) == 2 and got.tolist() == want.tolist() and int(got.sum()) == n_var
        assert (m.covered(c) == covered).all()
        assert len(m.run(5)[0]) == 0                                 # nothing left to capture
        assert len(m.apply_order([20])) == 0
        # the samples behind the stop were not used up: after a restart they can be listed again
        m.reset()
        assert m.apply_order([20, 21]).tolist() == order_ref.order_curve(cols, [20, 21])[0].tolist()


def test_zero_gain_rows_and_an_empty_list(dev):
    n_var, n_samp = 3000, 12
    dense = ou.random_dense(np.random.default_rng(2), n_var, n_samp)
    dense[:, 5] = dense[:, 1]
    cols = ou.npo.pack_columns(dense)
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        assert m.apply_order([]).tolist() == []
        assert m.stats()["iterations"] == 0
        got = m.apply_order([1, 5, 0])
        assert got.tolist() == order_ref.order_curve(cols, [1, 5, 0])[0].tolist() and got[1] == 0
        assert m.stats()["iterations"] == 3


# ----------------------------------------------------------------- the loop goes on as if the samples had started out used
def configure(m, state, weights, decremental, exact):
    m.set_state(state)
    m.set_weights(weights)
    m.set_decremental(decremental)
    m.set_af_exact_scores(exact)
    m.reset()


def assert_same_rows(got, want, exact_scores):
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    if exact_scores:
        assert got[2].tolist() == want[2].tolist()
    else:
        # AF scores reported without their chains are the fixed-point estimate: a sum of float32-rounded values, within
        # 2^-24 (relative) of the float64 sum per addend, all addends of one sign; either call may report either
        np.testing.assert_allclose(got[2], want[2], rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("af", [None, "f32", "f64"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("decremental,exact", [(False, True), (True, False), (True, True), (False, False)])
def test_run_after_apply_order_equals_a_fresh_context_with_them_used(dev, af, weighted, decremental, exact):
    n_samp, chunk_vars, k = 300, [30_000, 50_001], 60
    rng = np.random.default_rng(17)
    state = np.ones(n_samp, np.uint8)
    state[rng.choice(n_samp, 30, replace=False)] = 2
    state[[3, 250]] = 0
    prefix = [int(s) for s in rng.permutation(np.flatnonzero(state == 1))[:7]]
    prefix.insert(3, int(np.flatnonzero(state == 2)[0]))                              # ... and an excluded one among them
    weights = rng.choice([0.5, 1.0, 1.0, 2.25], size=n_samp) if weighted else None
    a, cols = synth_matrix(dev, n_samp, chunk_vars, seed=5, af=af)
    b, _ = synth_matrix(dev, n_samp, chunk_vars, seed=5, af=af)
    with a, b:
        configure(a, state, weights, decremental, exact)
        start = covered_of(a)
        gains = a.apply_order(prefix)
        want, covered = order_ref.order_curve(cols, prefix, covered=start)
        assert gains.tolist() == want.tolist() and (covered_of(a) == covered).all()
        used = state.copy()
        used[prefix] = 0
        configure(b, used, weights, decremental, exact)
        got, ref = a.run(k), b.run(k)
        assert len(ref[0]) == k
        assert_same_rows(got, ref, exact or af is None)
        assert (covered_of(a) == covered_of(b)).all()
        sa, sb = a.stats(), b.stats()
        assert sa["iterations"] == len(prefix) + k and sa["tot_captured"] == int(gains.sum()) + sb["tot_captured"]


@pytest.mark.parametrize("af", [None, "f32"])
def test_run_apply_order_run(dev, af):
    n_samp, chunk_vars, first, second = 200, [40_000, 25_000], 9, 30
    a, cols = synth_matrix(dev, n_samp, chunk_vars, seed=8, af=af)
    b, _ = synth_matrix(dev, n_samp, chunk_vars, seed=8, af=af)
    with a, b:
        winners = a.run(first)[0]
        assert len(winners) == first
        listed = [s for s in (150, 3, 77, 42, 199) if s not in winners]
        before = covered_of(a)
        gains = a.apply_order(listed)
        want, covered = order_ref.order_curve(cols, listed, covered=before)
        assert gains.tolist() == want.tolist() and (covered_of(a) == covered).all()
        used = np.ones(n_samp, np.uint8)
        used[winners] = 0
        used[listed] = 0
        b.set_state(used)
        assert_same_rows(a.run(second), b.run(second), True)
        with pytest.raises(dev.nat.NativeError) as e:
            a.apply_order([int(winners[0])])                         # a winner of the loop is used
        assert e.value.code == EINVAL


def test_continuation_where_the_persistent_loop_runs(dev):
    n_samp, n_var, k = 2504, 1_103_547, 40
    a, cols = synth_matrix(dev, n_samp, [n_var], seed=1)
    b, _ = synth_matrix(dev, n_samp, [n_var], seed=1)
    prefix = [0, 2400, 17, 999, 5, 1234]
    with a, b:
        gains = a.apply_order(prefix)
        assert gains.tolist() == order_ref.order_curve(cols, prefix)[0].tolist()
        used = np.ones(n_samp, np.uint8)
        used[prefix] = 0
        b.set_state(used)
        assert_same_rows(a.run(k), b.run(k), True)
        assert a.stats()["persist_iterations"] > 0 and b.stats()["persist_iterations"] > 0
        assert (covered_of(a) == covered_of(b)).all()


# ----------------------------------------------------------------- errors
def test_bad_lists_are_refused_and_change_nothing(dev):
    n_var, n_samp = 9000, 30
    cols = ou.npo.pack_columns(ou.random_dense(np.random.default_rng(4), n_var, n_samp))
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        state = np.ones(n_samp, np.uint8)
        state[11] = 0
        m.set_state(state)
        winners = m.run(2)[0]
        covered, stats = m.covered(c), m.stats()
        for bad in ([1, 2, 1], [5, 11], [int(winners[1])], [3, n_samp], [-1]):     # duplicate, used, used by the loop, range
            with pytest.raises(dev.nat.NativeError) as e:
                m.apply_order(bad)
            assert e.value.code == EINVAL, bad
            assert (m.covered(c) == covered).all() and m.stats() == stats
        import ctypes
        done = ctypes.c_int64(7)
        assert dev.nat.lib().utm_apply_order(m._h, None, 2, None, ctypes.byref(done)) == EINVAL
        assert dev.nat.lib().utm_apply_order(m._h, None, 0, None, None) == EINVAL
        free = [s for s in range(n_samp) if s != 11 and s not in winners]
        assert m.apply_order(free[:3]).tolist() == order_ref.order_curve(cols, free[:3], covered=covered)[0].tolist()


def test_a_shard_refuses_fixed_orders(dev):
    n_var = 2000
    cols = ou.npo.pack_columns(ou.random_dense(np.random.default_rng(6), n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.apply_order([3])
        assert e.value.code == ESTATE


# ----------------------------------------------------------------- the command line against the reference-made fixtures
def run_cli(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def case_argv(t, tmp_path, extra=()):
    if "inputs" in t:
        files = [os.path.join(ou.GOLD, n + ".npz") for n in t["inputs"]]
    else:
        files = []
        for i, p in enumerate(t["part_list"]):
            files.append(str(tmp_path / f"part{i}.npz"))
            np.savez(files[-1], GT=p["GT"], AF=p["AF"], samples=p["samples"])
    argv = ["--include", ",".join(t["include"]), "-c", str(t["count"])]
    if t["af"]:
        argv += ["--af"]
    if t["af_dtype"] == "f32":               # float32 AF values are what a store keeps (as the reference's hdf5 does)
        argv += ["--lowmem", str(tmp_path / "store.utm")]
    if t["subset"]:
        argv += ["--subset", os.path.join(ou.GOLD, t["subset"])]
    if t["exclude"]:
        argv += ["--exclude", ",".join(t["exclude"])]
    if t["weights"]:
        argv += ["--weights", os.path.join(ou.GOLD, t["weights"])]
    out = str(tmp_path / "out.tsv")
    return argv + list(extra) + ["-o", out] + files, out


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("name", order_ref.case_names())
def test_cli_include_reproduces_the_reference_made_rows(name, chunked, tmp_path):
    t = order_ref.load_case(name)
    argv, out = case_argv(t, tmp_path, ["--maxmem", "0", "--buffer", "64"] if chunked else [])
    run_cli(argv)
    assert open(out).read() == order_ref.case_tsv(t)


def fixture_matrix(af):
    parts = [ou.load_part(n) for n in ("chunk0", "chunk1")]
    matrix, var_count, samples = ou.npo.build_matrix(parts, af=af)
    values = None
    if af:
        values = np.concatenate([np.asarray(p["AF"], np.float64).reshape(-1)[np.unpackbits(p["GT"], axis=1).any(axis=1)]
                                 for p in parts])
    return ou.npo.pack_columns(matrix != 0), matrix.shape[0], var_count, [str(s) for s in samples], values


def rows_text(cols, n_var, var_count, samples, order):
    gains, _ = order_ref.order_curve(cols, order, n_var=n_var)
    text, total = "sample\tvar_count\tnew_count\ttot_captured\tpct_captured\n", np.int64(0)
    for s, gain in zip(order, gains):
        total += gain
        text += "\t".join(str(x) for x in [samples[s], int(var_count[s]), int(gain), int(total), round(total / n_var, 4)]) + "\n"
    return text


@pytest.mark.parametrize("af", [False, True])
@pytest.mark.parametrize("count", ["25", "-1"])
def test_cli_mode_topn(af, count, tmp_path):
    cols, n_var, var_count, samples, values = fixture_matrix(af)
    state = np.ones(len(samples), np.uint8)
    _, _, scores = ou.c_score(cols, n_var, state, af=values)          # greedy's first iteration, as the oracle scores it
    order = order_ref.topn_order(scores, state)
    if count != "-1":
        order = order[:int(count)]
    out = str(tmp_path / "out.tsv")
    run_cli(["--mode", "topN", "-c", count] + (["--af"] if af else []) + ["-o", out] +
            [os.path.join(ou.GOLD, n + ".npz") for n in ("chunk0", "chunk1")])
    assert open(out).read() == rows_text(cols, n_var, var_count, samples, order)


@pytest.mark.parametrize("af", [False, True])
def test_cli_mode_random(af, tmp_path):
    cols, n_var, var_count, samples, _ = fixture_matrix(af)
    order = order_ref.random_order(np.ones(len(samples), np.uint8), 3)[:30]
    out = str(tmp_path / "out.tsv")
    run_cli(["--mode", "random", "--seed", "3", "-c", "30"] + (["--af"] if af else []) + ["-o", out] +
            [os.path.join(ou.GOLD, n + ".npz") for n in ("chunk0", "chunk1")])
    assert open(out).read() == rows_text(cols, n_var, var_count, samples, order)


def test_cli_include_then_topn_fills_what_is_left_of_count(tmp_path):
    cols, n_var, var_count, samples, _ = fixture_matrix(False)
    prefix = [0, 2400, 17]
    state = np.ones(len(samples), np.uint8)
    state[prefix] = 0
    _, _, scores = ou.c_score(cols, n_var, state)
    order = prefix + order_ref.topn_order(scores, state)[:7].tolist()
    out = str(tmp_path / "out.tsv")
    run_cli(["--include", ",".join(samples[s] for s in prefix), "--mode", "topN", "-c", "10", "-o", out] +
            [os.path.join(ou.GOLD, n + ".npz") for n in ("chunk0", "chunk1")])
    assert open(out).read() == rows_text(cols, n_var, var_count, samples, order)


# ----------------------------------------------------------------- size
def test_whole_order_of_a_two_million_variant_matrix_in_one_call(dev):
    n_samp, n_var = 2504, 2_000_000
    m, cols = synth_matrix(dev, n_samp, [n_var], seed=2)
    with m:
        order = np.random.default_rng(9).permutation(n_samp)
        want, covered = order_ref.order_curve(cols, order, n_var=n_var)
        got = m.apply_order(order)
        assert got.tolist() == want.tolist()
        assert (covered_of(m) == covered).all()
