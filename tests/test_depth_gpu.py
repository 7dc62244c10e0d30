"""GPU: the selection with a coverage depth M > 1 (utm_set_depth / k_depth_apply / select --depth).

The truth is the numpy restatement tests/depth_ref.py, which tests/test_depth_host.py holds against the recorded traces
of the reference's own code at M = 1.  At M > 1 the device has to equal it exactly: winners, new_count, at_depth, the
float64 scores bit for bit, and the per-variant support afterwards."""
import os

import numpy as np
import pytest

import depth_ref
import oracle_util as ou
import order_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def af_matrix(dense, af, kind):
    """The matrix the reference would score: presence, or presence x AF as float64 / float32 (its hdf5 store)."""
    if kind is None:
        return dense
    if kind == "f32":
        return dense * af.astype(np.float32)[:, None]
    return dense * af[:, None]


def context(dev, dense, af, kind, chunk_vars=None):
    """A device context over `dense` (bool variants x samples) cut into chunks along the variants."""
    n_var, n_samp = dense.shape
    m = dev.DeviceMatrix(n_samp)
    lo = 0
    for n in chunk_vars or [n_var]:
        c = m.add_chunk(n)
        m.upload_columns(c, npo.pack_columns(dense[lo:lo + n]))
        if kind is not None:
            m.set_af(c, af[lo:lo + n].astype(np.float32 if kind == "f32" else np.float64))
        lo += n
    assert lo == n_var
    return m


def support_all(m):
    return np.concatenate([m.support(c) for c in range(len(m.chunk_vars))])


def covered_bits(m):
    return np.concatenate([np.unpackbits(m.covered(c).view(np.uint8), bitorder="little")[:n] for c, n in enumerate(m.chunk_vars)])


def check_run(m, matrix, state, weights, depth, k):
    """m.run(k) at `depth` against the restatement: rows, scores, at_depth, support, covered."""
    m.set_state(state)
    m.set_weights(weights)
    m.set_depth(depth)
    m.reset()
    want = depth_ref.greedy(matrix, state.copy(), k, weights, depth)
    idx, new, score = m.run(k)
    assert idx.tolist() == [r[0] for r in want]
    assert new.tolist() == [r[1] for r in want]
    assert [float(s).hex() for s in score] == [float(r[2]).hex() for r in want]
    assert m.at_depth(0, len(idx)).tolist() == [r[3] for r in want]
    used = state.copy()
    used[idx] = 0
    support = np.minimum(depth_ref.support_of(matrix, used), depth)
    assert (support_all(m) == support).all()
    assert (covered_bits(m) == (support >= depth)).all()
    st = m.stats()
    assert st["iterations"] == len(want) and st["tot_captured"] == sum(r[1] for r in want)
    assert st["persist_iterations"] == 0 and st["decr_iterations"] == 0 and st["af_deferred_rows"] == 0
    return want


def seeded(n_var=3000, n_samp=70, seed=11):
    rng = np.random.default_rng(seed)
    dense = ou.random_dense(rng, n_var, n_samp)
    af = rng.integers(1, 2 * n_samp, size=n_var) / (2.0 * n_samp) / 3.0     # not representable in float32
    af[rng.random(n_var) < 0.05] = 0.0                                        # AF == 0 rows: never scored, never counted
    return rng, dense, af


# ----------------------------------------------------------------- the ABI against the restatement
@pytest.mark.parametrize("chunked", [False, True], ids=["one-chunk", "chunks"])
@pytest.mark.parametrize("states", ["all", "subset-used"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("kind", [None, "f32", "f64"], ids=["int", "af32", "af64"])
@pytest.mark.parametrize("depth", [2, 3, 5])
def test_seeded_matrix_equals_the_restatement(dev, depth, kind, weighted, states, chunked):
    rng, dense, af = seeded()
    n_var, n_samp = dense.shape
    state = np.ones(n_samp, np.uint8)
    if states == "subset-used":
        state[rng.choice(n_samp, 20, replace=False)] = 2
        state[[4, 33, 34]] = 0                                               # start out used: they add support
    weights = rng.choice([-1.5, 0.5, 1.0, 1.0, 2.25], size=n_samp) if weighted else None
    with context(dev, dense, af, kind, [1024, 64, 1024, 888] if chunked else None) as m:
        want = check_run(m, af_matrix(dense, af, kind), state, weights, depth, n_samp)
        assert len(want) >= 20


@pytest.mark.parametrize("parts,kind,depth,weighted,k", [
    (("tiny",), None, 2, False, 36), (("tiny",), "f64", 3, True, 36), (("tiny",), "f32", 5, False, 36),
    (("chunk0", "chunk1", "chunk2"), None, 2, True, 8), (("chunk0", "chunk1"), "f64", 3, False, 6),
    (("chunk0", "chunk1"), "f32", 2, True, 6), (("mid",), None, 5, False, 8), (("mid",), "f64", 2, True, 6)])
def test_fixture_parts_equal_the_restatement(dev, parts, kind, depth, weighted, k):
    part_list = [ou.load_part(n) for n in parts]
    dense, _, samples = npo.build_matrix(part_list)
    af = np.concatenate([np.asarray(p["AF"], np.float64).reshape(-1)[np.unpackbits(p["GT"], axis=1).any(axis=1)] for p in part_list])
    rng = np.random.default_rng(len(samples) + depth)
    state = np.ones(len(samples), np.uint8)
    state[rng.choice(len(samples), len(samples) // 5, replace=False)] = 2
    state[[1, 7]] = 0
    weights = rng.choice([-2.0, 0.5, 1.0, 1.0, 3.0], size=len(samples)) if weighted else None
    rows = [int((np.unpackbits(p["GT"], axis=1).any(axis=1)).sum()) for p in part_list]
    with context(dev, dense, af, kind, rows) as m:
        check_run(m, af_matrix(dense, af, kind), state, weights, depth, k)


def test_depth_1_set_explicitly_is_the_context_that_never_heard_of_it(dev):
    n_samp, n_var, k = 300, 80_000, 120
    a, b = dev.DeviceMatrix(n_samp), dev.DeviceMatrix(n_samp)
    with a, b:
        for m in (a, b):
            m.synth_fill(m.add_chunk(n_var), seed=4)
        a.set_depth(2)
        a.set_depth(1)                                                # back to 1: nothing of depth 2 may linger
        got, want = a.run(k), b.run(k)
        for x, y in zip(got, want):
            assert x.tolist() == y.tolist()
        sa, sb = a.stats(), b.stats()
        assert sb["persist_iterations"] > 0                           # the persistent loop is what ran
        for key in sa:
            if key not in ("score_ms", "loop_ms"):
                assert sa[key] == sb[key], key
        assert a.depth()["apply_launches"] == 0
        assert (a.covered(0) == b.covered(0)).all()
        assert (a.support(0) == covered_bits(a)).all()                 # at depth 1 the support is the covered bit
        # ... and decremental passes are still taken at depth 1
        for m in (a, b):
            m.set_decremental(True, 100.0)                            # (a threshold every later iteration passes)
        a.set_depth(1)
        got, want = a.run(k), b.run(k)
        assert got[0].tolist() == want[0].tolist() and a.stats()["decr_iterations"] == b.stats()["decr_iterations"] > 0


@pytest.mark.parametrize("kind", [None, "f32"])
def test_depth_2_with_decremental_and_the_persistent_loop_requested(dev, kind):
    rng, dense, af = seeded(6000, 90, seed=5)
    state = np.ones(90, np.uint8)
    with context(dev, dense, af, kind) as m:
        m.set_decremental(True, 100.0)                                # asked for, and off while the depth is 2
        want = check_run(m, af_matrix(dense, af, kind), state, None, 2, 40)
        assert len(want) == 40 and m.depth()["apply_launches"] == 40
        # back at depth 1 the same context takes both again
        m.set_depth(1)
        m.set_state(state)
        m.run(40)
        assert m.stats()["decr_iterations"] > 0


@pytest.mark.parametrize("kind", [None, "f64"])
def test_apply_order_then_run_equals_a_fresh_context_with_them_used(dev, kind):
    rng, dense, af = seeded(5000, 80, seed=9)
    n_samp, depth, k = 80, 2, 25
    matrix = af_matrix(dense, af, kind)
    state = np.ones(n_samp, np.uint8)
    state[rng.choice(n_samp, 10, replace=False)] = 2
    state[[2, 50]] = 0
    prefix = [int(s) for s in rng.permutation(np.flatnonzero(state == 1))[:6]] + [int(np.flatnonzero(state == 2)[0])]
    with context(dev, dense, af, kind, [2048, 2952]) as a, context(dev, dense, af, kind, [2048, 2952]) as b:
        a.set_state(state)
        a.set_depth(depth)
        a.reset()
        ref_state = state.copy()
        want = depth_ref.fixed_order(matrix, ref_state, prefix, depth)
        gains = a.apply_order(prefix)
        assert gains.tolist() == [r[1] for r in want]
        assert a.at_depth(0, len(gains)).tolist() == [r[2] for r in want]
        assert (support_all(a) == np.minimum(depth_ref.support_of(matrix, ref_state), depth)).all()
        b.set_state(ref_state)
        b.set_depth(depth)
        got, ref = a.run(k), b.run(k)
        assert len(ref[0]) == k
        for x, y in zip(got, ref):
            assert x.tolist() == y.tolist()
        assert a.at_depth(len(prefix), k).tolist() == b.at_depth(0, k).tolist()
        assert (support_all(a) == support_all(b)).all() and (covered_bits(a) == covered_bits(b)).all()
        assert a.stats()["tot_captured"] == int(gains.sum()) + b.stats()["tot_captured"]
        cont = depth_ref.greedy(matrix, ref_state, k, None, depth)
        assert got[0].tolist() == [r[0] for r in cont] and got[1].tolist() == [r[1] for r in cont]


def test_a_fixed_order_ends_after_the_row_that_fills_every_variant_to_depth(dev):
    rng = np.random.default_rng(3)
    dense = ou.random_dense(rng, 900, 12)
    dense[:, 3] = dense[:, 8] = True
    with context(dev, dense, None, None) as m:
        m.set_depth(2)
        gains = m.apply_order([5, 3, 8, 1, 2])
        want = depth_ref.fixed_order(dense, np.ones(12, np.uint8), [5, 3, 8, 1, 2], 2)
        assert len(gains) == 3 and gains.tolist() == [r[1] for r in want] and int(gains.sum()) == 2 * 900
        assert m.at_depth(0, 3).tolist() == [r[2] for r in want] and m.at_depth(2, 1)[0] == 900
        assert len(m.run(3)[0]) == 0 and (support_all(m) == 2).all()


def test_errors_leave_the_context_usable(dev):
    rng, dense, af = seeded(2000, 20, seed=2)
    with context(dev, dense, None, None) as m:
        for bad in (0, 256, -1):
            with pytest.raises(dev.nat.NativeError) as e:
                m.set_depth(bad)
            assert e.value.code == EINVAL
        with pytest.raises(dev.nat.NativeError) as e:
            m.at_depth(0, 0)                                           # depth 1 keeps no such record
        assert e.value.code == ESTATE
        check_run(m, dense, np.ones(20, np.uint8), None, 2, 5)
        with pytest.raises(dev.nat.NativeError) as e:
            m.at_depth(3, 5)
        assert e.value.code == EINVAL
    with dev.DeviceMatrix(30, first_sample=10, n_local=20) as shard:
        c = shard.add_chunk(2000)
        shard.upload_columns(c, npo.pack_columns(dense))
        with pytest.raises(dev.nat.NativeError) as e:
            shard.set_depth(2)
        assert e.value.code == ESTATE
        shard.set_depth(1)
        assert shard.local_best()[1] >= 0                              # still scores


# ----------------------------------------------------------------- full size
def test_packed_form_equals_the_restatement_on_small_cases():
    for seed, depth in ((1, 2), (2, 3), (3, 5)):
        rng, dense, _ = seeded(1500, 40, seed)
        state = np.ones(40, np.uint8)
        state[rng.choice(40, 8, replace=False)] = 2
        state[[0, 9]] = 0
        want = depth_ref.greedy(dense, state.copy(), 40, None, depth)
        final = state.copy()
        got, support = depth_ref.packed_greedy(npo.pack_columns(dense), 1500, final, 40, depth)
        assert got == [(r[0], r[1], r[3]) for r in want]
        assert (support == np.minimum(depth_ref.support_of(dense, final), depth)).all()


def test_chr22_sized_matrix_first_32_rows(dev):
    n_samp, n_var, depth, k = 2504, 1_103_547, 2, 32
    with dev.DeviceMatrix(n_samp) as m:
        c = m.add_chunk(n_var)
        m.synth_fill(c, seed=1)
        cols = np.empty((n_samp, (n_var + 63) // 64), np.uint64)
        for lo in range(0, n_samp, 512):
            m.download_columns(c, lo, min(512, n_samp - lo), out=cols[lo:lo + 512])
        m.set_depth(depth)
        idx, new, _ = m.run(k)
        want, support = depth_ref.packed_greedy(cols, n_var, np.ones(n_samp, np.uint8), k, depth)
        assert idx.tolist() == [r[0] for r in want] and new.tolist() == [r[1] for r in want]
        assert m.at_depth(0, k).tolist() == [r[2] for r in want]
        assert (m.support(c) == support).all()
        st = m.stats()
        assert st["persist_iterations"] == 0 and m.depth()["apply_launches"] == k


# ----------------------------------------------------------------- the command line
FILES = [os.path.join(ou.GOLD, n + ".npz") for n in ("chunk0", "chunk1")]


def cli(argv, tmp_path):
    from utmos_amd.select import select_main
    out = str(tmp_path / "out.tsv")
    select_main(argv + ["-o", out] + FILES)
    return open(out).read()


def cli_inputs(af):
    matrix, var_count, samples = npo.build_matrix([ou.load_part(n) for n in ("chunk0", "chunk1")], af=af)
    return matrix, var_count, [str(s) for s in samples]


@pytest.mark.parametrize("extra", [[], ["--maxmem", "0", "--buffer", "64"], ["--brute-force"]], ids=["default", "chunked", "brute"])
def test_cli_depth_2(extra, tmp_path):
    matrix, var_count, samples = cli_inputs(False)
    rows = depth_ref.greedy(matrix, np.ones(len(samples), np.uint8), 20, None, 2)
    assert cli(["--depth", "2", "-c", "20"] + extra, tmp_path) == depth_ref.tsv(rows, samples, var_count, matrix.shape[0], 2)


def test_cli_depth_2_af_and_weights(tmp_path):
    matrix, var_count, samples = cli_inputs(True)
    w = npo.weight_vector(np.asarray(samples), ou.read_weights(os.path.join(ou.GOLD, "weights.txt")))
    rows = depth_ref.greedy(matrix, np.ones(len(samples), np.uint8), 20, w, 2)
    got = cli(["--depth", "2", "-c", "20", "--af", "--weights", os.path.join(ou.GOLD, "weights.txt")], tmp_path)
    assert got == depth_ref.tsv(rows, samples, var_count, matrix.shape[0], 2)


def test_cli_depth_3_include_then_greedy(tmp_path):
    matrix, var_count, samples = cli_inputs(False)
    prefix = [0, 2400, 17]
    state = np.ones(len(samples), np.uint8)
    first = depth_ref.fixed_order(matrix, state, prefix, 3)
    rest = depth_ref.greedy(matrix, state, 7, None, 3)
    want = depth_ref.tsv(first, samples, var_count, matrix.shape[0], 3) + \
        depth_ref.tsv(rest, samples, var_count, matrix.shape[0], 3, sum(r[1] for r in first), header=False)
    assert cli(["--depth", "3", "-c", "10", "--include", ",".join(samples[s] for s in prefix)], tmp_path) == want


def test_cli_depth_2_mode_topn(tmp_path):
    matrix, var_count, samples = cli_inputs(False)
    state = np.ones(len(samples), np.uint8)
    scores = depth_ref.calculate_scores(matrix, state, None, 2)[2]
    order = order_ref.topn_order(scores, state)[:20]
    rows = depth_ref.fixed_order(matrix, state, order, 2)
    assert cli(["--depth", "2", "-c", "20", "--mode", "topN"], tmp_path) == depth_ref.tsv(rows, samples, var_count, matrix.shape[0], 2)


def test_cli_depth_1_writes_todays_five_columns(tmp_path):
    matrix, var_count, samples = cli_inputs(False)
    rows = depth_ref.greedy(matrix, np.ones(len(samples), np.uint8), 10, None, 1)
    want = depth_ref.tsv(rows, samples, var_count, matrix.shape[0], 1)
    assert cli(["--depth", "1", "-c", "10"], tmp_path) == want == cli(["-c", "10"], tmp_path)


def test_cli_depth_on_several_processes_exits_1(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli(["--depth", "2", "-c", "5"], tmp_path)
    assert e.value.code == 1
