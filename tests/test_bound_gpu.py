"""GPU: the coverage bound through the C ABI (utm_coverage_bound: k_swap_masks + k_bound_init, then k_bound_sums, k_bound_pick
and k_bound_update per iteration) and DeviceMatrix.coverage_bound.

History, bound, best iteration, live count and the multipliers are held against the numpy restatement (tests/bound_ref.py)
and the CPU build bit for bit.  The shapes sit on the kernels' edges: one variant, a word + 1, a 4,096-variant table tile
- 1, the 32,768 variants of a mask tile +- 0 / + 1, three of them + 5 with one all-ones column (a 32-bit partial sum of
more than 65,536 multipliers at Q would wrap), sample counts on both sides of a workgroup's 128 candidates, 1,100
candidates for the pick (wider than its workgroup), ties on both sides of its blocks and 4,100 candidates (more than it keeps
in registers)."""
import ctypes
import functools

import numpy as np
import pytest

import bound_ref
import oracle_util as ou
from bound_ref import Q, host_bound
from oracle_util import npo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
TIMING = ("score_ms", "loop_ms")
TALL = 3 * 32768 + 5
T = 12


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


@functools.lru_cache(maxsize=None)
def seeded(n_var, n_samp):
    rng = np.random.default_rng(n_var * 7 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    if n_var == TALL:
        dense[:, 3] = True                                               # one all-ones column
    dense.setflags(write=False)
    return dense


def uploaded(dev, cols_per_chunk, chunk_vars, **kw):
    m = dev.DeviceMatrix(cols_per_chunk[0].shape[0], **kw)
    for cols, n_var in zip(cols_per_chunk, chunk_vars):
        m.upload_columns(m.add_chunk(n_var), cols)
    return m


def as_dict(res):
    return dict(hist=res.hist, bound=res.bound, best_iter=res.best_iter, n_live=res.n_live,
                lambdas=None if res.lambdas is None else np.concatenate(res.lambdas))


def same(got, want, lambdas=True):
    assert got["hist"].tolist() == want["hist"].tolist()
    assert (got["bound"], got["best_iter"], got["n_live"]) == (want["bound"], want["best_iter"], want["n_live"])
    if lambdas:
        assert np.array_equal(got["lambdas"], want["lambdas"])


def deterministic(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


# ----------------------------------------------------------------- 1. the ABI against the restatement and the CPU build
@pytest.mark.parametrize("n_samp", [17, 70, 200])
@pytest.mark.parametrize("n_var", [1, 65, 8191, 32768, 32769, TALL])
def test_bound_equals_the_restatement_and_the_cpu_build(dev, n_var, n_samp):
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    with uploaded(dev, [cols], [n_var]) as mat:
        for k in (1, 5, n_samp):
            got = as_dict(mat.coverage_bound(k, iters=T, period=2, want_lambda=True))
            same(got, bound_ref.coverage_bound(dense, k, iters=T, period=2))
            same(got, host_bound(cols, n_var, k, iters=T, period=2))
        if n_var == TALL:
            assert got["hist"][0] > 2 ** 32                              # the all-ones column alone: more than 32 bits
        # a list in another order, with `given`, default step and period
        rng = np.random.default_rng(n_var + n_samp)
        order = rng.permutation(n_samp)
        given, cand = order[:2], order[1:]                               # (order[1] is in both lists)
        got = as_dict(mat.coverage_bound(4, cand=cand, given=given, iters=T, want_lambda=True))
        same(got, bound_ref.coverage_bound(dense, 4, cand=cand, given=given, iters=T))
        same(got, host_bound(cols, n_var, 4, cand=cand, given=given, iters=T))


def test_a_pick_wider_than_its_workgroup(dev):
    n_var, n_samp = 4101, 1100
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    with uploaded(dev, [cols], [n_var]) as mat:
        for k in (1, 37, 1100):
            got = as_dict(mat.coverage_bound(k, iters=T, period=2, want_lambda=True))
            same(got, bound_ref.coverage_bound(dense, k, iters=T, period=2))
            same(got, host_bound(cols, n_var, k, iters=T, period=2))


@pytest.mark.parametrize("n_samp,n_var", [(1100, 300), (4100, 65)])
def test_ties_across_the_pick_s_blocks_and_more_candidates_than_it_keeps_in_registers(dev, n_samp, n_var):
    """Seven distinct columns repeated over all samples: every sum ties with more than a hundred others, on both sides of a
    block of 1,024 positions; 4,100 candidates are more than the pick's threads hold in registers (4 x 1,024)."""
    rng = np.random.default_rng(n_samp)
    dense = np.tile(ou.random_dense(rng, n_var, 7, density=0.3, sfs=False), (1, n_samp // 7 + 1))[:, :n_samp]
    cols = npo.pack_columns(dense)
    with uploaded(dev, [cols], [n_var]) as mat:
        for k in (1, 37, 1030, n_samp - 3):
            got = as_dict(mat.coverage_bound(k, iters=6, period=2, want_lambda=True))
            same(got, bound_ref.coverage_bound(dense, k, iters=6, period=2))


def test_two_chunks_equal_the_call_on_their_concatenation(dev):
    chunk_vars, n_samp = [4101, 5904], 70
    dense = seeded(sum(chunk_vars), n_samp)
    cols = [npo.pack_columns(dense[:4101]), npo.pack_columns(dense[4101:])]
    whole = npo.pack_columns(dense)
    with uploaded(dev, cols, chunk_vars) as two, uploaded(dev, [whole], [sum(chunk_vars)]) as one:
        for given in (None, [5, 40]):
            a = two.coverage_bound(6, given=given, iters=T, period=2, want_lambda=True)
            b = one.coverage_bound(6, given=given, iters=T, period=2, want_lambda=True)
            assert [len(x) for x in a.lambdas] == chunk_vars
            same(as_dict(a), as_dict(b))
            same(as_dict(a), bound_ref.coverage_bound(dense, 6, given=given or (), iters=T, period=2))


def test_the_bound_lies_between_greedy_and_the_trivial_bound(dev):
    n_var, n_samp, k = 32769, 200, 12
    dense = seeded(n_var, n_samp)
    with uploaded(dev, [npo.pack_columns(dense)], [n_var]) as mat:
        res = mat.coverage_bound(k, iters=60)
        greedy = int(mat.run(k)[1].sum())
        assert res.lambdas is None and res.pass_ms > 0
    assert greedy <= res.bound <= res.hist[0] // Q
    assert res.hist[0] // Q == int(np.sort(dense.sum(axis=0))[::-1][:k].sum())
    assert res.bound < res.hist[0] // Q                                  # the steps tighten it on a matrix with overlap


# ----------------------------------------------------------------- 2. stateless
def test_a_call_in_between_changes_nothing_of_the_selection(dev):
    rng = np.random.default_rng(21)
    n_var, n_samp = 40_000, 120
    dense = ou.random_dense(rng, n_var, n_samp)
    chunk_vars = [25_000, 15_000]
    cols = [npo.pack_columns(dense[:25_000]), npo.pack_columns(dense[25_000:])]
    state = np.ones(n_samp, np.uint8)
    state[[2, 50]] = 0
    state[[9, 10]] = 2
    a, b = uploaded(dev, cols, chunk_vars), uploaded(dev, cols, chunk_vars)
    with a, b:
        before = as_dict(a.coverage_bound(5, given=[2, 9], iters=T))
        for mat in (a, b):
            mat.set_state(state)
            mat.reset()
        first = a.run(10)
        covered, stats = [a.covered(c) for c in range(2)], deterministic(a.stats())
        got = as_dict(a.coverage_bound(10, iters=T, period=2, want_lambda=True))    # used and excluded samples are candidates too
        same(got, bound_ref.coverage_bound(dense, 10, iters=T, period=2))
        assert all((a.covered(c) == covered[c]).all() for c in range(2)) and deterministic(a.stats()) == stats
        second, twenty = a.run(10), b.run(20)
        assert len(twenty[0]) == 20
        assert all(np.concatenate([x, y]).tolist() == z.tolist() for x, y, z in zip(first, second, twenty))
        assert deterministic(a.stats()) == deterministic(b.stats())
        assert all((a.covered(c) == b.covered(c)).all() for c in range(2))
        same(as_dict(a.coverage_bound(5, given=[2, 9], iters=T)), before, lambdas=False)
        # in the middle of a stepped run
        for mat in (a, b):
            mat.reset()
        rows = [a.step() for _ in range(3)]
        a.coverage_bound(7, iters=T)
        rows += [a.step() for _ in range(3)]
        assert rows == [b.step() for _ in range(6)]


# ----------------------------------------------------------------- 3. errors
def test_bad_arguments_are_refused_and_leave_the_outputs(dev):
    n_var, n_samp = 9000, 30
    dense = seeded(n_var, n_samp)
    cols = npo.pack_columns(dense)
    lib = dev.nat.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    with uploaded(dev, [cols], [n_var]) as mat:
        mat.run(3)
        covered, stats = mat.covered(0), deterministic(mat.stats())
        hist, lam = np.full(5, 1234, np.int64), np.full(n_var, 1234, np.uint32)
        bound, best, n_live = ctypes.c_int64(1234), ctypes.c_int32(1234), ctypes.c_int64(1234)
        table = (ctypes.c_void_p * 1)(lam.ctypes.data)

        def call(cand=None, n_cand=None, given=None, n_given=None, k=2, iters=5, step0=0, h=hist):
            c = None if cand is None else np.asarray(cand, dtype=np.int64)
            g = None if given is None else np.asarray(given, dtype=np.int64)
            return lib.utm_coverage_bound(mat._h, p(c), (0 if c is None else len(c)) if n_cand is None else n_cand, p(g),
                                          (0 if g is None else len(g)) if n_given is None else n_given, k, iters, step0, 0, p(h),
                                          ctypes.byref(bound), ctypes.byref(best), ctypes.byref(n_live), table, None)

        assert call(h=None) == EINVAL                                    # NULL hist_out
        assert call(n_cand=2) == EINVAL and call(n_given=1) == EINVAL    # NULL lists with a length
        assert call(cand=[1, 30]) == EINVAL and call(given=[-1]) == EINVAL
        assert call(cand=[4, 5, 4]) == EINVAL and call(given=[7, 7]) == EINVAL
        assert call(k=0) == EINVAL and call(iters=0) == EINVAL and call(iters=65536) == EINVAL and call(step0=Q + 1) == EINVAL
        assert (hist == 1234).all() and (lam == 1234).all()
        assert (bound.value, best.value, n_live.value) == (1234, 1234, 1234)
        assert (mat.covered(0) == covered).all() and deterministic(mat.stats()) == stats
        assert call(cand=[7, 8, 1], given=[2]) == 0
        want = bound_ref.coverage_bound(dense, 2, cand=[7, 8, 1], given=[2], iters=5)
        assert hist.tolist() == want["hist"].tolist() and np.array_equal(lam, want["lambdas"])
        assert (bound.value, best.value, n_live.value) == (want["bound"], want["best_iter"], want["n_live"])
        assert len(mat.run(5)[0]) == 5


def test_a_shard_refuses_and_works_afterwards(dev):
    n_var = 2000
    cols = npo.pack_columns(seeded(n_var, 8))
    with dev.DeviceMatrix(10, first_sample=2, n_local=8) as m:
        c = m.add_chunk(n_var)
        m.upload_columns(c, cols)
        with pytest.raises(dev.nat.NativeError) as e:
            m.coverage_bound(2, iters=3)
        assert e.value.code == ESTATE
        assert m.var_count().tolist() == np.bitwise_count(cols).sum(axis=1).tolist()     # the context still answers


def test_kernel_times_are_kept_only_with_profile_events(dev):
    n_var, n_samp = 8191, 70
    cols = npo.pack_columns(seeded(n_var, n_samp))
    with uploaded(dev, [cols], [n_var]) as plain, uploaded(dev, [cols], [n_var], profile_events=True) as timed:
        a, b = plain.coverage_bound(5, iters=T), timed.coverage_bound(5, iters=T)
        assert a.hist.tolist() == b.hist.tolist()
        assert plain.coverage_bound_times() == (0.0, 0.0, 0.0)
        assert all(ms > 0 for ms in timed.coverage_bound_times())
