"""The coverage bound without a GPU: the CPU build (utm_coverage_bound_host) against the numpy restatement
(tests/bound_ref.py) bit for bit, its validity against the exhaustive optimum of tiny instances, the cases with a known
answer, the tie rule, `given`, and the argument errors."""
import ctypes

import numpy as np
import pytest

import bound_ref
import oracle_util as ou
from bound_ref import Q, SENT, host_bound, p
from oracle_util import npo

EINVAL = -1


def same(got, want):
    assert got["hist"].tolist() == want["hist"].tolist()
    assert (got["bound"], got["best_iter"], got["n_live"]) == (want["bound"], want["best_iter"], want["n_live"])
    assert got["lambdas"].tolist() == want["lambdas"].tolist()


@pytest.mark.parametrize("n_samp", [1, 17, 70])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 8191])
def test_cpu_build_equals_the_restatement(n_var, n_samp):
    rng = np.random.default_rng(n_var * 100 + n_samp)
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    cand = rng.permutation(n_samp)[:max(1, n_samp - 2)]
    n_c = len(cand)
    for k in sorted({1, 5, n_c, n_c + 3}):
        for kw in (dict(period=2), dict(step0=1), dict(period=2, wp=cols.shape[1] + 3), dict()):
            ref_kw = {a: b for a, b in kw.items() if a != "wp"}
            same(host_bound(cols, n_var, k, cand=cand, **kw), bound_ref.coverage_bound(dense, k, cand=cand, iters=12, **ref_kw))
    same(host_bound(cols, n_var, 3, period=2), bound_ref.coverage_bound(dense, 3, iters=12, period=2))   # NULL list: everyone


def test_every_bound_is_at_or_above_the_exhaustive_optimum():
    rng = np.random.default_rng(11)
    for case in range(32):
        n_samp, n_var, k = int(rng.integers(6, 13)), int(rng.integers(10, 60)), int(rng.integers(1, 5))
        dense = rng.random((n_var, n_samp)) < rng.uniform(0.1, 0.5)
        cols = npo.pack_columns(dense)
        best = bound_ref.exhaustive_optimum(dense, k)
        for iters in (1, 7, 60):
            got = host_bound(cols, n_var, k, iters=iters)
            assert (got["hist"] // Q >= best).all(), (case, iters)
            assert got["bound"] >= best
        rows = list(npo.greedy(dense, dense.sum(axis=0), k, np.arange(n_samp), np.ones(n_samp, np.uint8)))
        order = [int(r[0]) for r in rows]
        assert bound_ref.online_bound(dense, order, k, np.arange(n_samp)) >= best, case


def test_disjoint_columns_are_bounded_exactly_at_once():
    dense = np.zeros((30, 5), bool)
    for s, (lo, hi) in enumerate([(0, 3), (3, 10), (10, 12), (12, 24), (24, 30)]):
        dense[lo:hi, s] = True
    got = host_bound(npo.pack_columns(dense), 30, 2, iters=3)
    assert got["hist"][0] == (12 + 7) * Q == bound_ref.exhaustive_optimum(dense, 2) * Q
    assert got["bound"] == 19 and got["best_iter"] == 0


def test_identical_columns_reach_their_count():
    n = 100
    dense = np.ones((n, 6), bool)
    for k in (2, 3):                                                   # step Q/4 held for five iterations: lambda reaches 0 by t = 4
        got = host_bound(npo.pack_columns(dense), n, k, iters=6, period=5)
        assert got["hist"][0] == k * n * Q                             # the trivial bound counts every column again
        assert n * Q in got["hist"][:5].tolist()
        assert got["bound"] == n


def test_with_no_more_candidates_than_k_the_bound_is_their_union():
    rng = np.random.default_rng(5)
    dense = rng.random((500, 9)) < 0.2
    cand = [7, 2, 4]
    for k in (3, 8):
        got = host_bound(npo.pack_columns(dense), 500, k, cand=cand, iters=60)
        assert got["bound"] == bound_ref.captured(dense, cand)


def test_a_tie_goes_to_the_earlier_position_in_the_list():
    """Samples 1 and 2 carry four variants each, different ones, and tie for the second place of k = 2 beside sample 0.  (At
    k = 1 no tie can matter: c_v - 1 is never positive there, so lambda stays at Q and the history is constant.)"""
    dense = np.zeros((12, 3), bool)
    dense[[0, 2, 4, 6, 8, 9, 10], 0] = True
    dense[[2, 4, 9, 10], 1] = True
    dense[[0, 1, 6, 10], 2] = True
    cols = npo.pack_columns(dense)
    a, b = host_bound(cols, 12, 2, cand=[0, 1, 2], period=2), host_bound(cols, 12, 2, cand=[0, 2, 1], period=2)
    same(a, bound_ref.coverage_bound(dense, 2, cand=[0, 1, 2], iters=12, period=2))
    same(b, bound_ref.coverage_bound(dense, 2, cand=[0, 2, 1], iters=12, period=2))
    assert a["hist"][0] == b["hist"][0] == 11 * Q
    assert a["hist"][1:].tolist() != b["hist"][1:].tolist()             # the order of the list decided the pick
    one = host_bound(cols, 12, 1, cand=[0, 1, 2], period=2)
    assert (one["hist"] == 7 * Q).all()


def test_given_is_the_call_on_the_rows_no_given_sample_carries():
    rng = np.random.default_rng(9)
    dense = ou.random_dense(rng, 700, 20)
    given, cand = [3, 11], [s for s in range(20) if s not in (3, 11)]
    rest = ~dense[:, given].any(axis=1)
    got = host_bound(npo.pack_columns(dense), 700, 4, cand=cand, given=given, period=2)
    want = host_bound(npo.pack_columns(dense[rest]), int(rest.sum()), 4, cand=cand, period=2)
    assert got["hist"].tolist() == want["hist"].tolist() and got["n_live"] == want["n_live"] == int(rest.sum())
    assert got["lambdas"][rest].tolist() == want["lambdas"].tolist() and (got["lambdas"][~rest] == 0).all()
    same(got, bound_ref.coverage_bound(dense, 4, cand=cand, given=given, iters=12, period=2))
    # a sample in both lists has no live variants: it adds nothing
    both = host_bound(npo.pack_columns(dense), 700, 4, cand=cand + [3], given=given, period=2)
    assert both["hist"].tolist() == got["hist"].tolist() and both["lambdas"].tolist() == got["lambdas"].tolist()


def test_bad_arguments_are_refused_and_leave_the_outputs():
    from utmos_amd import _native as nat
    lib = nat.lib()
    cols = np.zeros((4, 1), np.uint64)
    bad = [dict(cand=[0, 4]), dict(cand=[1, 1]), dict(given=[9]), dict(given=[2, 2]), dict(k=0), dict(k=-3), dict(iters=0),
           dict(iters=65536), dict(step0=Q + 1)]
    for kw in bad:
        args = dict(k=2, iters=5)
        args.update(kw)
        rc, out = host_bound(cols, 10, args.pop("k"), want_rc=True, **args)
        assert rc == EINVAL and lib.utm_last_error(), kw
        assert (out["hist"] == SENT).all() and (out["lambdas"] == SENT).all(), kw
        assert (out["bound"], out["best_iter"], out["n_live"]) == (SENT, SENT, SENT), kw
    i64, i32 = ctypes.c_int64(SENT), ctypes.c_int32(SENT)
    hist = np.full(5, SENT, np.int64)
    call = lambda cand, n_cand, given, n_given, h: lib.utm_coverage_bound_host(p(cols), 1, 10, 4, cand, n_cand, given, n_given, 2, 5, 0, 0, h,
                                                                               ctypes.byref(i64), ctypes.byref(i32), ctypes.byref(i64), None)
    assert call(None, 0, None, 0, None) == EINVAL                       # NULL hist_out
    assert call(None, 2, None, 0, p(hist)) == EINVAL                    # NULL lists with a length
    assert call(None, 0, None, 1, p(hist)) == EINVAL
    assert (hist == SENT).all() and i64.value == SENT and i32.value == SENT
    assert lib.utm_coverage_bound_host(p(cols), 1, 65, 4, None, 0, None, 0, 2, 5, 0, 0, p(hist), None, None, None, None) == EINVAL  # more variants than words
    assert call(None, 0, None, 0, p(hist)) == 0 and (hist == 0).all()   # an empty matrix: nothing to capture


# ----------------------------------------------------------------- command line
@pytest.mark.parametrize("extra,word", [(["--af"], "--af"), (["--weights", "w.txt"], "--weights"), (["--depth", "2"], "--depth")])
def test_the_bound_is_refused_where_the_objective_is_not_the_plain_count(extra, word, capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as err:
        select.parse_args(["--bound-out", "b.tsv"] + extra + ["x.npz"])
    message = capsys.readouterr().err
    assert err.value.code == 1 and "--bound-out" in message and word in message
    select.parse_args(extra + ["x.npz"])                                 # (without the flag the same options pass)
    select.parse_args(["--bound-out", "b.tsv", "--groups", "g.tsv", "--group-max", "2", "x.npz"])    # a quota is allowed


def test_bound_flags_need_bound_out_and_sane_values(capsys):
    from utmos_amd import select
    for argv in (["--bound-at", "3"], ["--bound-iters", "10"], ["--bound-out", "b.tsv", "--bound-iters", "0"],
                 ["--bound-out", "b.tsv", "--bound-iters", "65536"], ["--bound-out", "b.tsv", "--bound-at", "0"],
                 ["--bound-out", "b.tsv", "--bound-at", "x"]):
        with pytest.raises(SystemExit) as err:
            select.parse_args(argv + ["x.npz"])
        assert err.value.code == 1, argv
    args = select.parse_args(["--bound-out", "b.tsv", "--bound-at", "3,8", "--bound-iters", "50", "x.npz"])
    assert (args.bound_out, args.bound_at, args.bound_iters) == ("b.tsv", "3,8", 50)


def test_a_size_within_the_include_samples_and_several_processes_are_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--bound-out", "b.tsv", "--include", "A,B", "--bound-at", "2", "does_not_exist.npz"])
    assert err.value.code == 1 and "--bound-at 2" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as err:
        select.select_main(["--bound-out", "b.tsv", "does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_the_flags_default_to_off_and_are_not_in_the_options_line_then(capsys):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])
    assert args.bound_out is None and args.bound_at is None and args.bound_iters is None
    line = capsys.readouterr().err
    assert "options in effect" in line and "bound" not in line


def test_the_online_bound_from_the_table_equals_its_definition():
    """utmos_amd.bound.online_bound works on the (new, missed) table of samples.sample_table; here that table comes from
    the dense matrix by definition."""
    from utmos_amd.bound import online_bound
    rng = np.random.default_rng(4)
    dense = ou.random_dense(rng, 400, 15)
    order = np.asarray([3, 8, 1, 12, 5])
    rank = np.full(400, -1)
    for i, s in reversed(list(enumerate(order))):
        rank[dense[:, s]] = i
    new = np.stack([(dense & (rank == i)[:, None]).sum(axis=0) for i in range(len(order))], axis=1)
    missed = (dense & (rank < 0)[:, None]).sum(axis=0)
    prefix = np.concatenate([[0], np.cumsum([(rank == i).sum() for i in range(len(order))])])
    for given, size in (([], 5), ([], 3), ([3, 8], 5), ([12], 4), ([14], 5)):
        cand = np.asarray([s for s in range(15) if s not in given and s != 7])
        assert online_bound(new, missed, prefix, order, size, cand, given) == bound_ref.online_bound(dense, order, size, cand, given)
