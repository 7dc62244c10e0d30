"""Fixed orders without a GPU: the numpy restatement against the reference-made fixtures, the order helpers, the
command line's refusals, and the CPU build of the kernel's walk."""
import ctypes
import logging

import numpy as np
import pytest

import oracle_util as ou
import order_ref


@pytest.mark.parametrize("name", order_ref.case_names())
def test_restatement_reproduces_the_reference_made_gains(name):
    t = order_ref.load_case(name)
    assert t["cols"].shape[1] * 64 >= t["n_var"] > (t["cols"].shape[1] - 1) * 64
    gains, covered = order_ref.order_curve(t["cols"], t["order"], n_var=t["n_var"])
    assert gains.tolist() == t["gains"]
    if len(t["gains"]) < len(t["order"]):                 # the prefix captured everything before its end
        assert int(np.bitwise_count(covered).sum()) == t["n_var"] and not t["cont_idx"]
    # the continuation's gains follow from its winners the same way
    more, _ = order_ref.order_curve(t["cols"], t["cont_idx"], covered=covered)
    assert more.tolist() == t["cont_gains"]
    assert [int(t["var_count"][s]) for s in t["order"][:len(gains)] + t["cont_idx"]] == t["rows_var_count"]


def test_fixtures_cover_the_cases_that_matter():
    cases = {n: order_ref.load_case(n) for n in order_ref.case_names()}
    assert any(0 in t["gains"] for t in cases.values())                                   # a member that adds nothing
    assert any(len(t["gains"]) < len(t["order"]) for t in cases.values())                 # early stop inside the prefix
    assert any(t["outside_subset"] for t in cases.values())
    assert all(t["n_var"] % 64 for t in cases.values() if "parts" in t)
    assert {t["af_dtype"] for t in cases.values()} == {None, "f64", "f32"}
    assert cases["chunks_int"]["gains"] == [59, 24, 19, 16, 16]


# ----------------------------------------------------------------- order helpers
def test_topn_order_ranks_like_repeated_first_maximum():
    from utmos_amd.select import topn_order
    scores = np.array([3.0, 7.0, 7.0, 0.0, 5.0, 7.0, -1.0, 2.0])
    states = np.array([1, 1, 1, 1, 1, 2, 1, 0], dtype=np.uint8)
    got = topn_order(scores, states)
    assert got.tolist() == [1, 2, 4, 0]                   # ties to the lower index; excluded 5, used 7, zero and negative cut
    assert got.tolist() == order_ref.topn_order(scores, states).tolist()
    assert topn_order(np.zeros(5), np.ones(5, np.uint8)).tolist() == []
    assert topn_order(np.array([-2.0, -1.0, -3.0]), np.ones(3, np.uint8)).tolist() == []  # negative weights: nothing
    rng = np.random.default_rng(5)
    for _ in range(20):
        scores = rng.integers(-2, 6, size=40).astype(np.float64) * rng.choice([0.5, 1.0, 2.5], size=40)
        states = rng.choice([0, 1, 1, 1, 2], size=40).astype(np.uint8)
        want = order_ref.topn_order(scores, states)
        assert topn_order(scores, states).tolist() == want.tolist()
        # ... which is np.argmax taken again and again with the winner masked
        left = np.where(states == 1, scores, 0.0)
        for s in want:
            assert int(np.argmax(left)) == s
            left[s] = 0.0
        assert left.max() <= 0


def test_random_order_is_seeded_and_only_takes_selectable_samples():
    from utmos_amd.select import random_order
    states = np.array([1, 0, 1, 2, 1, 1, 2, 1], dtype=np.uint8)
    a, b, c = random_order(states, 3), random_order(states, 3), random_order(states, 4)
    assert a.tolist() == b.tolist() and a.tolist() != c.tolist()
    assert sorted(a.tolist()) == [0, 2, 4, 5, 7]
    assert a.tolist() == order_ref.random_order(states, 3).tolist()
    assert a.tolist() == np.random.default_rng(3).permutation(np.array([0, 2, 4, 5, 7])).tolist()


# ----------------------------------------------------------------- command line
class _ShapeOnly:
    """Stands in for a DeviceMatrix where run_selection only looks at the shape before it refuses."""
    shape = (10, 4)


def _data():
    return {"data": _ShapeOnly(), "samples": np.array(["A", "B", "C", "D"]), "var_count": np.zeros(4, np.int64)}


def test_unknown_include_name_exits_1_and_names_it(caplog):
    from utmos_amd import select
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        select.run_selection(_data(), 2, include=["A", "NOPE"])
    assert err.value.code == 1 and "NOPE" in caplog.text


def test_include_of_an_excluded_sample_exits_1_and_names_it(caplog):
    from utmos_amd import select
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        select.run_selection(_data(), 2, exclude=["C"], include=["A", "C"])
    assert err.value.code == 1 and "C" in caplog.text


def test_include_keeps_the_order_given_and_drops_later_duplicates():
    from utmos_amd import select
    names = ["A", "B", "C", "D"]
    assert select.resolve_include(names, ["C", "A", "C", "B", "A"], ["D"]).tolist() == [2, 0, 1]
    assert select.resolve_include(names, None, None).tolist() == []
    with pytest.raises(ValueError):
        select.run_selection(_data(), 2, mode="bogus")


def test_mode_bogus_is_refused_by_the_parser(capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as err:
        select.select_main(["--mode", "bogus", "x.npz"])
    assert err.value.code == 2 and "bogus" in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--include", "A"], ["--mode", "topN"], ["--mode", "random", "--seed", "2"]])
def test_several_processes_refuse_fixed_orders_before_loading(extra, monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(extra + ["does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err   # (the command logs to stderr)


def test_new_flags_default_to_todays_command(monkeypatch):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])
    assert args.include is None and args.mode == "greedy" and args.seed == 0


# ----------------------------------------------------------------- the kernel's walk, built for the CPU
@pytest.mark.parametrize("n_samp,n_var,seed", [(1, 1, 0), (7, 63, 1), (65, 4097, 2), (40, 70000, 3)])
def test_cpu_build_of_the_curve_equals_the_restatement(n_samp, n_var, seed):
    from utmos_amd import _native as nat
    rng = np.random.default_rng(seed)
    cols = ou.npo.pack_columns(ou.random_dense(rng, n_var, n_samp))
    wp = cols.shape[1]
    covered0 = cols[rng.integers(0, n_samp)] & rng.integers(0, 2 ** 63, size=wp, dtype=np.uint64)
    for order in (np.arange(n_samp), rng.permutation(n_samp)[:max(1, n_samp // 2)], np.array([n_samp - 1])):
        covered = covered0.copy()
        counts = np.zeros(len(order), np.uint64)
        order32 = np.ascontiguousarray(order, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        nat.check(nat.lib().utm_order_curve_host(p(cols), wp, p(covered), p(order32), len(order32), p(counts)))
        gains, want = order_ref.order_curve(cols, order, covered=covered0)
        assert counts.astype(np.int64).tolist() == gains.tolist()
        assert (covered == want).all()
