"""Swap gains without a GPU: the CPU build of k_swap_masks / k_swap_pairs (utm_swap_gains_host) against the numpy
restatement by definition (tests/swap_ref.py), the hand case, utmos_amd/refine.py backed by the CPU build, and the
command line's refusals."""
import ctypes

import numpy as np
import pytest

import oracle_util as ou
import swap_ref
from oracle_util import npo

EINVAL = -1
N_SAMP = 80


def host_swap(cols, panel, n_var):
    """(gains, unique, new, base) of one chunk by the CPU build; every output is prefilled so that a value that is not
    written shows."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    panel32 = np.ascontiguousarray(panel, dtype=np.uint32)
    k, n = len(panel32), cols.shape[0]
    gains, unique, new = np.full((k, n), 77, np.int64), np.full(k, 77, np.int64), np.full(n, 77, np.int64)
    base = ctypes.c_int64(77)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_swap_gains_host(p(cols), cols.shape[1], n_var, n, p(panel32), k, p(gains), p(unique), p(new), ctypes.byref(base)))
    return gains, unique, new, base.value


class HostMatrix:
    """What refine() needs of a DeviceMatrix, backed by the CPU build."""

    def __init__(self, cols, n_var):
        self.cols, self.n_var, self.calls = cols, n_var, 0

    def swap_gains(self, panel):
        self.calls += 1
        return host_swap(self.cols, panel, self.n_var)


def filled(rng, n_var, n_samp, fill):
    dense = ou.random_dense(rng, n_var, n_samp) if fill == "sparse" else ou.random_dense(rng, n_var, n_samp, density=0.65, sfs=False)
    return npo.pack_columns(dense)


@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 1000])
def test_cpu_build_equals_the_restatement(n_var, fill):
    rng = np.random.default_rng(n_var + len(fill))
    cols = filled(rng, n_var, N_SAMP, fill)
    for k in (0, 1, 2, 63, 64, 65):
        panel = rng.permutation(N_SAMP)[:k]
        gains, unique, new, base = host_swap(cols, panel, n_var)
        want, want_base = swap_ref.swap_gains(cols, panel, n_var)
        if k == 0:
            assert base == 0 and (new == 77).all()                       # base = 0, nothing else is written
            continue
        assert base == want_base and (gains == want).all(), k
        assert (unique == swap_ref.unique_counts(cols, panel, n_var)).all(), k
        assert (new == swap_ref.new_counts(cols, panel, n_var)).all(), k
        # the formula's two fixed points: a member for itself changes nothing, for another member it only loses
        for i, member in enumerate(panel):
            assert gains[i, member] == 0
            others = np.delete(panel, i)
            assert (gains[i, others] == -unique[i]).all()


@pytest.mark.parametrize("n_var,k", [(1, 1), (65, 2), (1000, 7), (200, 65)])
def test_the_packed_restatement_equals_the_unpacked_definition(n_var, k):
    rng = np.random.default_rng(n_var)
    cols = filled(rng, n_var, 30 if k < 30 else N_SAMP, "sparse")
    panel = rng.permutation(cols.shape[0])[:k]
    fast, slow = swap_ref.swap_gains(cols, panel, n_var), swap_ref.swap_gains_unpacked(cols, panel, n_var)
    assert fast[1] == slow[1] and (fast[0] == slow[0]).all()


def test_padding_bits_of_the_last_word_do_not_count():
    cols = np.zeros((3, 2), np.uint64)
    cols[0, 0] = 0b0011
    cols[1, 0] = 0b0110
    cols[2, 1] = np.uint64(1) << np.uint64(2)                            # variant 66
    gains, unique, new, base = host_swap(cols, [0], 67)
    assert base == 2 and unique.tolist() == [2] and new.tolist() == [0, 1, 1]
    assert gains.tolist() == [[0, 0, -1]]                                # sample 1: wins one, wins back one, loses two; sample 2: wins one, loses two


def test_cpu_build_refuses_bad_arguments_and_leaves_the_outputs():
    from utmos_amd import _native as nat
    lib = nat.lib()
    cols = np.zeros((4, 1), np.uint64)
    gains, unique, new = np.full((2, 4), 5, np.int64), np.full(2, 5, np.int64), np.full(4, 5, np.int64)
    base = ctypes.c_int64(5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = lambda panel, k, g=gains, n_var=10: lib.utm_swap_gains_host(p(cols), 1, n_var, 4, None if panel is None else p(np.asarray(panel, np.uint32)),
                                                                      k, None if g is None else p(g), p(unique), p(new), ctypes.byref(base))
    assert call(None, 2) == EINVAL                                       # NULL panel with k > 0
    assert call([0, 1], 2, g=None) == EINVAL                             # NULL gain_out with k > 0
    assert call([0, 4], 2) == EINVAL and b"not in" in lib.utm_last_error()
    assert call([1, 1], 2) == EINVAL and b"twice" in lib.utm_last_error()
    assert call([0, 1], 2, n_var=65) == EINVAL                           # more variants than words
    assert (gains == 5).all() and (unique == 5).all() and (new == 5).all() and base.value == 5
    assert call(None, 0, g=None) == 0 and base.value == 0 and (new == 5).all()
    assert lib.utm_swap_gains_host(p(cols), 1, 10, 4, p(np.asarray([2, 0], np.uint32)), 2, p(gains), None, None, None) == 0
    assert (gains == 0).all()                                            # an empty matrix: nothing to win or lose


# ----------------------------------------------------------------- the hand case
# A = {1,2,3,4}, B = {1,2,5}, C = {3,4,6} over 6 variants: greedy takes A (4), then B (+1) = 5; [C, B] captures all 6.
A, B, C = 0, 1, 2


def hand_case():
    dense = np.zeros((6, 3), bool)
    dense[[0, 1, 2, 3], A] = True
    dense[[0, 1, 4], B] = True
    dense[[2, 3, 5], C] = True
    return npo.pack_columns(dense), dense


def test_hand_case_gains():
    cols, dense = hand_case()
    rows = list(npo.greedy(dense, dense.sum(axis=0), 2, np.array(["A", "B", "C"]), np.ones(3, np.uint8)))
    assert [r[0] for r in rows] == ["A", "B"] and rows[-1][3] == 5
    gains, unique, new, base = host_swap(cols, [A, B], 6)
    assert base == 5 and unique.tolist() == [2, 1] and new.tolist() == [0, 0, 1]
    assert gains[0].tolist() == [0, -2, 1]                               # A leaves: +1 with C
    assert gains[1].tolist() == [-1, 0, 0]                               # B leaves: 0 with C


def test_refine_on_the_hand_case_ends_at_c_b_after_one_swap():
    from utmos_amd.refine import refine
    cols, _ = hand_case()
    m = HostMatrix(cols, 6)
    panel, log = refine(m, [A, B], np.ones(3, np.uint8))
    assert panel == [C, B] and log == [(1, A, C, 1, 6)]
    assert m.calls == 2                                                  # the second round finds nothing
    assert host_swap(cols, panel, 6)[3] == 6


def test_refine_respects_pinned_members_and_max_swaps_and_states():
    from utmos_amd.refine import refine
    cols, _ = hand_case()
    ones = np.ones(3, np.uint8)
    assert refine(HostMatrix(cols, 6), [A, B], ones, pinned=[A]) == ([A, B], [])       # only B may leave: 0 at best
    m = HostMatrix(cols, 6)
    assert refine(m, [A, B], ones, max_swaps=0) == ([A, B], []) and m.calls == 0
    assert refine(HostMatrix(cols, 6), [A, B], ones, max_swaps=1)[0] == [C, B]
    assert refine(HostMatrix(cols, 6), [A, B], np.array([1, 1, 2], np.uint8)) == ([A, B], [])   # C is excluded: nobody to bring in
    assert refine(HostMatrix(cols, 6), [], ones) == ([], [])


def test_ties_go_to_the_smallest_position_then_the_smallest_sample():
    from utmos_amd.refine import best_swap
    gains = np.array([[0, 3, 1, 3], [0, 3, 3, 9], [0, 9, 0, 9]])
    panel, everyone = [0, 5, 6], np.array([False, True, True, True])
    assert best_swap(gains, panel, everyone) == (9, 1, 3)                # position 1 before position 2
    assert best_swap(gains, panel, everyone, pinned=[5]) == (9, 2, 1)    # ... then sample 1 before sample 3
    assert best_swap(gains, panel, np.array([False, False, True, False])) == (3, 1, 2)
    assert best_swap(gains, panel, everyone, pinned=[0, 5, 6]) is None
    assert best_swap(gains, panel, np.zeros(4, bool)) is None


def test_refine_on_a_random_matrix_ends_where_no_swap_helps_and_the_log_adds_up():
    from utmos_amd.refine import refine
    rng = np.random.default_rng(3)
    n_var, n_samp, k = 3000, 60, 8
    dense = ou.random_dense(rng, n_var, n_samp)
    cols = npo.pack_columns(dense)
    states = np.ones(n_samp, np.uint8)
    states[[4, 9]] = 2
    rows = list(npo.greedy(dense, dense.sum(axis=0), k, np.arange(n_samp), states.copy()))
    start = [int(r[0]) for r in rows]
    worse = start[:-2] + [s for s in range(n_samp) if s not in start and states[s] == 1][:2]   # a panel with room to improve
    panel, log = refine(HostMatrix(cols, n_var), worse, states)
    assert log and [e[0] for e in log] == list(range(1, len(log) + 1)) and all(e[3] > 0 for e in log)
    base0 = swap_ref.swap_gains(cols, worse, n_var)[1]
    gains, base = swap_ref.swap_gains(cols, panel, n_var)
    assert base == log[-1][4] == base0 + sum(e[3] for e in log)
    candidates = (states == 1) & ~np.isin(np.arange(n_samp), panel)
    assert gains[:, candidates].max() <= 0                               # a local optimum of the 1-swap neighbourhood
    assert not set(panel) & {4, 9} and len(set(panel)) == k


# ----------------------------------------------------------------- command line
@pytest.mark.parametrize("extra,word", [(["--af"], "--af"), (["--weights", "w.txt"], "--weights"), (["--depth", "2"], "--depth"),
                                        (["--mode", "topN"], "--mode topN"), (["--mode", "random"], "--mode random")])
def test_refine_is_refused_where_the_objective_is_not_the_plain_count(extra, word, capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as err:
        select.parse_args(["--refine", "3"] + extra + ["x.npz"])
    message = capsys.readouterr().err
    assert err.value.code == 1 and "--refine" in message and word in message
    select.parse_args(extra + ["x.npz"])                                 # (without --refine the same options pass)


def test_refine_takes_minus_one_and_refuses_less_and_refine_out_needs_it(capsys):
    from utmos_amd import select
    assert select.parse_args(["--refine", "-1", "x.npz"]).refine == -1
    for argv in (["--refine", "-2", "x.npz"], ["--refine-out", "s.tsv", "x.npz"]):
        with pytest.raises(SystemExit) as err:
            select.parse_args(argv)
        assert err.value.code == 1


def test_several_processes_refuse_refine_before_loading(monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--refine", "1", "does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_the_flags_default_to_off_and_are_not_in_the_options_line_then(capsys):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])
    assert args.refine == 0 and args.refine_out is None
    line = capsys.readouterr().err
    assert "options in effect" in line and "refine" not in line
    select.parse_args(["--refine", "2", "--refine-out", "s.tsv", "x.npz"])
    line = capsys.readouterr().err
    assert '"refine": 2' in line and '"refine_out": "s.tsv"' in line
