"""Pair counts without a GPU: the CPU build of k_swap_masks / k_pair_counts (utm_pair_counts_host) against the numpy
restatement by definition (tests/pair_ref.py), its identities, the reference's own recorded score vectors, the refusals
of the ABI, utmos_amd/overlap.py's row composition and the command line's refusals."""
import ctypes

import numpy as np
import pytest

import oracle_util as ou
import pair_ref
from oracle_util import npo

EINVAL = -1
N_SAMP = 140
LISTS = (0, 1, 2, 63, 64, 65, 130)


def host_pairs(cols, indices, n_var, given=()):
    """The n x n matrix of one chunk by the CPU build; prefilled so that a value that is not written shows."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx, panel = np.ascontiguousarray(indices, dtype=np.uint32), np.ascontiguousarray(given, dtype=np.uint32)
    out = np.full((len(idx), len(idx)), 77, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None
    nat.check(nat.lib().utm_pair_counts_host(cols.ctypes.data_as(ctypes.c_void_p), cols.shape[1], n_var, cols.shape[0], p(idx), len(idx),
                                             p(panel), len(panel), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def host_swap_new(cols, panel, n_var):
    """new_out of utm_swap_gains_host: per sample, the variants it carries and no panel member does."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    panel32 = np.ascontiguousarray(panel, dtype=np.uint32)
    gains, new = np.zeros((len(panel32), cols.shape[0]), np.int64), np.zeros(cols.shape[0], np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_swap_gains_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(panel32), len(panel32), p(gains), None, p(new), None))
    return new


def filled(rng, n_var, n_samp, fill):
    dense = ou.random_dense(rng, n_var, n_samp) if fill == "sparse" else ou.random_dense(rng, n_var, n_samp, density=0.65, sfs=False)
    return npo.pack_columns(dense)


# ----------------------------------------------------------------- the CPU build against the restatement
@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 1000])
def test_cpu_build_equals_the_restatement_and_its_identities_hold(n_var, fill):
    rng = np.random.default_rng(n_var + len(fill))
    cols = filled(rng, n_var, N_SAMP, fill)
    popcount = np.bitwise_count(cols).sum(axis=1, dtype=np.int64)
    for n in LISTS:
        for n_given in (0, 1, 5):
            order = rng.permutation(N_SAMP)                              # (not in index order)
            indices, given = order[:n], order[N_SAMP - n_given:] if n_given else order[:0]
            if n >= 2 and n_given:
                given = np.concatenate([given[:-1], indices[1:2]])       # one sample in both lists
            got = host_pairs(cols, indices, n_var, given)
            assert got.shape == (n, n) and (got == pair_ref.pair_counts(cols, indices, n_var, given)).all(), (n, n_given)
            if n <= 65:
                assert (got == pair_ref.pair_counts_unpacked(cols, indices, n_var, given)).all(), (n, n_given)
            assert (got == got.T).all()
            if n_given == 0:
                assert (np.diagonal(got) == popcount[indices]).all()
            else:
                assert (np.diagonal(got) == host_swap_new(cols, given, n_var)[indices]).all()
                if n >= 2:
                    assert (got[1] == 0).all() and (got[:, 1] == 0).all()    # the sample that is given as well
            if n:
                assert (got <= np.diagonal(got)[:, None]).all() and (got >= 0).all()


@pytest.mark.parametrize("n_var,n,n_given", [(1, 1, 0), (65, 2, 1), (1000, 7, 5), (200, 65, 3), (1000, 130, 0)])
def test_the_packed_restatement_equals_the_unpacked_definition(n_var, n, n_given):
    rng = np.random.default_rng(n_var + n)
    cols = filled(rng, n_var, N_SAMP, "sparse")
    order = rng.permutation(N_SAMP)
    indices, given = order[:n], order[n - 1:n - 1 + n_given]             # (overlapping by one sample when given)
    assert (pair_ref.pair_counts(cols, indices, n_var, given) == pair_ref.pair_counts_unpacked(cols, indices, n_var, given)).all()


def test_the_hand_case():
    dense = np.zeros((6, 3), bool)                                       # A = {1,2,3,4}, B = {1,2,5}, C = {3,4,6}
    dense[[0, 1, 2, 3], 0] = True
    dense[[0, 1, 4], 1] = True
    dense[[2, 3, 5], 2] = True
    cols = npo.pack_columns(dense)
    assert host_pairs(cols, [0, 1, 2], 6).tolist() == [[4, 2, 2], [2, 3, 0], [2, 0, 3]]
    assert host_pairs(cols, [2, 0], 6).tolist() == [[3, 2], [2, 4]]
    assert host_pairs(cols, [0, 1, 2], 6, given=[1]).tolist() == [[2, 0, 2], [0, 0, 0], [2, 0, 3]]


def test_padding_bits_of_the_last_word_are_cut_from_the_mask():
    cols = np.zeros((3, 2), np.uint64)
    cols[0, 0] = 0b0011
    cols[1, 0] = 0b0110
    cols[2, 1] = np.uint64(1) << np.uint64(2)                            # variant 66 of 67
    assert host_pairs(cols, [0, 1, 2], 67).tolist() == [[2, 1, 0], [1, 2, 0], [0, 0, 1]]
    assert host_pairs(cols, [0, 1], 67, given=[2]).tolist() == [[2, 1], [1, 2]]
    assert host_pairs(cols, [1, 2], 67, given=[0]).tolist() == [[1, 0], [0, 1]]


# ----------------------------------------------------------------- anchored on the reference's own score vectors
def integer_traces():
    """Recorded runs of the reference that carry every sample's score of every iteration, count integers, weigh nothing
    and start from no used sample."""
    names = []
    for name in ou.trace_names():
        t = ou.load_trace(name)
        if "scores_hex" not in t or "idx" not in t or "state" in t or "weight_vector_hex" in t or len(t["scores_hex"]) < 2:
            continue
        kw = ou.trace_options(t)
        if kw.get("af") or kw.get("weights"):
            continue
        names.append(name)
    return names


def test_there_are_traces_to_anchor_on():
    assert len(integer_traces()) >= 2


@pytest.mark.parametrize("name", integer_traces())
def test_shared_counts_are_what_the_references_first_pick_takes_from_every_score(name):
    t = ou.load_trace(name)
    kw = ou.trace_options(t)
    matrix, _, samples = npo.build_matrix(t["part_list"])
    state = npo.initial_state(samples, kw.get("subset"), kw.get("exclude"))
    scores = [np.array([float.fromhex(x) for x in vec]) for vec in t["scores_hex"][:2]]
    w = t["idx"][0]                                                      # the first winner
    cols = npo.pack_columns(np.asarray(matrix) != 0)
    shared = host_pairs(cols, np.arange(len(samples)), matrix.shape[0])
    scored = np.flatnonzero(np.asarray(state) == 1)                      # (a masked sample's score is 0, not its count)
    assert w in scored and len(scored) >= 2
    assert (np.diagonal(shared)[scored] == scores[0][scored]).all()
    others = scored[scored != w]
    assert (shared[w][others] == scores[0][others] - scores[1][others]).all()


# ----------------------------------------------------------------- refusals of the ABI
def test_cpu_build_refuses_bad_arguments_and_leaves_out():
    from utmos_amd import _native as nat
    lib = nat.lib()
    cols = np.zeros((4, 1), np.uint64)
    out = np.full((2, 2), 5, np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    u32 = lambda a: None if a is None else np.asarray(a, np.uint32)

    def call(idx, n, given=None, n_given=0, dest=out, n_var=10):
        return lib.utm_pair_counts_host(p(cols), 1, n_var, 4, p(u32(idx)), n, p(u32(given)), n_given, p(dest))

    assert call(None, 2) == EINVAL                                       # NULL list with a nonzero length
    assert call([0, 1], 2, None, 1) == EINVAL                            # ... the given list
    assert call([0, 1], 2, dest=None) == EINVAL                          # NULL out with n > 0
    assert call([0, 4], 2) == EINVAL and b"not in" in lib.utm_last_error()
    assert call([0, 1], 2, [4], 1) == EINVAL and b"given" in lib.utm_last_error()
    assert call([1, 1], 2) == EINVAL and b"twice" in lib.utm_last_error()
    assert call([0, 1], 2, [2, 2], 2) == EINVAL and b"twice" in lib.utm_last_error()
    assert call([0, 1], 2, n_var=65) == EINVAL                           # more variants than words
    assert (out == 5).all()
    assert call(None, 0, dest=None) == 0 and call(None, 0, [1], 1) == 0 and (out == 5).all()   # n == 0 writes nothing
    assert call([2, 0], 2) == 0 and (out == 0).all()                     # an empty matrix: nothing shared
    assert lib.utm_pair_counts(None, None, 0, None, 0, 0, None, None) == EINVAL and b"ctx" in lib.utm_last_error()


# ----------------------------------------------------------------- the rows of the command
def test_pair_rows_compose_round_and_handle_an_empty_union():
    from utmos_amd.overlap import pair_rows
    shared = np.array([[3, 1, 0, 0], [1, 4, 2, 0], [0, 2, 2, 0], [0, 0, 0, 0]])
    names = ["a", "b", "c", "z"]
    rows = pair_rows(shared, names, "jaccard", -1)
    assert len(rows) == 6 and all(len(r) == 7 for r in rows)
    by_pair = {(r[0], r[1]): r for r in rows}
    assert by_pair[("a", "b")] == ["a", "b", 3, 4, 1, round(1 / 6, 4), 6] and by_pair[("a", "b")][5] == 0.1667
    assert by_pair[("b", "c")] == ["b", "c", 4, 2, 2, 0.5, 4]
    assert by_pair[("a", "c")] == ["a", "c", 3, 2, 0, 0.0, 5]
    assert by_pair[("c", "z")] == ["c", "z", 2, 0, 0, 0.0, 2]
    empty = pair_rows(np.zeros((2, 2), np.int64), ["x", "y"], "jaccard", -1)
    assert empty == [["x", "y", 0, 0, 0, 0.0, 0]]                        # an empty union: 0, not a division by zero
    assert pair_rows(np.zeros((1, 1), np.int64), ["x"]) == [] and pair_rows(np.zeros((0, 0), np.int64), []) == []


def test_pair_rows_sort_keys_tie_order_and_top():
    from utmos_amd.overlap import pair_rows
    shared = np.array([[3, 1, 0, 0], [1, 4, 2, 0], [0, 2, 2, 0], [0, 0, 0, 0]])
    names = ["a", "b", "c", "z"]
    pairs = lambda rows: [(r[0], r[1]) for r in rows]
    # jaccard: 0.5, 0.1667, then four zeros in (a, b) order
    assert pairs(pair_rows(shared, names, "jaccard", -1)) == [("b", "c"), ("a", "b"), ("a", "c"), ("a", "z"), ("b", "z"), ("c", "z")]
    # joint: ab 6, ac 5, then bc = bz = 4 (the smaller b first), az 3, cz 2
    assert pairs(pair_rows(shared, names, "joint", -1)) == [("a", "b"), ("a", "c"), ("b", "c"), ("b", "z"), ("a", "z"), ("c", "z")]
    # shared: bc 2, ab 1, then zeros in (a, b) order
    assert pairs(pair_rows(shared, names, "shared", -1)) == [("b", "c"), ("a", "b"), ("a", "c"), ("a", "z"), ("b", "z"), ("c", "z")]
    assert pairs(pair_rows(shared, names, "shared", 2)) == [("b", "c"), ("a", "b")]
    assert pair_rows(shared, names, "shared", 0) == [] and len(pair_rows(shared, names)) == 6    # (default top = 20)
    tied = np.array([[2, 1, 1], [1, 2, 1], [1, 1, 2]])
    assert pairs(pair_rows(tied, ["p", "q", "r"], "jaccard", -1)) == [("p", "q"), ("p", "r"), ("q", "r")]
    with pytest.raises(ValueError):
        pair_rows(shared, names, "count", -1)
    with pytest.raises(ValueError):
        pair_rows(shared, names[:3])


def test_the_tsv_of_the_rows(tmp_path):
    from utmos_amd import overlap
    path = tmp_path / "pairs.tsv"
    with open(path, "w") as fout:
        overlap.write_pairs(fout, overlap.pair_rows(np.array([[3, 1], [1, 4]]), ["a", "b"]))
    assert open(path).read() == "sample_a\tsample_b\tcount_a\tcount_b\tshared\tjaccard\tjoint\na\tb\t3\t4\t1\t0.1667\t6\n"


# ----------------------------------------------------------------- command line
def test_the_command_is_listed():
    from utmos_amd import __main__ as cli
    assert "overlap" in cli.COMMANDS and "  overlap " in cli._usage()


def test_several_processes_are_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import overlap, select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        overlap.overlap_main(["does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_af_is_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import overlap, select
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        overlap.overlap_main(["--af", "does_not_exist.npz"])
    assert err.value.code == 1 and "--af" in capsys.readouterr().err


def test_unusable_inputs_and_options_are_refused(monkeypatch, capsys):
    from utmos_amd import overlap
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv in ([], ["does_not_exist.npz"], ["a.utm", "b.npz"], ["--top", "-2", "x.npz"]):
        with pytest.raises(SystemExit) as err:
            overlap.parse_args(argv)
        assert err.value.code == 1, argv
    with pytest.raises(SystemExit) as err:
        overlap.parse_args(["--sort", "count", "x.npz"])                 # (argparse's own refusal)
    assert err.value.code == 2


def test_an_unknown_given_name_exits_naming_it(capsys):
    from utmos_amd import overlap
    assert overlap.resolve_given(np.array(["a", "b", "c"]), ["c", "a", "c"]).tolist() == [2, 0]
    assert overlap.resolve_given(np.array(["a"]), None).tolist() == []
    with pytest.raises(SystemExit) as err:
        overlap.resolve_given(np.array(["a", "b"]), ["b", "nobody"])
    assert err.value.code == 1 and "nobody" in capsys.readouterr().err
