"""Variant filters without a GPU: the CPU build of the compaction's word arithmetic (utm_filter_columns_host) against the
numpy restatement (tests/filter_ref.py), the criteria masks against hand-written cases, and the refusals that need no
device."""
import ctypes

import numpy as np
import pytest

import filter_ref
import oracle_util as ou
from oracle_util import npo

EINVAL = -1
N_SAMP = 70


def host_filter(cols, n_var, keep_words, wp_out):
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    out = np.full((cols.shape[0], wp_out), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)     # (every word has to be written)
    kept = ctypes.c_uint64(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nat.check(nat.lib().utm_filter_columns_host(p(cols), cols.shape[1], n_var, cols.shape[0], p(keep_words), p(out), wp_out,
                                                ctypes.byref(kept)))
    return out, kept.value


_MATRIX = {}


def matrix(n_var):
    """(dense, packed columns) of a seeded matrix, made once per size."""
    if n_var not in _MATRIX:
        dense = ou.random_dense(np.random.default_rng(n_var), n_var, N_SAMP, density=0.4, sfs=n_var % 2 == 0)
        _MATRIX[n_var] = (dense, npo.pack_columns(dense))
    return _MATRIX[n_var]


@pytest.mark.parametrize("n_var", filter_ref.SIZES)
def test_cpu_build_equals_the_restatement_word_for_word(n_var):
    dense, cols = matrix(n_var)
    names = set()
    for name, keep in filter_ref.mask_cases(n_var).items():
        kept = int(keep.sum())
        wp_out = (kept + 63) // 64 + 3                           # padding up to wp_out is part of the comparison
        want, _ = filter_ref.filter_columns(cols, n_var, keep, wp_out)
        got, n_kept = host_filter(cols, n_var, filter_ref.pack_keep(keep), wp_out)
        assert n_kept == kept, name
        assert (got == want).all(), name
        if name == "ones":
            assert (got[:, :cols.shape[1]] == cols).all()         # the identity, bit for bit
        if name == "zeros":
            assert n_kept == 0 and not got.any()
        names.add(name)
    assert {"ones", "zeros", "first", "last", "alternating", "random0.5", "alternating_words", "every_shift"} <= names
    if n_var > 8192:
        assert {"kept64", "kept8192", "aligned_mid_tile"} <= names
        assert int(filter_ref.mask_cases(n_var)["kept8192"].sum()) == 8192 and int(filter_ref.mask_cases(n_var)["kept64"].sum()) == 64


@pytest.mark.parametrize("n_var", [1, 63, 65, 8191, 100_003])
def test_garbage_above_n_var_in_the_last_keep_word_is_ignored(n_var):
    dense, cols = matrix(n_var)
    keep = filter_ref.mask_cases(n_var)["random0.5"]
    dirty = filter_ref.pack_keep(keep, garbage=True)
    assert (dirty != filter_ref.pack_keep(keep)).any()
    wp_out = (int(keep.sum()) + 63) // 64 + 1
    got, n_kept = host_filter(cols, n_var, dirty, wp_out)
    assert n_kept == int(keep.sum()) and (got == filter_ref.filter_columns(cols, n_var, keep, wp_out)[0]).all()


def test_the_restatement_is_dense_indexing():
    dense, cols = matrix(8193)
    keep = filter_ref.mask_cases(8193)["random0.5"]
    got, kept = filter_ref.filter_columns(cols, 8193, keep)
    assert (filter_ref.unpack_columns(got, kept) == dense[keep]).all()


def test_cpu_build_refuses_bad_arguments():
    from utmos_amd import _native as nat
    lib = nat.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cols, keep, out = np.zeros((2, 1), np.uint64), np.full(1, ~np.uint64(0)), np.zeros((2, 1), np.uint64)
    assert lib.utm_filter_columns_host(p(cols), 1, 64, 2, None, p(out), 1, None) == EINVAL
    assert lib.utm_filter_columns_host(None, 1, 64, 2, p(keep), p(out), 1, None) == EINVAL
    assert lib.utm_filter_columns_host(p(cols), 1, 65, 2, p(keep), p(out), 1, None) == EINVAL      # more variants than words
    assert lib.utm_filter_columns_host(p(cols), 1, 64, 2, p(keep), p(out), 0, None) == EINVAL      # 64 kept bits in no words
    assert lib.utm_filter_columns_host(p(cols), 1, 64, 2, p(keep), p(out), 1, None) == 0


# ----------------------------------------------------------------- the criteria
def test_af_bounds_are_inclusive_and_compare_exact_values():
    from utmos_amd import variant_filter as vf
    af64 = np.array([0.0, 0.01, 0.05, 0.1, 0.5, 1.0])
    assert vf.af_mask(af64, 0.01, 0.1).tolist() == [False, True, True, True, False, False]
    assert vf.af_mask(af64, None, 0.05).tolist() == [True, True, True, False, False, False]
    assert vf.af_mask(af64, 0.5, None).tolist() == [False, False, False, False, True, True]
    # float32(0.1) is 0.100000001490116...: above the float64 bound 0.1, so it passes --min-af 0.1 and fails --max-af 0.1;
    # the float64 value 0.1 passes both.  0.5 is the same number in both formats.
    af32 = af64.astype(np.float32)
    assert float(af32[3]) > 0.1
    assert vf.af_mask(af32, 0.1, None).tolist() == [False, False, False, True, True, True]
    assert vf.af_mask(af32, None, 0.1).tolist() == [True, True, True, False, False, False]
    assert vf.af_mask(af64, None, 0.1).tolist() == [True, True, True, True, False, False]
    assert vf.af_mask(af32, 0.5, 0.5).tolist() == vf.af_mask(af64, 0.5, 0.5).tolist() == [False, False, False, False, True, False]
    rng = np.random.default_rng(3)
    for af in (rng.random(500), rng.random(500).astype(np.float32)):
        assert (vf.af_mask(af, 0.2, 0.7) == filter_ref.af_keep(af, 0.2, 0.7)).all()


def test_carrier_bounds_are_inclusive_and_count_the_cohort_only():
    from utmos_amd import variant_filter as vf
    assert vf.carrier_mask([0, 1, 2, 3, 4], 2, 3).tolist() == [False, False, True, True, False]
    assert vf.carrier_mask([0, 1, 2], 2, None).tolist() == [False, False, True]
    assert vf.carrier_mask([0, 1, 2], None, 1).tolist() == [True, True, False]
    names = np.array(["A", "B", "C", "D", "E"])
    assert vf.cohort_indices(names, None, None).tolist() == [0, 1, 2, 3, 4]
    assert vf.cohort_indices(names, ["A", "C", "E"], None).tolist() == [0, 2, 4]
    assert vf.cohort_indices(names, ["A", "C", "E"], ["C"]).tolist() == [0, 4]
    assert vf.cohort_indices(names, None, ["B"]).tolist() == [0, 2, 3, 4]
    dense = np.array([[1, 1, 0, 0, 0], [1, 0, 1, 0, 1], [0, 1, 0, 1, 0]], dtype=bool)
    cohort = vf.cohort_indices(names, ["A", "C", "E"], None)
    counts = dense[:, cohort].sum(axis=1)
    assert counts.tolist() == [1, 3, 0]                           # B and D are outside the cohort
    assert vf.carrier_mask(counts, 2, None).tolist() == filter_ref.carrier_keep(dense, cohort, 2).tolist() == [False, True, False]


def test_variant_lists_keep_drop_and_refuse(tmp_path):
    from utmos_amd import variant_filter as vf
    origin = {"part": np.array([0, 0, 0, 1, 1], np.int32), "row": np.array([0, 2, 5, 0, 3], np.int64)}
    assert vf.listed_mask(origin["part"], origin["row"], [1, 0], [0, 2]).tolist() == [False, True, False, True, False]
    assert filter_ref.listed_keep(origin["part"], origin["row"], [1, 0], [0, 2]).tolist() == [False, True, False, True, False]
    with pytest.raises(vf.FilterError, match=r"part 0, row 1"):
        vf.listed_mask(origin["part"], origin["row"], [0, 0], [0, 1])         # record 1 of file 0 was dropped: nobody carries it
    with pytest.raises(vf.FilterError, match=r"part 2, row 0"):
        vf.listed_mask(origin["part"], origin["row"], [2], [0])
    good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
    np.savez(good, part=np.array([0, 1], np.int32), row=np.array([5, 3], np.int64), rank=np.array([1, -1], np.int32))
    np.savez(bad, part=np.array([0, 1], np.int32))
    assert [a.tolist() for a in vf.read_variant_list(good)] == [[0, 1], [5, 3]]
    with pytest.raises(vf.FilterError, match="no array `row`"):
        vf.read_variant_list(bad)
    crit = vf.Criteria(keep_variants=good)
    masks = vf.build_masks(crit, [2, 3], origin=origin)
    assert [m.tolist() for m in masks] == [[False, False], [True, False, True]]
    masks = vf.build_masks(vf.Criteria(drop_variants=good, max_af=0.3), [2, 3], chunk_af=[np.array([0.1, 0.4]), np.array([0.2, 0.2, 0.2])],
                           origin=origin)
    assert [m.tolist() for m in masks] == [[True, False], [False, True, False]]
    with pytest.raises(vf.FilterError, match="carries none"):
        vf.build_masks(vf.Criteria(min_af=0.1), [2, 3], chunk_af=None)


# ----------------------------------------------------------------- command line, before any device call
@pytest.mark.parametrize("flags", [["--min-af", "0.1"], ["--min-carriers", "2"], ["--keep-variants", "k.npz"], ["--drop-variants", "k.npz"]])
def test_several_processes_refuse_the_filters_before_loading(flags, monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(flags + ["does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_filter_command_refuses_several_processes(monkeypatch, capsys, tmp_path):
    from utmos_amd import select, variant_filter as vf
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        vf.filter_main(["--min-af", "0.1", "-o", str(tmp_path / "o.utm"), "x.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


class _NoAfStore:
    """Stands in for a DeviceMatrix loaded from a store written without --af: the AF criteria fail before any device call."""
    chunk_vars = [10, 20]

    def filter_variants(self, chunk, keep):
        pytest.fail("the device was called")

    def carrier_counts(self, *a, **k):
        pytest.fail("the device was called")


def test_an_input_without_af_ends_the_af_filters_with_status_1(capsys):
    from utmos_amd import select, variant_filter as vf
    with pytest.raises(vf.FilterError, match="carries none"):
        vf.apply(_NoAfStore(), vf.Criteria(max_af=0.05), ["A", "B"], chunk_af=None)
    select.setup_logging(False)
    with pytest.raises(SystemExit) as err:
        select.filter_loaded(_NoAfStore(), (vf.Criteria(max_af=0.05), None, None), ["A", "B"], None, None)
    assert err.value.code == 1 and "carries none" in capsys.readouterr().err


def test_the_flags_default_to_off_and_stay_out_of_the_options_line(capsys):
    from utmos_amd import select
    args = select.parse_args(["x.npz"])
    assert args.min_af is None and args.keep_variants is None and args.max_carriers is None
    assert "min_af" not in capsys.readouterr().err
    select.parse_args(["--min-carriers", "2", "x.npz"])
    assert '"min_carriers": 2' in capsys.readouterr().err


def test_filters_are_refused_while_a_store_is_being_written(capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as err:
        select.parse_args(["--lowmem", "new.utm", "--min-af", "0.1", "x.npz"])
    assert err.value.code == 1 and "filter -o" in capsys.readouterr().err
