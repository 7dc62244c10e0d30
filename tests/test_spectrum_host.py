"""Carrier counts without a GPU: the CPU build of k_carrier_counts' word arithmetic (utm_carrier_counts_host) against the
numpy restatement by definition (tests/spectrum_ref.py), the refusals of the ABI, utmos_amd/spectrum.py's closed-form
random-panel curve against exact rationals and against all orders of a small matrix, its classes, its TSV writers and the
command line's refusals."""
import ctypes
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle_util as ou
import order_ref
import spectrum_ref
from oracle_util import npo

EINVAL = -1
B = 16                                        # UTM_SPEC_B: columns per carry-save block
N_SAMP = 270
LISTS = (0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 255, 256, 257)   # plane counts 4 | 8 | 12 are crossed at 16 and 256
SENTINEL = 77


def host_counts(cols, indices, n_var, given=(), want_hist=True, want_count=True):
    """(hist, count) of one chunk by the CPU build; prefilled so that a value that is not written shows."""
    from utmos_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    idx, panel = np.ascontiguousarray(indices, dtype=np.uint32), np.ascontiguousarray(given, dtype=np.uint32)
    hist = np.full(len(idx) + 1, SENTINEL, np.int64) if want_hist else None
    count = np.full(n_var, SENTINEL, np.int32) if want_count else None
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and len(a) else None
    nat.check(nat.lib().utm_carrier_counts_host(cols.ctypes.data_as(ctypes.c_void_p), cols.shape[1], n_var, cols.shape[0], p(idx), len(idx),
                                                p(panel), len(panel), p(hist), p(count)))
    return hist, count


@functools.lru_cache(maxsize=None)
def filled(n_var, fill):
    rng = np.random.default_rng(n_var + len(fill))
    dense = ou.random_dense(rng, n_var, N_SAMP) if fill == "sparse" else ou.random_dense(rng, n_var, N_SAMP, density=0.9, sfs=False)
    dense[[0, n_var // 2, n_var - 1]] = True                             # carried by everybody: bin n is hit
    cols = npo.pack_columns(dense)
    cols.setflags(write=False)
    return cols


# ----------------------------------------------------------------- the CPU build against the restatement
@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("n_var", [1, 63, 64, 65, 8191, 8192, 8193])
def test_cpu_build_equals_the_restatement(n_var, fill):
    cols = filled(n_var, fill)
    rng = np.random.default_rng(n_var + 3 * len(fill))
    for n in LISTS:
        order = rng.permutation(N_SAMP)                                  # (not in index order)
        indices = order[:n]
        for given in (order[:0], order[N_SAMP - 5:], np.concatenate([order[N_SAMP - 2:], order[:1]])):   # none, apart, one in both
            if n == 0 and len(given) == 3:
                given = given[:2]
            hist, count = host_counts(cols, indices, n_var, given)
            want_hist, want_count = spectrum_ref.carrier_counts(cols, indices, n_var, given)
            assert hist.dtype == np.int64 and hist.shape == (n + 1,) and (hist == want_hist).all(), (n, len(given))
            assert (count == want_count).all(), (n, len(given))
            assert hist.sum() == n_var - (want_count < 0).sum()
            if len(given) == 0 and n:
                assert hist[n] >= 1                                      # the rows everybody carries
            if len(given) == 0:
                assert (count >= 0).all()
    only_hist = host_counts(cols, order[:40], n_var, order[50:53], want_count=False)[0]
    only_count = host_counts(cols, order[:40], n_var, order[50:53], want_hist=False)[1]
    both = host_counts(cols, order[:40], n_var, order[50:53])
    assert (only_hist == both[0]).all() and (only_count == both[1]).all()


def test_the_wider_plane_counts_are_crossed_too():
    """4,096 and 65,536 listed samples: where the instantiations go from 12 to 16 and from 16 to 20 planes."""
    n_var, n_samp = 65, 65540
    rng = np.random.default_rng(11)
    dense = rng.random((n_var, n_samp)) < rng.random(n_var)[:, None]
    dense[[0, 64]] = True
    cols = npo.pack_columns(dense)
    order = rng.permutation(n_samp)
    for n in (4095, 4096, 4097, 65535, 65536, 65537):
        for given in (order[:0], order[n:n + 2]):
            hist, count = host_counts(cols, order[:n], n_var, given)
            want_hist, want_count = spectrum_ref.carrier_counts(cols, order[:n], n_var, given)
            assert (hist == want_hist).all() and (count == want_count).all(), n
            assert hist[n] == (0 if len(given) else 2)                   # the rows everybody carries are masked by any panel


def test_the_hand_case():
    dense = np.zeros((6, 3), bool)                                       # A = {1,2,3,4}, B = {1,2,5}, C = {3,4,6}
    dense[[0, 1, 2, 3], 0] = True
    dense[[0, 1, 4], 1] = True
    dense[[2, 3, 5], 2] = True
    cols = npo.pack_columns(dense)
    hist, count = host_counts(cols, [0, 1, 2], 6)
    assert hist.tolist() == [0, 2, 4, 0] and count.tolist() == [2, 2, 2, 2, 1, 1]
    hist, count = host_counts(cols, [2, 0], 6, given=[1])
    assert hist.tolist() == [0, 1, 2] and count.tolist() == [-1, -1, 2, 2, -1, 1]
    hist, count = host_counts(cols, [], 6, given=[1])
    assert hist.tolist() == [3] and count.tolist() == [-1, -1, 0, 0, -1, 0]
    hist, count = host_counts(cols, [], 6)
    assert hist.tolist() == [6] and count.tolist() == [0] * 6
    hist, count = host_counts(cols, [1], 6, given=[1])                   # a sample in both lists contributes nothing
    assert hist.tolist() == [3, 0] and count.tolist() == [-1, -1, 0, 0, -1, 0]


def test_padding_bits_of_the_last_word_are_not_counted():
    cols = np.zeros((3, 2), np.uint64)
    cols[0, 0] = 0b0011
    cols[1, 0] = 0b0110
    cols[2, 1] = np.uint64(1) << np.uint64(2)                            # variant 66 of 67
    hist, count = host_counts(cols, [0, 1, 2], 67)
    assert hist.tolist() == [63, 3, 1, 0] and count[:3].tolist() == [1, 2, 1] and count[66] == 1
    hist, _ = host_counts(cols, [0, 1], 67, given=[2])
    assert hist.tolist() == [63, 2, 1]


# ----------------------------------------------------------------- refusals of the ABI
def test_cpu_build_refuses_bad_arguments_and_leaves_the_outputs():
    from utmos_amd import _native as nat
    lib = nat.lib()
    cols = np.zeros((4, 1), np.uint64)
    hist, count = np.full(3, 5, np.int64), np.full(10, 5, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    u32 = lambda a: None if a is None else np.asarray(a, np.uint32)

    def call(idx, n, given=None, n_given=0, h=hist, c=count, n_var=10, n_samp=4):
        return lib.utm_carrier_counts_host(p(cols), 1, n_var, n_samp, p(u32(idx)), n, p(u32(given)), n_given, p(h), p(c))

    assert call(None, 2) == EINVAL                                       # NULL list with a nonzero length
    assert call([0, 1], 2, None, 1) == EINVAL                            # ... the given list
    assert call([0, 1], 2, h=None, c=None) == EINVAL                     # both outputs NULL
    assert call([0, 4], 2) == EINVAL and b"not in" in lib.utm_last_error()
    assert call([0, 1], 2, [4], 1) == EINVAL and b"given" in lib.utm_last_error()
    assert call([1, 1], 2) == EINVAL and b"twice" in lib.utm_last_error()
    assert call([0, 1], 2, [2, 2], 2) == EINVAL and b"twice" in lib.utm_last_error()
    assert call([0, 1], 2, n_var=65) == EINVAL                           # more variants than words
    assert call([0, 1, 2, 3, 0], 5) == EINVAL                            # more listed than samples
    big = np.zeros(1 << 20, np.uint32)
    assert call(big, 1 << 20, n_samp=1 << 20) == EINVAL and b"counter" in lib.utm_last_error()   # above 2^20 - 1
    assert (hist == 5).all() and (count == 5).all()
    assert call([2, 0], 2) == 0 and hist.tolist() == [10, 0, 0] and (count == 0).all()          # an empty matrix
    assert lib.utm_carrier_counts(None, 0, None, 0, None, 0, 0, p(hist), None, None) == EINVAL and b"ctx" in lib.utm_last_error()


# ----------------------------------------------------------------- the closed-form curve
def exact_curve(hist):
    """E[0..n] as exact rationals from the binomial coefficients."""
    n = len(hist) - 1
    return [sum(int(hist[c]) * (1 - Fraction(math.comb(n - c, k), math.comb(n, k))) for c in range(1, n + 1)) for k in range(n + 1)]


def assert_within(curve, exact, n):
    """Relative error at most 4 n 2^-53: at most 2 k roundings per ratio r_c(k), whose effect on 1 - r_c(k) is at most
    r / (1 - r) <= n / k times larger, plus an n-term sum of non-negative terms."""
    bound = Fraction(4 * n, 1 << 53)
    worst = 0.0
    for k, (got, want) in enumerate(zip(curve, exact)):
        err = abs(Fraction(float(got)) - want)
        assert err <= bound * want, (n, k, float(got), float(want))
        if want:
            worst = max(worst, float(err / want))
    print(f"n = {n}: worst relative error {worst:.3g}, bound {float(bound):.3g}")


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_expected_curve_against_exact_rationals(n):
    from utmos_amd.spectrum import expected_curve
    rng = np.random.default_rng(n)
    for hist in (rng.integers(0, 1000, size=n + 1), (1e6 / np.arange(1, n + 2)).astype(np.int64), np.eye(n + 1, dtype=np.int64)[n] * 12345):
        curve = expected_curve(hist)
        assert curve.dtype == np.float64 and curve.shape == (n + 1,) and curve[0] == 0.0
        assert_within(curve, exact_curve(hist), n)
        assert curve[n] == hist[1:].sum() and (np.diff(curve) >= 0).all()


def test_expected_curve_is_the_mean_over_all_orders():
    from utmos_amd.spectrum import expected_curve
    n_var, n = 40, 6
    dense = ou.random_dense(np.random.default_rng(6), n_var, n, density=0.3, sfs=False)
    cols = npo.pack_columns(dense)
    hist, _ = spectrum_ref.carrier_counts(cols, range(n), n_var)
    total = np.zeros(n + 1, dtype=np.int64)
    orders = list(itertools.permutations(range(n)))
    assert len(orders) == 720
    for order in orders:
        total[1:] += np.cumsum(order_ref.order_curve(cols, order)[0])
    assert_within(expected_curve(hist), [Fraction(int(t), 720) for t in total], n)


def test_expected_curve_of_degenerate_histograms():
    from utmos_amd.spectrum import expected_curve
    assert expected_curve([9]).tolist() == [0.0]                         # no samples listed
    assert expected_curve([4, 0, 0]).tolist() == [0.0, 0.0, 0.0]         # nothing carried
    assert expected_curve([0, 0, 5]).tolist() == [0.0, 5.0, 5.0]         # core variants: any one sample has them
    assert expected_curve([1, 6, 0]).tolist() == [0.0, 3.0, 6.0]         # private variants: linear
    with pytest.raises(ValueError):
        expected_curve([])


def test_classes_of_a_hand_made_histogram():
    from utmos_amd.spectrum import classes
    hist = np.zeros(21, np.int64)
    hist[[0, 1, 2, 18, 19, 20]] = [7, 5, 3, 2, 4, 6]
    assert classes(hist, 0.95) == {"private": 5, "core": 6, "soft_core": 10, "absent": 7, "total": 27}   # ceil(19.0) = 19
    assert classes(hist, 0.9)["soft_core"] == 12 and classes(hist, 0.91)["soft_core"] == 10             # 18 | ceil(18.2) = 19
    assert classes(hist, 1.0)["soft_core"] == 6 and classes(hist, 0.0)["soft_core"] == 20               # never the absent ones
    assert classes([4], 0.95) == {"private": 0, "core": 0, "soft_core": 0, "absent": 4, "total": 4}
    assert classes([1, 2], 0.95) == {"private": 2, "core": 2, "soft_core": 2, "absent": 1, "total": 3}
    with pytest.raises(ValueError):
        classes(hist, 1.5)


# ----------------------------------------------------------------- the TSVs
def test_the_tsv_of_the_histogram(tmp_path):
    from utmos_amd import spectrum
    path = tmp_path / "s.tsv"
    with open(path, "w") as fout:
        spectrum.write_spectrum(fout, np.array([1, 6, 0]))
    assert open(path).read() == "carriers\tvariants\tpct\n0\t1\t0.1429\n1\t6\t0.8571\n2\t0\t0.0\n"
    with open(path, "w") as fout:
        spectrum.write_spectrum(fout, np.array([0, 0]))
    assert open(path).read() == "carriers\tvariants\tpct\n0\t0\t0.0\n1\t0\t0.0\n"        # an empty total: 0, not a division by zero


def test_the_tsv_of_the_curve(tmp_path):
    from utmos_amd import spectrum
    path = tmp_path / "c.tsv"
    with open(path, "w") as fout:
        spectrum.write_curve(fout, np.array([1, 6, 0]))
    assert open(path).read() == "k\texpected_captured\texpected_new\tpct_captured\n1\t3.00\t3.00\t0.4286\n2\t6.00\t3.00\t0.8571\n"
    with open(path, "w") as fout:
        spectrum.write_curve(fout, np.array([3, 1, 1, 1]))               # E = 0, 2, 8/3, 3
    assert open(path).read() == ("k\texpected_captured\texpected_new\tpct_captured\n1\t2.00\t2.00\t0.3333\n2\t2.67\t0.67\t0.4444\n"
                                 "3\t3.00\t0.33\t0.5\n")
    with open(path, "w") as fout:
        spectrum.write_curve(fout, np.array([0, 0]))
    assert open(path).read() == "k\texpected_captured\texpected_new\tpct_captured\n1\t0.00\t0.00\t0.0\n"


# ----------------------------------------------------------------- command line
def test_the_command_is_listed():
    from utmos_amd import __main__ as cli
    assert "spectrum" in cli.COMMANDS and "  spectrum " in cli._usage()


def test_several_processes_are_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import select, spectrum
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        spectrum.spectrum_main(["does_not_exist.npz"])
    assert err.value.code == 1 and "single process" in capsys.readouterr().err


def test_af_is_refused_before_loading(monkeypatch, capsys):
    from utmos_amd import select, spectrum
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        spectrum.spectrum_main(["--af", "does_not_exist.npz"])
    assert err.value.code == 1 and "--af" in capsys.readouterr().err


def test_unusable_inputs_and_options_are_refused(monkeypatch):
    from utmos_amd import spectrum
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv in ([], ["does_not_exist.npz"], ["a.utm", "b.npz"], ["a.hdf5", "b.npz"], ["--quorum", "1.5", "x.npz"]):
        with pytest.raises(SystemExit) as err:
            spectrum.parse_args(argv)
        assert err.value.code == 1, argv
