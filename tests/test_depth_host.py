"""Coverage depth without a GPU: the CPU build of k_depth_apply's word arithmetic against numpy, the restatement
(tests/depth_ref.py) at M = 1 against the recorded traces of the reference's own code, and the command line's
argument handling."""
import ctypes

import numpy as np
import pytest

import depth_ref
import oracle_util as ou
import order_ref
from oracle_util import npo

DEPTHS = [1, 2, 3, 4, 7, 8, 255]


def bit_length(m):
    return int(m).bit_length()


def planes_of(support, m, wp):
    """uint8 support per variant -> planes[p * wp + w] (bit p of every variant's support) and covered = (support == m)."""
    planes = np.zeros(bit_length(m) * wp, np.uint64)
    for p in range(bit_length(m)):
        planes[p * wp:(p + 1) * wp] = np.packbits((support >> p) & 1, bitorder="little").view(np.uint64)
    return planes, np.packbits(support == m, bitorder="little").view(np.uint64).copy()


def support_of(planes, m, wp):
    out = np.zeros(wp * 64, np.int64)
    for p in range(bit_length(m)):
        out |= np.unpackbits(planes[p * wp:(p + 1) * wp].view(np.uint8), bitorder="little").astype(np.int64) << p
    return out


def apply_host(col, covered, planes, m):
    from utmos_amd import _native as nat
    units, newly = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = nat.lib().utm_depth_apply_host(col.ctypes.data, len(col), covered.ctypes.data, planes.ctypes.data, m,
                                        ctypes.byref(units), ctypes.byref(newly))
    assert rc == 0, nat.lib().utm_last_error()
    return units.value, newly.value


@pytest.mark.parametrize("m", DEPTHS)
def test_word_arithmetic_equals_numpy_on_seeded_planes(m):
    rng = np.random.default_rng(100 + m)
    wp = 37
    # every support from 0 to m occurs, saturated variants (whole words of them too) included
    support = rng.integers(0, m + 1, size=wp * 64).astype(np.uint8)
    support[:128] = m
    support[128:192] = 0
    support[rng.random(wp * 64) < 0.3] = m
    planes, covered = planes_of(support, m, wp)
    want = support.astype(np.int64)
    for _ in range(6):
        col = rng.integers(0, 2 ** 63, size=wp, dtype=np.uint64) | (rng.integers(0, 2, size=wp, dtype=np.uint64) << np.uint64(63))
        col[3] = 0
        col[4] = ~np.uint64(0)
        bits = np.unpackbits(col.view(np.uint8), bitorder="little").astype(np.int64)
        add = bits * (want < m)
        after = want + add
        units, newly = apply_host(col, covered, planes, m)
        assert units == int(add.sum()) and newly == int(((after == m) & (want < m)).sum())
        want = after
        assert (support_of(planes, m, wp) == want).all() and want.max() <= m
        assert (covered == np.packbits(want == m, bitorder="little").view(np.uint64)).all()


@pytest.mark.parametrize("m", DEPTHS)
def test_a_column_added_more_than_m_times_saturates(m):
    wp = 5
    rng = np.random.default_rng(m)
    col = rng.integers(0, 2 ** 62, size=wp, dtype=np.uint64)
    bits = np.unpackbits(col.view(np.uint8), bitorder="little").astype(np.int64)
    planes, covered = np.zeros(bit_length(m) * wp, np.uint64), np.zeros(wp, np.uint64)
    for i in range(m + 3):
        units, newly = apply_host(col, covered, planes, m)
        assert units == (int(bits.sum()) if i < m else 0)
        assert newly == (int(bits.sum()) if i == m - 1 else 0)
    assert (support_of(planes, m, wp) == bits * m).all() and (covered == col).all()


def test_bad_arguments_of_the_host_build():
    from utmos_amd import _native as nat
    a = np.zeros(4, np.uint64)
    u = ctypes.c_uint64(0)
    lib = nat.lib()
    assert lib.utm_depth_apply_host(None, 4, a.ctypes.data, a.ctypes.data, 1, ctypes.byref(u), ctypes.byref(u)) == -1
    for m in (0, 256, -1):
        assert lib.utm_depth_apply_host(a.ctypes.data, 4, a.ctypes.data, a.ctypes.data, m, ctypes.byref(u), ctypes.byref(u)) == -1
    assert lib.utm_set_depth(None, 2) == -1 and lib.utm_get_support(None, 0, None) == -1


# ----------------------------------------------------------------- the restatement at M = 1 is the reference
def trace_setup(t):
    kw = ou.trace_options(t)
    matrix, var_count, samples = npo.build_matrix(t["part_list"], af=bool(kw.get("af")), af_dtype=kw.get("af_dtype") or "f64")
    state = np.array(t["state"], dtype=np.uint8) if "state" in t else npo.initial_state(samples, kw.get("subset"), kw.get("exclude"))
    w = np.array([float.fromhex(x) for x in t["weight_vector_hex"]]) if "weight_vector_hex" in t \
        else npo.weight_vector(samples, kw.get("weights"))
    return matrix, var_count, samples, state, w, npo.resolve_count(len(samples), kw.get("count", 0.02))


TRACES = ["ties_int", "ties_af", "tiny_all", "tiny_all_af", "initial_used_int", "initial_used_af32", "initial_used_af64",
          "initial_used_af64_weights", "weights_signed_int", "weights_signed_af", "weights_all_negative",
          "weights_all_negative_with_masked", "all_excluded", "zero_score_stop", "af_zero_rows", "af_zero_rows_f32",
          "af_zero_rows_int", "subset_exclude_af_weights", "mid_int", "mid_af", "mid_af32_c300"]


@pytest.mark.parametrize("name", TRACES)
def test_restatement_at_depth_1_reproduces_the_reference_trace(name):
    t = ou.load_trace(name)
    matrix, var_count, samples, state, w, k = trace_setup(t)
    if name.startswith("mid"):
        k = min(k, 40)                                             # (the first rows of the long ones)
    if "scores_hex" in t:                                          # the whole vector handed to argmax, every iteration
        probe = state.copy()
        for it, vec in enumerate(t["scores_hex"][:k]):
            best, _, scores = depth_ref.calculate_scores(matrix, probe, w, 1)
            assert [float(x + 0.0).hex() for x in scores] == [float(float.fromhex(x) + 0.0).hex() for x in vec], it
            if best is None:
                break
            probe[best] = 0
    rows = depth_ref.greedy(matrix, state, k, w, 1)
    want = [ln.split("\t") for ln in t["tsv"].splitlines()[1:]][:k]
    assert [r[0] for r in rows] == t["idx"][:k]
    assert [r[1] for r in rows] == [int(r[2]) for r in want]
    assert [float(r[2]).hex() for r in rows] == t["score_hex"][:k]
    assert depth_ref.tsv(rows, samples, var_count, matrix.shape[0], 1) == "\n".join(t["tsv"].split("\n")[:len(rows) + 1]) + "\n"
    # at M = 1 the sixth figure is tot_captured plus what the initially used samples cover
    assert all(r[3] >= int(ln[3]) for r, ln in zip(rows, want))


@pytest.mark.parametrize("name", order_ref.case_names())
def test_fixed_order_restatement_at_depth_1_reproduces_the_recorded_orders(name):
    t = order_ref.load_case(name)
    matrix, var_count, samples = npo.build_matrix(t["part_list"], af=t["af"], af_dtype=t["af_dtype"] or "f64")
    state = npo.initial_state(samples, ou.read_list(ou.os.path.join(ou.GOLD, t["subset"])) if t["subset"] else None, t["exclude"])
    w = npo.weight_vector(samples, ou.read_weights(ou.os.path.join(ou.GOLD, t["weights"])) if t["weights"] else None)
    rows = depth_ref.fixed_order(matrix, state, t["order"], 1)
    assert [r[1] for r in rows] == t["gains"]
    total = sum(t["gains"])
    if t["cont_idx"]:
        cont = depth_ref.greedy(matrix, state, len(t["cont_idx"]), w, 1)
        assert [r[0] for r in cont] == t["cont_idx"] and [r[1] for r in cont] == t["cont_gains"]
        text = depth_ref.tsv(rows, t["samples"], var_count, t["n_var"], 1) + depth_ref.tsv(cont, t["samples"], var_count, t["n_var"], 1, total, header=False)
        assert text == order_ref.case_tsv(t)


def test_depth_2_on_a_hand_made_matrix():
    # variants x samples; sample 0 and 1 are twins, variant 3 has one carrier only
    dense = np.array([[1, 1, 0, 0],
                      [1, 1, 1, 0],
                      [0, 0, 1, 1],
                      [0, 0, 0, 1]], dtype=bool)
    rows = depth_ref.greedy(dense, np.ones(4, np.uint8), 4, None, 2)
    # 0 (2 units), then its twin 1 (2 more: variants 0 and 1 are saturated); sample 3 is now worth 2 (variants 2, 3)
    # against sample 2's 1 (variant 1 counts no more); sample 2 brings variant 2 to depth; variant 3 stays at 1
    assert [(r[0], r[1], r[3]) for r in rows] == [(0, 2, 0), (1, 2, 2), (3, 2, 2), (2, 1, 3)]
    packed, support = depth_ref.packed_greedy(npo.pack_columns(dense), 4, np.ones(4, np.uint8), 4, 2)
    assert packed == [(r[0], r[1], r[3]) for r in rows] and support.tolist() == [2, 2, 2, 1]


# ----------------------------------------------------------------- command line
@pytest.mark.parametrize("value", ["0", "256", "-3"])
def test_depth_out_of_range_exits_1(value, capsys):
    from utmos_amd import select
    with pytest.raises(SystemExit) as e:
        select.parse_args(["--depth", value, "x.npz"])             # (parse_args sets the logging up itself: stderr)
    assert e.value.code == 1 and "--depth must be between 1 and 255" in capsys.readouterr().err


def test_depth_with_several_processes_exits_1(monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        select.select_main(["--depth", "2", "x.npz"])
    assert e.value.code == 1 and "--depth above 1 needs the whole sample axis on one GPU" in capsys.readouterr().err


def test_depth_defaults_to_1_and_headers():
    from utmos_amd import select
    assert select.parse_args(["x.npz"]).depth == 1 and select.parse_args(["--depth", "3", "x.npz"]).depth == 3
    assert select.HEADER == depth_ref.HEADER and select.HEADER_DEPTH == depth_ref.HEADER_DEPTH
    assert select.HEADER_DEPTH.rstrip("\n").split("\t")[:5] == select.HEADER.rstrip("\n").split("\t")
    assert select.HEADER_DEPTH.rstrip("\n").split("\t")[5] == "at_depth"


def test_run_selection_refuses_a_depth_out_of_range():
    from utmos_amd import select

    class ShapeOnly:
        shape = (10, 4)

    data = {"data": ShapeOnly(), "samples": np.array(["A", "B", "C", "D"]), "var_count": np.zeros(4, np.int64)}
    for bad in (0, 256):
        with pytest.raises(ValueError, match="depth"):
            select.run_selection(data, 2, depth=bad)
