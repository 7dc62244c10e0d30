"""Every environment knob against the sequential float64 C oracle (include/utmos_hip.h: "None of these changes a
result").  SWEEP maps a knob to the cases it runs on; each knob takes its default, both ends of its legal range, one value
in between and one illegal value (knob_defs.sweep_values, from g_knobs), and every run must give the oracle's sample
order, new_count and float64 scores bit for bit.  An illegal value must also take the default's path.  COMBOS pin the
settings that reach code the defaults never run (k_score_afs<32, 8>, launch_score_int<4>, non-temporal loads on small
matrices, the stand-alone k_pick, k_cand + chains + a separate pick, ...).  Knobs are read at context creation, so
each run sets them before its DeviceMatrix is made.  test_knob_table.py (CPU) keeps SWEEP complete."""
import numpy as np
import pytest

import knob_defs
import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

# ----------------------------------------------------------------- the table
# knob -> {"cases": [...], "env": {other knobs for the whole sweep}, "values": [...] (default: knob_defs.sweep_values)}
_LAUNCH = {"UTM_PERSISTENT": "0"}            # (knobs of the per-iteration launches: keep the persistent loop out)
SWEEP = {
    "UTM_TARGET_WGS": {"cases": ["int", "af32"], "env": _LAUNCH},
    "UTM_MIN_WGS": {"cases": ["int", "af32"], "env": _LAUNCH},
    "UTM_MIN_WGS_BIG": {"cases": ["int", "af32"], "env": dict(_LAUNCH, UTM_AF_STEPS="32")},
    "UTM_TILE_STEPS": {"cases": ["int", "int_chunks"], "env": _LAUNCH},
    "UTM_NT_LOADS": {"cases": ["int", "af32"]},
    "UTM_NT_MIN_MB": {"cases": ["int"], "env": _LAUNCH},
    "UTM_SCORE_FORM": {"cases": ["int"], "env": dict(_LAUNCH, UTM_TILE_STEPS="16")},
    "UTM_FUSE_PICK": {"cases": ["int", "int_chunks"]},
    "UTM_PICK_THREADS": {"cases": ["wide"], "env": {"UTM_FUSE_PICK": "0"}, "values": ["0", "64", "512", "1024", "100", "2048"]},
    "UTM_BATCH": {"cases": ["int", "af32", "af64"], "values": ["0", "1", "3", "255", "257", "65536", "-1"]},
    "UTM_AF_STEPS": {"cases": ["af32", "af64"], "env": {"UTM_AF_SWITCH": "0", "UTM_MIN_WGS_BIG": "1"}},
    "UTM_AF_TARGET_WGS": {"cases": ["af32"]},
    "UTM_AF_TABLE_RUN": {"cases": ["af32"]},
    "UTM_AF_TABLE_WGS_PER_CU": {"cases": ["af32"]},
    "UTM_AF_TABLES": {"cases": ["af32", "af64"]},
    "UTM_CHAIN_PICK": {"cases": ["af64"]},
    "UTM_AF_VERIFY": {"cases": ["af64"]},
    "UTM_AF_RECORD": {"cases": ["af64"]},
    "UTM_AF_DEFER": {"cases": ["af64"]},
    "UTM_AF_SWITCH": {"cases": ["af32", "af64"]},
    "UTM_AF_DENSE_DELTA": {"cases": ["af32", "af64"]},
    "UTM_DECR_FIRST_BATCH": {"cases": ["int_decr"], "values": ["8", "1", "100", "65536", "32768", "0"]},
    "UTM_DECR_INTERLEAVED": {"cases": ["int_decr"]},
    "UTM_PERSISTENT": {"cases": ["int", "af32"]},
    "UTM_PERSIST_MAX_MB": {"cases": ["int"], "values": ["560", "0", "1", "16777216", "8388608", "-1"]},
    "UTM_PERSIST_WGS_PER_CU": {"cases": ["int"], "values": ["0", "1", "16", "8", "17"]},
    "UTM_PERSIST_MAX_TILES": {"cases": ["int"]},
    "UTM_PERSIST_TILE_KIB": {"cases": ["int", "af32"]},
    "UTM_PERSIST_TALL_MAX_SAMPLES": {"cases": ["int"], "env": {"UTM_PERSIST_MAX_TILES": "5"}},
    "UTM_PERSIST_MAX_SAMPLES": {"cases": ["int", "wide"]},
    "UTM_PERSIST_AF": {"cases": ["af32", "af64"]},
    "UTM_PERSIST_AF_MAX_TILES": {"cases": ["af32"]},
    "UTM_PERSIST_SPEC_TICKS": {"cases": ["af64"]},
    "UTM_PERSIST_CHAINERS": {"cases": ["af64"]},
    "UTM_PERSIST_AF_INTERVAL": {"cases": ["af64"]},
    "UTM_PERSIST_CLAIMS": {"cases": ["claims"]},
    "UTM_PERSIST_AHEAD_TICKS": {"cases": ["claims"]},
    "UTM_PERSIST_AHEAD0_TICKS": {"cases": ["claims"], "values": ["0", "50", "1073741824", "536870912", "-1"]},
}
# knobs whose paths need several processes or are test hooks that end a run on purpose: the tests that cover them
COVERED_ELSEWHERE = {
    "UTM_MBOX_SPINS_LOG2": "tests/test_gpu_errors.py::test_a_shard_that_never_posts_ends_the_loop_with_ecomm_and_the_context_recovers",
    "UTM_P2P_REPLICATE": "tests/test_gpu_parity.py::test_fused_device_side_exchange_three_processes",
    "UTM_TEST_REMOTE_WINNER": "tests/test_gpu_parity.py::test_rccl_exchange_single_rank",
    "UTM_TEST_MUTE_EXCHANGE": "tests/test_gpu_errors.py::test_a_shard_that_never_posts_ends_the_loop_with_ecomm_and_the_context_recovers",
    "UTM_TEST_DROP_ARRIVAL": "tests/test_gpu_persistent.py::test_withheld_partial_count_ends_in_an_error_and_the_context_recovers",
}

# (environment, cases, what the stats must show): settings that reach code the defaults never run
COMBOS = (
    # integer launches at every tile size and both 32 / 16 KiB forms, cached and non-temporal loads
    [({"UTM_PERSISTENT": "0", "UTM_TILE_STEPS": str(s), "UTM_SCORE_FORM": str(f), "UTM_NT_LOADS": str(nt)}, ["int"], "launches")
     for s in (2, 4, 8, 16, 32) for f in (0, 1) for nt in (0, 1)]
    # k_score_afs<32, 8> from the first pass on
    + [({"UTM_AF_STEPS": "32", "UTM_AF_SWITCH": "0", "UTM_MIN_WGS_BIG": "1"}, ["af32", "af64"], None)]
    # k_cand, then chains, then a separate pick; no sums on record; chained on the spot
    + [({k: "0"}, ["af64"], "chained") for k in ("UTM_CHAIN_PICK", "UTM_AF_VERIFY", "UTM_AF_RECORD", "UTM_AF_DEFER")]
    + [({"UTM_CHAIN_PICK": "0", "UTM_AF_VERIFY": "0", "UTM_AF_RECORD": "0", "UTM_AF_DEFER": "0"}, ["af64", "af64_chunks"], "chained")]
    + [({"UTM_AF_SWITCH": "0", "UTM_AF_DENSE_DELTA": "0"}, ["af32", "af64"], None),
       ({"UTM_AF_SWITCH": "1", "UTM_AF_DENSE_DELTA": "1"}, ["af32", "af64"], None)]
    # the stand-alone k_pick for integer runs, weighted and not, over several chunks
    + [({"UTM_FUSE_PICK": "0"}, ["int", "int_w", "int_chunks", "wide"], "launches")]
    # persistent-loop settings
    + [({"UTM_PERSIST_CLAIMS": "0"}, ["claims", "int"], "persistent"),
       ({"UTM_PERSIST_AHEAD_TICKS": "0"}, ["claims"], "persistent"),
       ({"UTM_PERSIST_AHEAD0_TICKS": "300"}, ["claims"], "persistent"),
       ({"UTM_PERSIST_WGS_PER_CU": "1"}, ["int", "int_w", "claims"], "persistent"),
       ({"UTM_PERSIST_MAX_TILES": "1"}, ["int"], "launches"),  # (even the 64 KiB tile cuts a column into 3)
       ({"UTM_PERSIST_MAX_TILES": "5"}, ["int"], "persistent"),  # (the 32 KiB tile: 5 a column)
       ({"UTM_PERSIST_MAX_TILES": "5", "UTM_PERSIST_TALL_MAX_SAMPLES": "0"}, ["int"], "launches"),
       ({"UTM_PERSIST_MAX_MB": "1"}, ["int", "int_w"], "launches")]
    + [({"UTM_BATCH": b}, ["int_w", "af64_chunks"], None) for b in ("1", "3", "255", "257")]
    + [({"UTM_DECR_FIRST_BATCH": b}, ["int_decr", "af32_decr"], "decremental") for b in ("1", "100")]
)


# ----------------------------------------------------------------- cases
def random_cols(rng, n_var, n_samp, ands):
    """Packed columns (S, W) with a carrier density of 2^-ands[s] per sample, the bits behind n_var clear."""
    w = (n_var + 63) // 64
    cols = np.empty((n_samp, w), np.uint64)
    for s in range(n_samp):
        c = rng.integers(0, 2 ** 64 - 1, w, dtype=np.uint64, endpoint=True)
        for _ in range(int(ands[s]) - 1):
            c &= rng.integers(0, 2 ** 64 - 1, w, dtype=np.uint64, endpoint=True)
        cols[s] = c
    if n_var % 64:
        cols[:, -1] &= np.uint64((1 << (n_var % 64)) - 1)
    return cols


def _state(n_samp, excluded, used):
    st = np.ones(n_samp, np.uint8)
    st[excluded] = 2                 # never selected, never cover
    st[used] = 0                     # used from the start: cover from the first iteration
    return st


def _signed_weights(rng, n_samp):
    return rng.choice([-2.0, -0.5, 0.0, 0.25, 1.0, 3.0], n_samp)


_CASES = {}


def case(name):
    """dict(cols, n_var, state, weights, af, chunks, decremental, k); built once per module."""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    c = {"weights": None, "af": None, "chunks": None, "decremental": None, "k": None}
    if name in ("int", "int_w", "int_chunks", "int_decr"):
        # 4 x 64 KiB + a ragged tile at every tile size; 130 samples (neither a multiple of 4 nor of 64)
        n_var, n_samp = 4 * 262_144 + 4_097, 130
        base = case("int")["cols"] if name != "int" else random_cols(rng, n_var, n_samp, rng.integers(3, 9, n_samp))
        c.update(cols=base, n_var=n_var, state=_state(n_samp, [3, 17, 100], [5, 64]))
        if name == "int_w":
            c["weights"] = _signed_weights(rng, n_samp)
        if name == "int_chunks":
            c["chunks"] = [0, 300_032, 700_032, n_var]   # (chunk starts on a word boundary of the packed columns)
        if name == "int_decr":
            c["decremental"] = 0.0
    elif name == "wide":
        # more than 1,024 selectable samples; the first winner (unique) sits at position 1,077: with 100 pick threads it
        # is thread 77's, in the second, partly filled wave
        n_var, n_samp = 40_000 + 17, 1_100
        cols = random_cols(rng, n_var, n_samp, rng.integers(4, 9, n_samp))
        cols[1077] |= random_cols(rng, n_var, 1, [2])[0]
        c.update(cols=cols, n_var=n_var, state=np.ones(n_samp, np.uint8), k=64)
    elif name == "claims":
        # 21 tiles of 8 KiB, 300 samples: with one resident block per CU the waves claim positions beyond their static two
        n_var, n_samp = 20 * 65_536 + 333, 300
        c.update(cols=random_cols(rng, n_var, n_samp, rng.integers(3, 9, n_samp)), n_var=n_var,
                 state=_state(n_samp, [7], [250]), k=48)
    elif name in ("af32", "af32_decr"):
        n_var, n_samp = 3 * 65_536 + 1_001, 130
        base = case("af32")["cols"] if name != "af32" else random_cols(rng, n_var, n_samp, rng.integers(3, 9, n_samp))
        c.update(cols=base, n_var=n_var, state=_state(n_samp, [2, 99], [9]),
                 af=(rng.integers(1, 2 * n_samp, n_var) / (2.0 * n_samp)).astype(np.float32))
        if name == "af32_decr":
            c["decremental"] = 0.0
    elif name in ("af64", "af64_chunks"):
        # every sample has a twin: the estimates tie, float64 chains tell them apart; signed weights and zeros
        n_var, half = 2 * 65_536 + 77, 65
        if name == "af64":
            base = random_cols(rng, n_var, half, rng.integers(4, 10, half))
            perm = rng.permutation(2 * half)
            cols = np.concatenate([base, base])[perm]
            w = np.concatenate([np.full(half, 1.0), np.full(half, 1.0)])[perm]
            w[rng.integers(0, 2 * half, 6)] = 0.0
            w[rng.integers(0, 2 * half, 4)] = -1.0
            af = (rng.integers(1, 12, n_var) / (4.0 * half) / 3.0).astype(np.float64)   # 53-bit mantissas
            c.update(cols=cols, n_var=n_var, state=_state(2 * half, [11], [40]), weights=w, af=af)
        else:
            c.update({k: v for k, v in case("af64").items() if k != "chunks"})
            c["chunks"] = [0, 69_952, n_var]
    else:
        raise KeyError(name)
    c["expected"] = ou.c_greedy(c["cols"], c["n_var"], c["state"], c["weights"], c["af"], k_max=c["k"])
    _CASES[name] = c
    return c


def _slice_cols(cols, lo, hi):
    """Columns of variants [lo, hi) (lo a multiple of 64)."""
    assert lo % 64 == 0
    part = cols[:, lo // 64:(hi + 63) // 64].copy()
    if hi % 64:
        part[:, -1] &= np.uint64((1 << (hi % 64)) - 1)
    return part


@pytest.fixture(scope="module")
def dev():
    from utmos_amd import _native as nat
    assert nat.device_count() >= 1, "no GPU visible"
    from utmos_amd import device
    return device


def run_case(dev, monkeypatch, name, env):
    """One run of a case with `env` set (and every other knob at its default); asserts the oracle's rows; -> stats."""
    for k in knob_defs.knobs():
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = case(name)
    n_samp = c["cols"].shape[0]
    bounds = c["chunks"] or [0, c["n_var"]]
    with dev.DeviceMatrix(n_samp) as m:
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            ch = m.add_chunk(hi - lo)
            m.upload_columns(ch, _slice_cols(c["cols"], lo, hi))
            if c["af"] is not None:
                m.set_af(ch, c["af"][lo:hi])
        m.set_state(c["state"])
        m.set_weights(c["weights"])
        if c["decremental"] is not None:
            m.set_decremental(True, c["decremental"])
        got = m.run(n_samp if c["k"] is None else c["k"])
        st = m.stats()
    exp = c["expected"]
    assert got[0].tolist() == exp[0].tolist(), (name, env)
    assert got[1].tolist() == exp[1].tolist(), (name, env)
    assert got[2].tolist() == exp[2].tolist(), (name, env)      # float64 scores, bit for bit
    return st


def _path(st):
    """What a run's stats say about the path it took (the same for an illegal value as for the default)."""
    return (st["persist_iterations"] > 0, st["af_table_passes"] > 0, st["decr_iterations"] > 0, st["af_deferred_rows"] > 0)


def _sweep_params():
    defs = knob_defs.knobs()
    out = []
    for knob, row in SWEEP.items():
        legal, bad = knob_defs.sweep_values(defs[knob])
        values = row.get("values") or legal + [bad]
        for v in values:
            for name in row["cases"]:
                out.append(pytest.param(knob, v, name, id=f"{knob}={v}-{name}"))
    return out


@pytest.mark.parametrize("knob,value,name", _sweep_params())
def test_knob_value_gives_the_oracles_rows(dev, monkeypatch, knob, value, name):
    k = knob_defs.knobs()[knob]
    env = dict(SWEEP[knob].get("env", {}))
    env[knob] = value
    st = run_case(dev, monkeypatch, name, env)
    v = float(value)
    if not knob_defs.legal(k, type(k["default"])(v)):
        # an illegal value leaves the default in place: the default's path, not just its rows
        base = dict(env)
        base.pop(knob)
        assert _path(st) == _path(run_case(dev, monkeypatch, name, base)), (knob, value, name)
    if name == "af64":
        assert st["af_chained_iterations"] > 0, st                       # the twins need chains
    if knob == "UTM_DECR_FIRST_BATCH" and (int(value) if knob_defs.legal(k, int(value)) else k["default"]) <= 100:
        assert st["decr_iterations"] > 0, st                             # (a first batch that is the whole run leaves none)


@pytest.mark.parametrize("env,name,expect", [pytest.param(e, n, x, id="-".join(f"{k[4:]}={v}" for k, v in e.items()) + "-" + n)
                                             for e, cases, x in COMBOS for n in cases])
def test_combination_gives_the_oracles_rows(dev, monkeypatch, env, name, expect):
    st = run_case(dev, monkeypatch, name, env)
    if expect == "launches":
        assert st["persist_iterations"] == 0, st
    elif expect == "persistent":
        assert st["persist_iterations"] > 0, st
    elif expect == "chained":
        assert st["af_chained_iterations"] > 0, st
        if env.get("UTM_AF_DEFER") == "0":
            assert st["af_deferred_rows"] == 0, st
    elif expect == "decremental":
        assert st["decr_iterations"] > 0, st
    if env.get("UTM_AF_SWITCH") == "0" and name.startswith("af"):
        assert st["af_table_passes"] == 0, st                            # (no dense full pass: the streaming kernel from the first)


def test_pick_threads_not_a_multiple_of_64_keeps_the_winner(dev, monkeypatch):
    """The first winner is unique and sits where thread 77 of a 100-thread pick would scan it (the second wave, partly
    filled).  A thread count that is not a multiple of 64 -- or above 1,024 -- is ignored: the row is the oracle's."""
    c = case("wide")
    assert c["expected"][0][0] == 1077
    scores = ou.c_score(c["cols"], c["n_var"], c["state"])[1]
    assert (scores == scores.max()).sum() == 1
    for value in ("100", "2048", "64"):
        run_case(dev, monkeypatch, "wide", {"UTM_FUSE_PICK": "0", "UTM_PICK_THREADS": value})


def _forced_tile_case():
    """float32 AF, 64 samples x 16.8M variants: 257 tiles of 8 KiB -- more than the AF forms' 8-bit arrival field counts."""
    rng = np.random.default_rng(257)
    n_var, n_samp = 256 * 65_536 + 4_097, 64
    cols = random_cols(rng, n_var, n_samp, rng.integers(5, 9, n_samp))
    af = (rng.integers(1, 2 * n_samp, n_var) / (2.0 * n_samp)).astype(np.float32)
    return cols, n_var, af


def test_forced_tile_beyond_the_arrival_fields_keeps_the_launches(dev, monkeypatch):
    monkeypatch.setenv("UTM_PERSIST_TILE_KIB", "8")
    cols, n_var, af = _forced_tile_case()
    n_samp, k = cols.shape[0], 24
    state = np.ones(n_samp, np.uint8)
    exp = ou.c_greedy(cols, n_var, state, None, af, k_max=k)
    with dev.DeviceMatrix(n_samp) as m:
        ch = m.add_chunk(n_var)
        m.upload_columns(ch, cols)
        m.set_af(ch, af)
        got = m.run(k)
        st = m.stats()
    assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
    assert got[2].tolist() == exp[2].tolist()
    assert st["persist_iterations"] == 0, st


def test_knob_parser_ignores_text_that_is_not_a_number(dev, monkeypatch):
    """Trailing text, a fraction for an integer knob and an empty value: the default holds."""
    base = _path(run_case(dev, monkeypatch, "int", {}))
    for v in ("1x", "0.5", " ", "nan"):
        assert _path(run_case(dev, monkeypatch, "int", {"UTM_PERSISTENT": v})) == base
    assert _path(run_case(dev, monkeypatch, "af32", {"UTM_AF_SWITCH": "nan", "UTM_AF_TABLES": "1e0"})) == \
        _path(run_case(dev, monkeypatch, "af32", {}))
