"""The knob table stays complete (no GPU): every knob of g_knobs (utmos_amd/csrc/utmos_hip.hip) is documented in the
Environment list of include/utmos_hip.h with the same default and range, and is swept by tests/test_gpu_knobs.py or named
there as covered elsewhere.  A knob added without a test fails here."""
import os
import re

import knob_defs
import test_gpu_knobs as tk


def test_every_knob_is_documented_with_its_default_and_range():
    knobs = knob_defs.knobs()
    assert len(knobs) >= 40
    doc = knob_defs.header_entries()
    for name, k in knobs.items():
        assert name in doc, f"{name} is not in the Environment list of include/utmos_hip.h"
        assert doc[name] == (knob_defs.fmt(k["default"]), knob_defs.range_text(k)), name
        assert knob_defs.legal(k, k["default"]), name
    assert set(doc) <= set(knobs), set(doc) - set(knobs)


def test_every_knob_is_swept_or_covered_elsewhere():
    knobs = set(knob_defs.knobs())
    swept, elsewhere = set(tk.SWEEP), set(tk.COVERED_ELSEWHERE)
    assert not swept & elsewhere
    assert knobs == swept | elsewhere, (knobs - swept - elsewhere, (swept | elsewhere) - knobs)
    for knob, row in tk.SWEEP.items():
        assert row["cases"], knob
        assert set(row.get("env", {})) <= knobs, knob
    for env, cases, _ in tk.COMBOS:
        assert set(env) <= knobs and cases, env


def test_the_tests_named_for_the_other_knobs_exist():
    root = knob_defs.ROOT
    for knob, test_id in tk.COVERED_ELSEWHERE.items():
        path, name = test_id.split("::")
        src = open(os.path.join(root, path)).read()
        assert re.search(r"^def %s\(" % re.escape(name), src, re.M), test_id
        assert knob in src, f"{test_id} does not set {knob}"


def test_sweep_values_span_each_range():
    """Each swept knob takes its default, both ends of its range and a value in between, plus one illegal value."""
    knobs = knob_defs.knobs()
    for knob, row in tk.SWEEP.items():
        k = knobs[knob]
        legal, bad = knob_defs.sweep_values(k)
        values = row.get("values") or legal + [bad]
        num = [type(k["default"])(float(v)) for v in values]
        assert k["default"] in num and k["lo"] in num and k["hi"] in num, knob
        assert any(not knob_defs.legal(k, v) for v in num), knob
