"""GPU: `select --bound-out` end to end on the committed golden parts.

The panel TSV must be byte-identical with and without the flag, and every column of the bound TSV is held against
tests/bound_ref.py on the matrix rebuilt from the original part files, under the printed order."""
import functools
import os

import numpy as np
import pytest

import bound_ref
import oracle_util as ou
from oracle_util import npo

pytestmark = pytest.mark.gpu

PARTS = ("chunk0", "chunk1", "chunk2")
HEADER = "k\tcaptured\tbound_trivial\tbound_online\tbound_lagrange\tbound\tshare"
ITERS = 40           # (--bound-iters: the restatement runs the same steps in numpy)


def run_select(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def files():
    return [os.path.join(ou.GOLD, name + ".npz") for name in PARTS]


@functools.lru_cache(maxsize=None)
def original():
    matrix, _, samples = npo.build_matrix([ou.load_part(name) for name in PARTS])
    dense = np.asarray(matrix) != 0
    dense.setflags(write=False)
    return dense, [str(s) for s in samples]


def lines_of(path):
    return [line.split("\t") for line in open(path).read().splitlines()]


CASES = {                # name: (flags of the selection, flags of the bound, what the restatement has to know)
    "plain": ([], [], {}),
    "include": (["--include", "SAMPLES 40 7"], [], dict(given=(40, 7))),
    "exclude": (["--exclude", "SAMPLES 3 11 12 50"], [], dict(excluded=(3, 11, 12, 50))),
    "at": ([], ["--bound-at", "3,8"], dict(sizes=(3, 8))),
    "refine": (["--refine", "-1"], [], {}),
    "min-carriers": (["--min-carriers", "2"], [], dict(min_carriers=2)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bound_file_equals_the_restatement_and_the_panel_is_unchanged(name, tmp_path):
    flags, bound_flags, how = CASES[name]
    dense, names = original()
    flags = [",".join(names[int(i)] for i in x.split()[1:]) if x.startswith("SAMPLES") else x for x in flags]
    plain, tsv, out = (str(tmp_path / f) for f in ("plain.tsv", "flag.tsv", "bound.tsv"))
    run_select(["-c", "8", "-o", plain] + flags + files())
    run_select(["-c", "8", "-o", tsv, "--bound-out", out, "--bound-iters", str(ITERS)] + bound_flags + flags + files())
    assert open(tsv).read() == open(plain).read()                        # byte-identical with and without the flag
    rows = lines_of(tsv)[1:]
    order = [names.index(r[0]) for r in rows]
    assert len(order) == 8
    if "min_carriers" in how:
        dense = dense[dense.sum(axis=1) >= how["min_carriers"]]
    given = list(how.get("given", ()))
    cand = [s for s in range(len(names)) if s not in given and s not in how.get("excluded", ())]
    got = lines_of(out)
    assert "\t".join(got[0]) == HEADER
    sizes = how.get("sizes", (8,))
    assert len(got) == 1 + len(sizes)
    for line, size in zip(got[1:], sizes):
        assert line == bound_ref.bound_row(dense, order, size, cand, given, ITERS), size
        assert int(line[1]) == int(rows[size - 1][3])                    # captured = the run's tot_captured at row K
        assert int(line[1]) <= int(line[5]) == min(int(line[2]), int(line[3]), int(line[4]))
        assert 0.0 < float(line[6]) <= 1.0


@pytest.mark.parametrize("extra,word", [(["--af"], "--af"), (["--weights", os.path.join(ou.GOLD, "weights.txt")], "--weights"),
                                        (["--depth", "2"], "--depth"), (["--include", "A,B", "--bound-at", "2"], "--bound-at")])
def test_what_the_bound_does_not_answer_is_refused_with_its_reason(extra, word, tmp_path, capsys):
    out = str(tmp_path / "bound.tsv")
    with pytest.raises(SystemExit) as err:
        run_select(["-c", "8", "-o", os.devnull, "--bound-out", out] + extra + files())
    assert err.value.code == 1 and word in capsys.readouterr().err
    assert not os.path.exists(out)


def test_several_processes_are_refused_before_loading(tmp_path, monkeypatch, capsys):
    from utmos_amd import select
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(select, "load_files", lambda *a, **k: pytest.fail("inputs were loaded"))
    with pytest.raises(SystemExit) as err:
        select.select_main(["--bound-out", str(tmp_path / "b.tsv")] + files())
    assert err.value.code == 1 and "single process" in capsys.readouterr().err
