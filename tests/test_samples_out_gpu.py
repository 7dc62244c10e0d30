"""GPU: `select --samples-out / --represent-out` and `spectrum --by-sample` end to end on the committed golden parts.

The per-sample tables are held against tests/class_ref.py applied to tests/rank_ref.py's ranks of the PRINTED order over
the matrix rebuilt from the original part files, for every way `select` makes its rows; against the loop itself
(utm_step + utm_peek_scores, which share nothing with the new code); and the output without the new flags against the
committed answer keys, byte for byte."""
import functools
import os

import numpy as np
import pytest

import class_ref
import oracle_util as ou
import rank_ref
import spectrum_ref
from oracle_util import npo

pytestmark = pytest.mark.gpu
CASES = ou.golden_cases()


def run_select(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def files_of(parts):
    return [os.path.join(ou.GOLD, name + ".npz") for name in parts]


@functools.lru_cache(maxsize=None)
def original(parts):
    """(dense bool (informative variants, samples), AF per variant, names) from the ORIGINAL part files."""
    loaded = [ou.load_part(name) for name in parts]
    matrix, _, samples = npo.build_matrix(loaded)
    names = [str(s) for s in samples]
    afs = []
    for p in loaded:
        informative = np.unpackbits(p["GT"], axis=1, count=len(names)).astype(bool).any(axis=1)
        afs.append(np.asarray(p["AF"], np.float64).reshape(-1)[informative])
    dense = np.asarray(matrix) != 0
    dense.setflags(write=False)
    return dense, np.concatenate(afs), names


def rows_of(tsv):
    return [line.split("\t") for line in open(tsv).read().splitlines()[1:]]


def expected_table(dense, order, depth):
    """(new, missed, total) by definition: class_ref on rank_ref's ranks of the order."""
    k = len(order)
    cols = npo.pack_columns(dense)
    rank = rank_ref.capture_rank(cols, order, depth, dense.shape[0])
    table = class_ref.class_counts(cols, np.where(rank < 0, k, rank), k + 1, None, dense.shape[0])
    return table[:, :k], table[:, k], table.sum(axis=1)


def represent_restated(names, order, new, total):
    """--represent-out restated: per row, the samples with total > 0 outside rows 0..i and their captured shares."""
    lines, cum = [], np.cumsum(new, axis=1)
    for i in range(len(order)):
        out = [j for j in range(len(names)) if total[j] > 0 and j not in set(order[:i + 1])]
        pct = np.asarray([cum[j, i] / total[j] for j in out])
        if not out:
            lines.append(f"{names[order[i]]}\t0\tnan\tnan\tnan\t.")
            continue
        lines.append("\t".join(str(x) for x in (names[order[i]], len(out), round(float(np.mean(pct)), 4), round(float(np.median(pct)), 4),
                                                 round(float(pct.min()), 4), names[out[int(np.flatnonzero(pct == pct.min())[0])]])))
    return "sample\tn_outside\tmean_pct\tmedian_pct\tmin_pct\tmin_sample\n" + "".join(line + "\n" for line in lines)


SELECTIONS = {
    "greedy": (("chunk0", "chunk1"), ["-c", "30"], 1),
    "greedy-chunks": (("chunk0", "chunk1", "chunk2"), ["-c", "12", "--maxmem", "0", "--buffer", "256"], 1),
    "mid": (("mid",), ["-c", "25"], 1),
    "af": (("chunk0", "chunk1"), ["-c", "20", "--af"], 1),
    "depth2": (("chunk0", "chunk1"), ["-c", "30", "--depth", "2"], 2),
    "include": (("chunk0", "chunk1"), ["-c", "20", "--include", "SAMPLES 900 5"], 1),
    "topN": (("chunk0", "chunk2"), ["-c", "20", "--mode", "topN"], 1),
    "refine": (("chunk0",), ["-c", "8", "--refine", "-1"], 1),
    "min-carriers": (("chunk0", "chunk1"), ["-c", "20", "--min-carriers", "2"], 1),
}


@pytest.mark.parametrize("name", sorted(SELECTIONS))
def test_the_file_equals_the_restatement_under_the_printed_order(name, tmp_path):
    parts, flags, depth = SELECTIONS[name]
    dense, af, names = original(parts)
    flags = [",".join(names[int(i)] for i in x.split()[1:]) if x.startswith("SAMPLES") else x for x in flags]
    plain, tsv, npz, rep = (str(tmp_path / f) for f in ("plain.tsv", "flag.tsv", "samples.npz", "represent.tsv"))
    run_select(flags + ["-o", plain] + files_of(parts))
    run_select(flags + ["-o", tsv, "--samples-out", npz, "--represent-out", rep] + files_of(parts))
    assert open(tsv).read() == open(plain).read()                        # the TSV is byte-identical with and without
    rows = rows_of(tsv)
    assert len(rows) >= 5
    order = [names.index(r[0]) for r in rows]
    if name == "af":
        dense = dense & (af != 0)[:, None]                               # the reference's float matrix holds nothing there
    if name == "min-carriers":
        dense = dense[dense.sum(axis=1) >= 2]
    want_new, want_missed, want_total = expected_table(dense, order, depth)
    with np.load(npz, allow_pickle=False) as z:
        assert sorted(z.files) == ["missed", "new", "panel", "samples", "total"]
        new, missed, total = z["new"], z["missed"], z["total"]
        assert z["samples"].tolist() == names and z["panel"].tolist() == order
    assert new.dtype == missed.dtype == total.dtype == np.int64 and new.shape == (len(names), len(order))
    assert (new == want_new).all() and (missed == want_missed).all() and (total == want_total).all()
    assert (new.sum(axis=1) + missed == total).all()
    if depth == 1:
        for i, member in enumerate(order):
            assert new[member, :i + 1].sum() == total[member]            # a member's own variants are all captured by its row
            assert new[member, i] == int(rows[i][2])                     # ... and what its row captured is the TSV's new_count
    else:
        assert new.sum() > 0 and (total[order] >= missed[order]).all()
    assert open(rep).read() == represent_restated(names, order, new, total)


def test_both_files_in_one_run_share_the_ranks(tmp_path):
    parts = ("chunk0", "chunk1")
    dense, _, names = original(parts)
    tsv, npz, variants = (str(tmp_path / f) for f in ("out.tsv", "samples.npz", "variants.npz"))
    run_select(["-c", "15", "-o", tsv, "--samples-out", npz, "--variants-out", variants] + files_of(parts))
    order = [names.index(r[0]) for r in rows_of(tsv)]
    with np.load(npz, allow_pickle=False) as z, np.load(variants, allow_pickle=False) as v:
        rank = v["rank"]
        assert (rank == rank_ref.capture_rank(npo.pack_columns(dense), order, 1, dense.shape[0])).all()
        assert (z["new"] == class_ref.class_counts_dense(dense, np.where(rank < 0, len(order), rank), len(order) + 1)[:, :len(order)]).all()


def test_the_loop_s_own_scores_agree(tmp_path):
    """None of the new code: after every utm_step, a still-selectable sample's count of utm_peek_scores is what the panel
    has NOT captured of it, so total - count is the cumulative `new`."""
    from utmos_amd import device
    parts = ("chunk0", "chunk1")
    dense, _, names = original(parts)
    tsv, npz = str(tmp_path / "out.tsv"), str(tmp_path / "samples.npz")
    run_select(["-c", "12", "-o", tsv, "--samples-out", npz] + files_of(parts))
    order = [names.index(r[0]) for r in rows_of(tsv)]
    with np.load(npz, allow_pickle=False) as z:
        new, total = z["new"], z["total"]
    with device.DeviceMatrix(len(names)) as m:
        m.upload_columns(m.add_chunk(dense.shape[0]), npo.pack_columns(dense))
        assert m.var_count().tolist() == total.tolist()
        selectable = np.ones(len(names), bool)
        for i, member in enumerate(order):
            assert m.step()[0] == member
            selectable[member] = False
            counts = m.peek_scores()[0]
            assert ((total - counts)[selectable] == new[:, :i + 1].sum(axis=1)[selectable]).all(), i


def test_a_run_that_selects_nothing_still_writes_the_files(tmp_path):
    parts = ("chunk0",)
    dense, _, names = original(parts)
    out, npz, rep = str(tmp_path / "out.tsv"), str(tmp_path / "samples.npz"), str(tmp_path / "rep.tsv")
    run_select(["-c", "5", "--exclude", ",".join(names), "-o", out, "--samples-out", npz, "--represent-out", rep] + files_of(parts))
    assert open(out).read().count("\n") == 1 and open(rep).read().count("\n") == 1
    with np.load(npz, allow_pickle=False) as z:
        assert z["new"].shape == (len(names), 0) and len(z["panel"]) == 0
        assert (z["missed"] == z["total"]).all() and z["total"].tolist() == dense.sum(axis=0).tolist()


# ----------------------------------------------------------------- spectrum --by-sample
@pytest.mark.parametrize("restricted", [False, True])
def test_spectrum_by_sample(tmp_path, restricted):
    from utmos_amd import spectrum
    parts = ("chunk0", "chunk1")
    dense, _, names = original(parts)
    subset, given = (names[3:200], [names[1], names[5]]) if restricted else (names, [])
    flags = ["--subset", ",".join(subset), "--given", ",".join(given), "--maxmem", "0", "--buffer", "64"] if restricted else []
    plain, tsv, npz = str(tmp_path / "plain.tsv"), str(tmp_path / "s.tsv"), str(tmp_path / "by.npz")
    spectrum.spectrum_main(flags + ["-o", plain] + files_of(parts))
    spectrum.spectrum_main(flags + ["-o", tsv, "--by-sample", npz] + files_of(parts))
    assert open(tsv).read() == open(plain).read()
    listed, panel = [names.index(s) for s in subset], [names.index(g) for g in given]
    hist, count = spectrum_ref.carrier_counts_dense(dense, listed, panel)
    with np.load(npz, allow_pickle=False) as z:
        assert sorted(z.files) == ["samples", "table"] and z["samples"].tolist() == subset
        table = z["table"]
    assert table.dtype == np.int64 and table.shape == (len(listed), len(listed) + 1)
    assert (table == class_ref.class_counts_dense(dense, count, len(listed) + 1, listed)).all()
    assert (table.sum(axis=0) == np.arange(len(listed) + 1) * hist).all()   # c carriers each see the variant once
    assert not table[:, 0].any() and table[:, 1].sum() == hist[1] > 0       # column 1: every sample's singletons
    beyond = ~dense[:, panel].any(axis=1) if panel else np.ones(dense.shape[0], bool)
    assert table.sum(axis=1).tolist() == dense[beyond][:, listed].sum(axis=0).tolist()   # a given sample's variants: nowhere
    assert bool((count < 0).any()) == restricted


# ----------------------------------------------------------------- nothing changes without the flags
@pytest.mark.parametrize("name", ["select_first", "select_multi", "select_af", "select_exclude", "select_weights_subset"])
def test_select_without_the_flags_is_the_answer_key(name, tmp_path, capfd):
    case = CASES[name]
    argv = [os.path.join(ou.GOLD, a) if a in ("weights.txt", "subset.txt", "exclude.txt") else a for a in case["args"]]
    out = str(tmp_path / "out.txt")
    run_select(argv + ["-o", out] + files_of(case["inputs"]))
    assert open(out).read() == ou.golden_text(case)
    capfd.readouterr()
    run_select(argv + files_of(case["inputs"]))                          # the TSV on stdout
    assert capfd.readouterr().out == ou.golden_text(case)
    run_select(argv + ["-o", out, "--samples-out", str(tmp_path / "s.npz"), "--represent-out", str(tmp_path / "r.tsv")] + files_of(case["inputs"]))
    assert open(out).read() == ou.golden_text(case)                      # ... and with them


def test_spectrum_stdout_is_unchanged(tmp_path, capfd):
    from utmos_amd import __main__ as cli
    from utmos_amd import spectrum
    part = os.path.join(ou.GOLD, "tiny.npz")
    matrix, _, samples = npo.build_matrix([ou.load_part("tiny")])
    want, _ = spectrum_ref.carrier_counts_dense(np.asarray(matrix) != 0, range(len(samples)))
    total = int(want.sum())
    text = spectrum.SPECTRUM_HEADER + "".join(f"{c}\t{v}\t{round(int(v) / total, 4)}\n" for c, v in enumerate(want))
    capfd.readouterr()
    assert cli.main(["spectrum", part]) == 0
    assert capfd.readouterr().out == text
    assert cli.main(["spectrum", "--by-sample", str(tmp_path / "b.npz"), part]) == 0
    assert capfd.readouterr().out == text
