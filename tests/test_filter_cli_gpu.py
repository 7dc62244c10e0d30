"""GPU: the variant filters through the command line.  The invariant: `select` with filter flags on the committed parts
writes, byte for byte, what `select` without them writes on copies of the parts from which the dropped records had been
removed beforehand (made here with numpy) -- the TSV and the --variants-out arrays, `row` mapped through the kept records."""
import os

import numpy as np
import pytest

import oracle_util as ou

pytestmark = pytest.mark.gpu

PARTS = ["chunk0", "chunk1", "chunk2"]


def run_select(argv):
    from utmos_amd.select import select_main
    select_main(argv)


def load_parts(names):
    parts = [ou.load_part(n) for n in names]
    n_samp = len(parts[0]["samples"])
    dense = [np.unpackbits(p["GT"], axis=1, count=n_samp).astype(bool) for p in parts]
    return parts, dense


def write_copies(tmp_path, parts, record_keep, tag):
    paths = []
    for k, (part, keep) in enumerate(zip(parts, record_keep)):
        path = str(tmp_path / f"{tag}_{k}.npz")
        np.savez(path, GT=part["GT"][keep], AF=np.asarray(part["AF"]).reshape(-1)[keep], samples=part["samples"])
        paths.append(path)
    return paths


def golden_paths(names):
    return [os.path.join(ou.GOLD, n + ".npz") for n in names]


def compare(tmp_path, names, filter_flags, other_flags, record_keep, tag):
    """select filter_flags other_flags originals == select other_flags copies: TSV and --variants-out."""
    parts, _ = load_parts(names)
    copies = write_copies(tmp_path, parts, record_keep, tag)
    out_a, out_b = str(tmp_path / f"{tag}_a.tsv"), str(tmp_path / f"{tag}_b.tsv")
    var_a, var_b = str(tmp_path / f"{tag}_a.npz"), str(tmp_path / f"{tag}_b.npz")
    run_select(filter_flags + other_flags + ["--variants-out", var_a, "-o", out_a] + golden_paths(names))
    run_select(other_flags + ["--variants-out", var_b, "-o", out_b] + copies)
    text = open(out_a).read()
    assert text == open(out_b).read(), tag
    assert len(text.splitlines()) > 2, tag                          # the case selects something
    a, b = np.load(var_a), np.load(var_b)
    assert a["rank"].tolist() == b["rank"].tolist() and a["part"].tolist() == b["part"].tolist(), tag
    mapped = np.concatenate([np.flatnonzero(record_keep[p])[b["row"][b["part"] == p]] for p in range(len(names))])
    assert a["row"].tolist() == mapped.tolist(), tag
    if "af" in a.files:
        assert a["af"].tolist() == b["af"].tolist(), tag
    return text


def informative(dense):
    return [d.any(axis=1) for d in dense]


def test_min_af_plain(tmp_path):
    parts, dense = load_parts(PARTS)
    bound = float(np.median(np.concatenate([np.asarray(p["AF"]).reshape(-1) for p in parts])))
    keep = [np.asarray(p["AF"]).reshape(-1) >= bound for p in parts]
    assert 0 < sum(int((k & i).sum()) for k, i in zip(keep, informative(dense))) < sum(int(i.sum()) for i in informative(dense))
    compare(tmp_path, PARTS, ["--min-af", repr(bound)], ["-c", "8"], keep, "minaf")


def test_max_af_with_af_scores(tmp_path):
    parts, dense = load_parts(PARTS)
    bound = float(np.quantile(np.concatenate([np.asarray(p["AF"]).reshape(-1) for p in parts]), 0.7))
    keep = [np.asarray(p["AF"]).reshape(-1) <= bound for p in parts]
    compare(tmp_path, PARTS, ["--max-af", repr(bound)], ["--af", "-c", "8"], keep, "maxaf")


def test_min_carriers_counts_the_cohort_with_weights_subset_and_exclude(tmp_path):
    parts, dense = load_parts(PARTS)
    names = np.asarray(parts[0]["samples"]).astype(str)
    subset, exclude = ou.read_list(os.path.join(ou.GOLD, "subset.txt")), ou.read_list(os.path.join(ou.GOLD, "exclude.txt"))
    cohort = np.isin(names, subset) & ~np.isin(names, exclude)
    assert 2 < cohort.sum() < len(names)
    keep = [d[:, cohort].sum(axis=1) >= 2 for d in dense]
    whole = [d.sum(axis=1) >= 2 for d in dense]
    assert any((k != w).any() for k, w in zip(keep, whole))         # the cohort matters in this case
    flags = ["--weights", os.path.join(ou.GOLD, "weights.txt"), "--subset", os.path.join(ou.GOLD, "subset.txt"), "--exclude",
             os.path.join(ou.GOLD, "exclude.txt"), "-c", "6"]
    compare(tmp_path, PARTS, ["--min-carriers", "2"], flags, keep, "mincar")


def test_max_carriers_at_depth_2(tmp_path):
    parts, dense = load_parts(PARTS)
    keep = [d.sum(axis=1) <= 10 for d in dense]
    compare(tmp_path, PARTS, ["--max-carriers", "10"], ["--depth", "2", "-c", "8"], keep, "maxcar")


def variant_list(path, dense, rng, share):
    """A list file naming `share` of the informative records of every part; -> the per-part boolean over all records."""
    listed, part, row = [], [], []
    for p, inf in enumerate(informative(dense)):
        chosen = np.zeros(len(inf), bool)
        rows = np.flatnonzero(inf)
        chosen[rng.choice(rows, int(len(rows) * share), replace=False)] = True
        listed.append(chosen)
        part += [p] * int(chosen.sum())
        row += np.flatnonzero(chosen).tolist()
    order = rng.permutation(len(part))                              # the list is a set: its order means nothing
    np.savez(path, part=np.asarray(part, np.int32)[order], row=np.asarray(row, np.int64)[order])
    return listed


def test_keep_variants_in_topn_mode(tmp_path):
    parts, dense = load_parts(PARTS)
    path = str(tmp_path / "keep.npz")
    listed = variant_list(path, dense, np.random.default_rng(1), 0.3)
    compare(tmp_path, PARTS, ["--keep-variants", path], ["--mode", "topN", "-c", "8"], listed, "keep")


def test_drop_variants_with_many_chunks_some_emptied(tmp_path):
    parts, dense = load_parts(PARTS)
    path = str(tmp_path / "drop.npz")
    # everything in the middle part and the tail of the first goes: with 64 variants per chunk whole chunks are emptied
    listed = [inf.copy() for inf in informative(dense)]
    listed[0][:len(listed[0]) // 3] = False
    listed[2][len(listed[2]) // 2:] = False
    part = np.concatenate([np.full(int(l.sum()), p, np.int32) for p, l in enumerate(listed)])
    row = np.concatenate([np.flatnonzero(l) for l in listed])
    np.savez(path, part=part, row=row)
    keep = [inf & ~l for inf, l in zip(informative(dense), listed)]
    assert int(listed[1].sum()) > 128 and sum(int(k.sum()) for k in keep) > 64
    compare(tmp_path, PARTS, ["--drop-variants", path], ["--maxmem", "0", "--buffer", "64", "-c", "8"], keep, "drop")


def test_two_combinations(tmp_path):
    parts, dense = load_parts(["mid"])
    af = np.asarray(parts[0]["AF"]).reshape(-1)
    bound = float(np.quantile(af, 0.3))
    keep = [(af >= bound) & (dense[0].sum(axis=1) <= 40)]
    compare(tmp_path, ["mid"], ["--min-af", repr(bound), "--max-carriers", "40"], ["--af", "-c", "6"], keep, "combo1")
    parts, dense = load_parts(PARTS)
    path = str(tmp_path / "drop2.npz")
    listed = variant_list(path, dense, np.random.default_rng(2), 0.2)
    keep = [(d.sum(axis=1) >= 2) & ~l for d, l in zip(dense, listed)]
    compare(tmp_path, PARTS, ["--min-carriers", "2", "--drop-variants", path], ["-c", "6"], keep, "combo2")


def test_a_filtered_run_from_a_store_and_the_filter_command(tmp_path):
    from utmos_amd.variant_filter import filter_main
    parts, dense = load_parts(PARTS)
    keep = [d.sum(axis=1) >= 2 for d in dense]
    copies = write_copies(tmp_path, parts, keep, "store")
    full, cut = str(tmp_path / "full.utm"), str(tmp_path / "cut.utm")
    outs = [str(tmp_path / f"s{k}.tsv") for k in range(5)]
    run_select(["--af", "-c", "8", "--lowmem", full, "-o", outs[0]] + golden_paths(PARTS))      # writes the store, unfiltered
    run_select(["--af", "-c", "8", "--min-carriers", "2", "-o", outs[1], full])                 # the filtered run from it
    run_select(["--af", "-c", "8", "--lowmem", cut, "-o", outs[2]] + copies)                    # float32 AF, like a store
    assert open(outs[1]).read() == open(outs[2]).read() != open(outs[0]).read()
    # filter -o: the store of the kept variants gives the same selection, and --kept-out says where its rows came from
    made, kept_path = str(tmp_path / "made.utm"), str(tmp_path / "kept.npz")
    filter_main(["--min-carriers", "2", "--af", "-o", made, "--kept-out", kept_path] + golden_paths(PARTS))
    run_select(["--af", "-c", "8", "-o", outs[3], made])
    assert open(outs[3]).read() == open(outs[2]).read()
    kept = np.load(kept_path)
    assert kept["part"].tolist() == np.concatenate([np.full(int(k.sum()), p) for p, k in enumerate(keep)]).tolist()
    assert kept["row"].tolist() == np.concatenate([np.flatnonzero(k) for k in keep]).tolist()
    assert kept["af"].tolist() == np.concatenate([np.asarray(p["AF"]).reshape(-1)[k] for p, k in zip(parts, keep)]).tolist()
    # a store without AF cannot answer an AF criterion
    plain = str(tmp_path / "plain.utm")
    run_select(["-c", "2", "--lowmem", plain, "-o", outs[4]] + golden_paths(PARTS))
    with pytest.raises(SystemExit) as err:
        run_select(["--max-af", "0.1", "-c", "2", "-o", outs[4], plain])
    assert err.value.code == 1


def rows_of(path):
    return [line.split("\t") for line in open(path).read().splitlines()[1:]]


def test_the_missed_variants_of_a_run_fed_back(tmp_path):
    first, var, again, rest = (str(tmp_path / n) for n in ("first.tsv", "v.npz", "again.tsv", "rest.tsv"))
    run_select(["-c", "5", "--variants-out", var, "-o", first] + golden_paths(PARTS))
    v = np.load(var)
    missed = v["rank"] < 0
    assert 0 < missed.sum() < len(missed)
    listed = str(tmp_path / "missed.npz")
    np.savez(listed, part=v["part"][missed], row=v["row"][missed])  # (the README's recipe)
    run_select(["-c", "-1", "--keep-variants", listed, "-o", rest] + golden_paths(PARTS))
    assert int(rows_of(rest)[-1][3]) == int(missed.sum())
    run_select(["-c", "5", "--drop-variants", listed, "-o", again] + golden_paths(PARTS))
    a, b = rows_of(first), rows_of(again)
    assert [r[0] for r in a] == [r[0] for r in b] and [r[2:4] for r in a] == [r[2:4] for r in b]
    assert float(b[-1][4]) == 1.0 and float(a[-1][4]) < 1.0


def test_no_variants_left_is_an_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as err:
        run_select(["--min-af", "2.0", "-o", str(tmp_path / "o.tsv")] + golden_paths(PARTS))
    assert err.value.code == 1 and "no variants are left" in capsys.readouterr().err
    listed = str(tmp_path / "unknown.npz")
    np.savez(listed, part=np.array([7], np.int32), row=np.array([0], np.int64))
    with pytest.raises(SystemExit) as err:
        run_select(["--keep-variants", listed, "-o", str(tmp_path / "o.tsv")] + golden_paths(PARTS))
    assert err.value.code == 1 and "part 7, row 0" in capsys.readouterr().err
