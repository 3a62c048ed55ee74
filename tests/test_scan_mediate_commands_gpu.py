"""`gbrs reconstruct --scan-mediate` and `gbrs scan --scan-mediate` over the mediation pass (needs an
MI355X): both files against GenomeScan.mediate driven by hand, the mediator table, a minimum LOD above every peak, and
runs without the new options, which write what they wrote."""
import os

import numpy as np
import pytest

import grid_cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401

pytestmark = pytest.mark.gpu

HEADER = "#phenotype\tchromosome\tposition\tlod\tmediator\tlod_mediated\tdrop\tz"
MEMBERS = ["best_index", "best_lod", "covariates", "lod0", "lod_med", "mean", "mediators", "min_lod", "n_used", "phenotypes", "points",
           "position", "samples", "sd", "target_chromosome", "target_phenotype", "targets", "used"]


def by_hand(scan, y, z, min_lod, top):
    """(targets [T, 2], points, GenomeScan.mediate's dict) of a prepared scan: every peak of at least min_lod."""
    found = scan.run(y)
    targets = np.argwhere((found["peak_index"] >= 0) & (found["peak_lod"] >= min_lod))
    points = found["peak_index"][targets[:, 0], targets[:, 1]]
    return targets, points, scan.mediate(y[:, targets[:, 0]], points, z, top=top, want_lod=True)


def assert_files(prefix, names, mediators, chrom_names, pos, targets, points, want):
    z = np.load(f"{prefix}.scan.mediation.npz")
    assert sorted(z.files) == MEMBERS
    assert z["phenotypes"].tolist() == names and z["mediators"].tolist() == mediators
    assert z["targets"].tolist() == [names[p] for p in targets[:, 0]]
    assert z["target_chromosome"].tolist() == [chrom_names[c] for c in targets[:, 1]]
    np.testing.assert_array_equal(z["target_phenotype"], targets[:, 0])
    np.testing.assert_array_equal(z["points"], points)
    np.testing.assert_array_equal(z["position"], pos[points])
    for key in ("lod0", "best_index", "best_lod", "mean", "sd", "n_used", "lod_med", "used"):
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    lines = open(f"{prefix}.scan.mediation.tsv").read().splitlines()
    assert lines[0] == HEADER
    expected = []
    for t, (p, c) in enumerate(targets):
        for k in range(want["best_index"].shape[1]):
            q = want["best_index"][t, k]
            if q >= 0:
                v, lod0 = float(want["best_lod"][t, k]), float(want["lod0"][t])
                zed = repr((v - float(want["mean"][t])) / float(want["sd"][t])) if want["sd"][t] > 0 else "NA"
                expected.append("\t".join([names[p], chrom_names[c], repr(float(pos[points[t]])), repr(lod0), mediators[q], repr(v),
                                           repr(lod0 - v), zed]))
    assert lines[1:] == expected
    return z


def test_the_commands_against_mediate(tmp_path, tables, caplog, monkeypatch):
    from gbrs_amd import cli
    from gbrs_amd.hmm import DiplotypeHMM, read_dosage_table
    from gbrs_amd.postproc import read_grid
    from gbrs_amd.scan import GenomeScan, rankz
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self.grid_points, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    rng = np.random.default_rng(30)
    names = [f"gene{p}" for p in range(5)]
    values = rng.normal(size=(N_FILES, 5))
    values[:, 4] = 2.5                                                            # a constant phenotype: no peak, no mediator
    other_names = [f"protein{p}" for p in range(3)]
    other = rng.normal(size=(N_FILES, 3))
    sex = np.array([0, 1, 1, 0, 0, 1], dtype=float)
    ids = [str(tmp_path / f"with{s}") for s in range(N_FILES)]
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    sample_file = cohort_files(tmp_path, "with")
    pheno = write_table(tmp_path / "pheno.tsv", ids, names, values)
    covar = write_table(tmp_path / "covar.tsv", ids, ["sex"], sex[:, None])
    mediators = write_table(tmp_path / "mediators.tsv", ids[::-1], other_names, other[::-1])       # the rows in another order
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]
    scan_args = ["--scan-pheno", pheno, "--scan-covar", covar, "--scan-rankz"]

    def reconstruct(out, extra):
        return cli.main(["reconstruct", "--sample-file", sample_file] + common + scan_args + ["--scan-out", str(tmp_path / out)] + extra)

    stage_file = tmp_path / "stages.json"
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(stage_file))
    with caplog.at_level("WARNING", logger="gbrs"):
        assert reconstruct("own", ["--scan-mediate", "--scan-mediate-min-lod", "0.05", "--scan-mediate-top", "3"]) == 0
    import json
    stages = json.loads(stage_file.read_text())
    assert stages["mediate"] > 0 and stages["scan"] >= 0
    monkeypatch.delenv("GBRS_STAGE_TIMES")
    assert not any(r.levelname == "ERROR" for r in caplog.records), [r.getMessage() for r in caplog.records]
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    seen.clear()
    chrom_names = [str(c) for c in p0.chroms]
    on = [c for c in p0.chroms if c in grid_b.points]
    pos = np.concatenate([np.asarray(grid_b.points[c], dtype=np.float64) for c in on])
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare(np.column_stack([np.ones(N_FILES), sex]))
    y = np.column_stack([rankz(values[:, p]) for p in range(5)])
    targets, at, want = by_hand(scan, y, y, 0.05, 3)
    assert len(targets) >= 4 and not (targets[:, 0] == 4).any()
    z = assert_files(tmp_path / "own", names, names, chrom_names, pos, targets, at, want)
    assert z["samples"].tolist() == ids and z["covariates"].tolist() == ["intercept", "sex"] and z["min_lod"] == 0.05
    assert not z["used"][:, 4].any() and not z["used"][np.arange(len(targets)), targets[:, 0]].any()
    # the mediators from their own table, its rows matched by id; --scan-rankz applies to it
    assert reconstruct("table", ["--scan-mediate", "--scan-mediate-min-lod", "0.05", "--scan-mediator-file", mediators]) == 0
    seen.clear()
    zt = np.column_stack([rankz(other[:, q]) for q in range(3)])
    targets_t, at_t, want_t = by_hand(scan, y, zt, 0.05, 5)
    assert_files(tmp_path / "table", names, other_names, chrom_names, pos, targets_t, at_t, want_t)
    assert want_t["best_index"].shape == (len(targets), 5) and (want_t["best_index"][:, 3:] == -1).all()
    # a minimum above every peak: both files with their headers only
    caplog.clear()
    with caplog.at_level("WARNING", logger="gbrs"):
        assert reconstruct("none", ["--scan-mediate", "--scan-mediate-min-lod", "1e9"]) == 0
    seen.clear()
    assert any("nothing to mediate" in r.getMessage() for r in caplog.records)
    assert open(tmp_path / "none.scan.mediation.tsv").read() == HEADER + "\n"
    empty = np.load(tmp_path / "none.scan.mediation.npz")
    assert sorted(empty.files) == MEMBERS and empty["lod0"].shape == (0,) and empty["best_index"].shape == (0, 5)
    assert empty["lod_med"].shape == (0, 5) and empty["mediators"].tolist() == names
    scan.close()
    # without the options: the same files, the same bytes (an .npz member by member: the archive carries its time)
    before = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path) if f.startswith("with0.")}
    assert reconstruct("plain", []) == 0
    seen.clear()
    assert sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("plain.")) == ["scan.npz", "scan.peaks.tsv"]
    assert sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("own.")) == \
        ["scan.mediation.npz", "scan.mediation.tsv", "scan.npz", "scan.peaks.tsv"]
    with open(tmp_path / "own.scan.peaks.tsv", "rb") as fa, open(tmp_path / "plain.scan.peaks.tsv", "rb") as fb:
        assert fa.read() == fb.read()
    a, b = np.load(tmp_path / "own.scan.npz"), np.load(tmp_path / "plain.scan.npz")
    assert a.files == b.files
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    after = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path) if f.startswith("with0.")}
    assert sorted(after) == sorted(before)
    for f in before:
        if not f.endswith(".npz"):
            assert after[f] == before[f], f
    # every violation is refused before any device work
    caplog.clear()
    for args, message in ((["--scan-mediate"], "--scan-mediate needs --scan-pheno"),
                          (["--scan-pheno", pheno, "--scan-mediate-top", "3"], "--scan-mediate-top needs --scan-mediate"),
                          (["--scan-pheno", pheno, "--scan-mediate", "--scan-mediate-top", "65"], "--scan-mediate-top must be")):
        with caplog.at_level("ERROR", logger="gbrs"):
            cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common + args)
        assert any(message in r.getMessage() for r in caplog.records), message
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]
    # gbrs scan --scan-mediate on the exported tables of the same samples, against a scan of those tables by hand
    listing = tmp_path / "list.tsv"
    listing.write_text("".join(f"{i}\t{i}.interpolated.genoprobs.tsv\n" for i in ids))
    assert cli.main(["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar,
                     "--scan-rankz", "--scan-out", str(tmp_path / "tables"), "--scan-mediate", "--scan-mediate-min-lod", "0.05",
                     "--scan-mediate-top", "2", "--scan-mediator-file", mediators]) == 0
    file_grid = read_grid(tables["grid"])
    order = list(file_grid)
    with open(f"{ids[0]}.interpolated.genoprobs.tsv") as fh:
        haplotypes = fh.readline().rstrip("\n")[2:].split("\t")
    counts = [len(file_grid[c]) for c in order]
    again = GenomeScan(len(haplotypes), counts)
    for i in ids:
        again.append(read_dosage_table(f"{i}.interpolated.genoprobs.tsv", haplotypes, sum(counts)))
    again.prepare(np.column_stack([np.ones(N_FILES), sex]))
    targets_f, at_f, want_f = by_hand(again, y, zt, 0.05, 2)
    again.close()
    assert len(targets_f) >= 4
    assert_files(tmp_path / "tables", names, other_names, [str(c) for c in order],
                 np.concatenate([np.asarray(file_grid[c], dtype=np.float64) for c in order]), targets_f, at_f, want_f)
    # and without the options gbrs scan writes its two files alone
    assert cli.main(["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar,
                     "--scan-rankz", "--scan-out", str(tmp_path / "bare")]) == 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("bare.")) == ["bare.scan.npz", "bare.scan.peaks.tsv"]
    with open(tmp_path / "tables.scan.peaks.tsv", "rb") as fa, open(tmp_path / "bare.scan.peaks.tsv", "rb") as fb:
        assert fa.read() == fb.read()
    a, b = np.load(tmp_path / "tables.scan.npz"), np.load(tmp_path / "bare.scan.npz")
    assert a.files == b.files
    for key in a.files:
        assert a[key].tobytes() == b[key].tobytes(), key
