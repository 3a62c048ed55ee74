"""`gbrs reconstruct --scan-effects / --scan-lod-drop` and `gbrs scan --scan-effects / --scan-lod-drop` (DESIGN.md §31;
needs an MI355X): the new files against GenomeScan.effects and GenomeScan.run(lod_drop=...) driven by hand, and runs
without the new options, which write what they wrote."""
import os

import numpy as np
import pytest

import grid_cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401

pytestmark = pytest.mark.gpu

MEMBERS = ["covariates", "effect", "founders", "lod", "min_lod", "phenotypes", "points", "position", "rank", "samples", "se", "sigma2",
           "target_chromosome", "target_phenotype", "targets"]
PEAKS = "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max"
SEX = np.array([0, 1, 1, 0, 0, 1], dtype=float)
MIN_LOD, DROP = 0.05, 1.5


def by_hand(scan, y):
    """(run's dict with the intervals, targets [T, 2], points, effects' dict) of a prepared scan."""
    found = scan.run(y, lod_drop=DROP)
    plain = scan.run(y)
    for key in plain:
        np.testing.assert_array_equal(found[key], plain[key], err_msg=key)
    targets = np.argwhere((found["peak_index"] >= 0) & (found["peak_lod"] >= MIN_LOD))
    points = found["peak_index"][targets[:, 0], targets[:, 1]]
    return found, targets, points, scan.effects(y, targets[:, 0], points)


def assert_files(prefix, names, founders, chrom_names, pos, found, targets, points, want):
    z = np.load(f"{prefix}.scan.effects.npz")
    assert sorted(z.files) == MEMBERS
    assert z["phenotypes"].tolist() == names and z["founders"].tolist() == founders and z["min_lod"] == MIN_LOD
    assert z["targets"].tolist() == [names[p] for p in targets[:, 0]]
    assert z["target_chromosome"].tolist() == [chrom_names[c] for c in targets[:, 1]]
    np.testing.assert_array_equal(z["target_phenotype"], targets[:, 0])
    np.testing.assert_array_equal(z["points"], points)
    np.testing.assert_array_equal(z["position"], pos[points])
    for key in ("effect", "se", "lod", "sigma2", "rank"):
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    lines = open(f"{prefix}.scan.effects.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\trank" + "".join(f"\teffect_{f}\tse_{f}" for f in founders)
    expected = []
    for t, (p, c) in enumerate(targets):
        row = [names[p], chrom_names[c], repr(float(pos[points[t]])), repr(float(want["lod"][t])), str(int(want["rank"][t]))]
        for e, s in zip(want["effect"][t], want["se"][t]):
            row += [repr(float(e)), repr(float(s))]
        expected.append("\t".join(row))
    assert lines[1:] == expected and len(expected) >= 3
    s = np.load(f"{prefix}.scan.npz")
    assert s["lod_drop"] == DROP
    np.testing.assert_array_equal(s["support_lo"], found["support_lo"])
    np.testing.assert_array_equal(s["support_hi"], found["support_hi"])
    np.testing.assert_array_equal(s["peak_index"], found["peak_index"])
    lines = open(f"{prefix}.scan.peaks.tsv").read().splitlines()
    assert lines[0] == PEAKS + "\tsupport_lo\tsupport_hi"
    peak, index = found["peak_lod"], found["peak_index"]
    expected = []
    for p, name in enumerate(names):
        on = [c for c in range(len(chrom_names)) if index[p, c] >= 0]
        top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
        for c in on:
            expected.append("\t".join([name, chrom_names[c], repr(float(pos[index[p, c]])), repr(float(peak[p, c])), str(int(c == top)),
                                       repr(float(pos[found["support_lo"][p, c]])), repr(float(pos[found["support_hi"][p, c]]))]))
    assert lines[1:] == expected


def assert_plain_is_the_rest(with_options, plain):
    """The files of a run without the options: the two scan files alone, the peaks file the other's without its last two
    columns, the archive the other's members without the three new ones, byte for byte."""
    folder, stem = os.path.split(plain)
    assert sorted(f for f in os.listdir(folder) if f.startswith(stem + ".")) == [stem + ".scan.npz", stem + ".scan.peaks.tsv"]
    cut = [line.rsplit("\t", 2)[0] for line in open(f"{with_options}.scan.peaks.tsv").read().splitlines()]
    assert open(f"{plain}.scan.peaks.tsv").read() == "\n".join(cut) + "\n" and cut[0] == PEAKS
    a, b = np.load(f"{with_options}.scan.npz"), np.load(f"{plain}.scan.npz")
    assert [k for k in a.files if k not in ("support_lo", "support_hi", "lod_drop")] == b.files
    for key in b.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_reconstruct_with_the_options(tmp_path, tables, caplog, monkeypatch):
    from gbrs_amd import cli
    from gbrs_amd.hmm import DiplotypeHMM
    from gbrs_amd.scan import GenomeScan, rankz
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self.grid_points, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    rng = np.random.default_rng(31)
    names = [f"gene{p}" for p in range(5)]
    values = rng.normal(size=(N_FILES, 5))
    values[:, 4] = 2.5                                                              # a constant phenotype: no peak
    ids = [str(tmp_path / f"with{s}") for s in range(N_FILES)]
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    sample_file = cohort_files(tmp_path, "with")
    pheno = write_table(tmp_path / "pheno.tsv", ids, names, values)
    covar = write_table(tmp_path / "covar.tsv", ids, ["sex"], SEX[:, None])
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]
    scan_args = ["--scan-pheno", pheno, "--scan-covar", covar, "--scan-rankz"]

    def reconstruct(out, extra):
        return cli.main(["reconstruct", "--sample-file", sample_file] + common + scan_args + ["--scan-out", str(tmp_path / out)] + extra)

    stage_file = tmp_path / "stages.json"
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(stage_file))
    with caplog.at_level("WARNING", logger="gbrs"):
        assert reconstruct("own", ["--scan-effects", "--scan-effects-min-lod", str(MIN_LOD), "--scan-lod-drop", str(DROP)]) == 0
    import json
    stages = json.loads(stage_file.read_text())
    assert stages["effects"] > 0 and stages["scan"] >= 0
    monkeypatch.delenv("GBRS_STAGE_TIMES")
    assert not any(r.levelname == "ERROR" for r in caplog.records), [r.getMessage() for r in caplog.records]
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    seen.clear()
    with open(tmp_path / "s0.genes.tpm") as fh:
        founders = fh.readline().rstrip().split("\t")[1:-1]
    assert len(founders) == H_FILES
    chrom_names = [str(c) for c in p0.chroms]
    on = [c for c in p0.chroms if c in grid_b.points]
    pos = np.concatenate([np.asarray(grid_b.points[c], dtype=np.float64) for c in on])
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare(np.column_stack([np.ones(N_FILES), SEX]))
    y = np.column_stack([rankz(values[:, p]) for p in range(5)])
    found, targets, at, want = by_hand(scan, y)
    scan.close()
    assert not (targets[:, 0] == 4).any()
    assert_files(tmp_path / "own", names, founders, chrom_names, pos, found, targets, at, want)
    assert sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("own.")) == \
        ["scan.effects.npz", "scan.effects.tsv", "scan.npz", "scan.peaks.tsv"]
    # a minimum above every peak: both files with their headers only
    caplog.clear()
    with caplog.at_level("WARNING", logger="gbrs"):
        assert reconstruct("none", ["--scan-effects", "--scan-effects-min-lod", "1e9"]) == 0
    seen.clear()
    assert any("no founder effects" in r.getMessage() for r in caplog.records)
    assert len(open(tmp_path / "none.scan.effects.tsv").read().splitlines()) == 1
    assert np.load(tmp_path / "none.scan.effects.npz")["effect"].shape == (0, H_FILES)
    assert open(tmp_path / "none.scan.peaks.tsv").read().splitlines()[0] == PEAKS   # no --scan-lod-drop: the peaks file as it was
    # without the options: the same files, the same bytes
    assert reconstruct("plain", []) == 0
    seen.clear()
    assert_plain_is_the_rest(str(tmp_path / "own"), str(tmp_path / "plain"))
    # every violation is refused before any device work
    caplog.clear()
    for args, message in ((["--scan-effects"], "--scan-effects needs --scan-pheno"),
                          (["--scan-lod-drop", "1.5"], "--scan-lod-drop needs --scan-pheno"),
                          (["--scan-pheno", pheno, "--scan-effects-min-lod", "3"], "--scan-effects-min-lod needs --scan-effects"),
                          (["--scan-pheno", pheno, "--scan-lod-drop", "-1"], "--scan-lod-drop must be")):
        with caplog.at_level("ERROR", logger="gbrs"):
            cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common + args)
        assert any(message in r.getMessage() for r in caplog.records), message
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]


def test_scan_with_the_options(tmp_path, tables):
    """gbrs scan on the exported tables of the six samples, against a scan of those tables by hand."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import read_dosage_table
    from gbrs_amd.postproc import read_grid
    from gbrs_amd.scan import GenomeScan, rankz
    rng = np.random.default_rng(32)
    names = [f"gene{p}" for p in range(4)]
    values = rng.normal(size=(N_FILES, 4))
    ids = [str(tmp_path / f"with{s}") for s in range(N_FILES)]
    pheno = write_table(tmp_path / "pheno.tsv", ids, names, values)
    covar = write_table(tmp_path / "covar.tsv", ids, ["sex"], SEX[:, None])
    assert cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "with"), "-t", tables["tprob"], "-x", tables["avecs"], "-g",
                     tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]) == 0
    listing = tmp_path / "list.tsv"
    listing.write_text("".join(f"{i}\t{i}.interpolated.genoprobs.tsv\n" for i in ids))
    command = ["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar, "--scan-rankz"]
    assert cli.main(command + ["--scan-out", str(tmp_path / "tables"), "--scan-effects", "--scan-effects-min-lod", str(MIN_LOD),
                               "--scan-lod-drop", str(DROP)]) == 0
    file_grid = read_grid(tables["grid"])
    order = list(file_grid)
    with open(f"{ids[0]}.interpolated.genoprobs.tsv") as fh:
        haplotypes = fh.readline().rstrip("\n")[2:].split("\t")
    counts = [len(file_grid[c]) for c in order]
    again = GenomeScan(len(haplotypes), counts)
    for i in ids:
        again.append(read_dosage_table(f"{i}.interpolated.genoprobs.tsv", haplotypes, sum(counts)))
    again.prepare(np.column_stack([np.ones(N_FILES), SEX]))
    y = np.column_stack([rankz(values[:, p]) for p in range(4)])
    found, targets, at, want = by_hand(again, y)
    again.close()
    assert_files(tmp_path / "tables", names, haplotypes, [str(c) for c in order],
                 np.concatenate([np.asarray(file_grid[c], dtype=np.float64) for c in order]), found, targets, at, want)
    # and without the options gbrs scan writes its two files alone, with the bytes they had
    assert cli.main(command + ["--scan-out", str(tmp_path / "bare")]) == 0
    assert_plain_is_the_rest(str(tmp_path / "tables"), str(tmp_path / "bare"))
