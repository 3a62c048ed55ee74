"""`gbrs reconstruct --scan-intcovar` and `gbrs scan --scan-intcovar` (needs an MI355X): the two new files
against GenomeScan.prepare_int / run_int driven by hand, and the plain scan's files, which are what a run without the option
writes, byte for byte."""
import os

import numpy as np
import pytest

import grid_cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401

pytestmark = pytest.mark.gpu

MEMBERS = ["phenotypes", "samples", "covariates", "intcovar", "chrom", "pos", "rank_full", "rank_add", "peak_full", "peak_full_index",
           "peak_full_add", "peak_int", "peak_int_index", "lod_full", "lod_add", "lod_int"]
HEADER = "#phenotype\tchromosome\tposition\tlod_full\tlod_add\tlod_int\tdf_full\tdf_add\tint_peak_position\tint_peak_lod"
SEX = np.array([0, 1, 1, 0, 0, 1], dtype=float)
AGE = np.array([0.3, -1.2, 0.8, 1.9, -0.4, 0.1])
MIN_LOD = 0.05


def assert_files(prefix, names, ids, chrom_names, pos, want, info):
    z = np.load(f"{prefix}.scan.int.npz")
    assert z.files == MEMBERS
    assert z["phenotypes"].tolist() == names and z["samples"].tolist() == ids
    assert z["covariates"].tolist() == ["intercept", "sex", "age"] and z["intcovar"].tolist() == ["sex"]
    np.testing.assert_array_equal(z["pos"], pos)
    np.testing.assert_array_equal(z["rank_full"], info["rank_full"])
    np.testing.assert_array_equal(z["rank_add"], info["rank_add"])
    for key in MEMBERS[8:]:
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    lines = open(f"{prefix}.scan.int.peaks.tsv").read().splitlines()
    assert lines[0] == HEADER
    expected = []
    for p, name in enumerate(names):
        for c in range(len(chrom_names)):
            m, mi = want["peak_full_index"][p, c], want["peak_int_index"][p, c]
            if m >= 0 and want["peak_full"][p, c] >= MIN_LOD:
                expected.append("\t".join([name, chrom_names[c], repr(float(pos[m])), repr(float(want["lod_full"][p, m])),
                                           repr(float(want["lod_add"][p, m])), repr(float(want["lod_int"][p, m])),
                                           str(int(info["rank_full"][m])), str(int(info["rank_add"][m])), repr(float(pos[mi])),
                                           repr(float(want["peak_int"][p, c]))]))
    assert lines[1:] == expected and len(expected) >= 3


def assert_the_plain_files_are_untouched(with_option, plain):
    folder, stem = os.path.split(plain)
    assert sorted(f for f in os.listdir(folder) if f.startswith(stem + ".")) == [stem + ".scan.npz", stem + ".scan.peaks.tsv"]
    other = os.path.basename(with_option)
    assert sorted(f for f in os.listdir(folder) if f.startswith(other + ".")) == \
        [other + ".scan.int.npz", other + ".scan.int.peaks.tsv", other + ".scan.npz", other + ".scan.peaks.tsv"]
    assert open(with_option + ".scan.peaks.tsv", "rb").read() == open(plain + ".scan.peaks.tsv", "rb").read()
    a, b = np.load(with_option + ".scan.npz"), np.load(plain + ".scan.npz")      # member by member: a zip carries its hour
    assert a.files == b.files
    for key in b.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_reconstruct_with_the_option(tmp_path, tables, caplog, monkeypatch):
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
    rng = np.random.default_rng(35)
    names = [f"gene{p}" for p in range(5)]
    values = rng.normal(size=(N_FILES, 5))
    values[:, 4] = 2.5                                                              # a constant phenotype: 0.0 throughout
    ids = [str(tmp_path / f"with{s}") for s in range(N_FILES)]
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    sample_file = cohort_files(tmp_path, "with")
    pheno = write_table(tmp_path / "pheno.tsv", ids, names, values)
    covar = write_table(tmp_path / "covar.tsv", ids, ["sex", "age"], np.column_stack([SEX, AGE]))
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]
    scan_args = ["--scan-pheno", pheno, "--scan-covar", covar, "--scan-rankz", "--scan-min-lod", str(MIN_LOD)]

    def reconstruct(out, extra):
        return cli.main(["reconstruct", "--sample-file", sample_file] + common + scan_args + ["--scan-out", str(tmp_path / out)] + extra)

    with caplog.at_level("WARNING", logger="gbrs"):
        assert reconstruct("own", ["--scan-intcovar", "sex"]) == 0
    assert not any(r.levelname == "ERROR" for r in caplog.records), [r.getMessage() for r in caplog.records]
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    seen.clear()
    chrom_names = [str(c) for c in p0.chroms]
    on = [c for c in p0.chroms if c in grid_b.points]
    pos = np.concatenate([np.asarray(grid_b.points[c], dtype=np.float64) for c in on])
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare_int(np.column_stack([np.ones(N_FILES), SEX, AGE]), [1])
    want = scan.run_int(np.column_stack([rankz(values[:, p]) for p in range(5)]))
    info = scan.int_info()
    scan.close()
    assert (want["lod_full"][4] == 0.0).all()
    assert_files(tmp_path / "own", names, ids, chrom_names, pos, want, info)
    assert reconstruct("plain", []) == 0
    seen.clear()
    assert_the_plain_files_are_untouched(str(tmp_path / "own"), str(tmp_path / "plain"))
    # every violation is refused before any device work
    caplog.clear()
    for args, message in ((["--scan-pheno", pheno, "--scan-intcovar", "sex"], "--scan-intcovar needs --scan-covar"),
                          (["--scan-pheno", pheno, "--scan-covar", covar, "--scan-intcovar", "weight"],
                           "--scan-intcovar: weight is not a column of --scan-covar"),
                          (["--scan-pheno", pheno, "--scan-covar", covar, "--scan-intcovar", "sex,sex"], "--scan-intcovar names sex twice"),
                          (["--scan-pheno", pheno, "--scan-covar", covar, "--scan-intcovar", "sex", "--scan-kinship", "loco"],
                           "--scan-intcovar cannot be combined with --scan-kinship")):
        with caplog.at_level("ERROR", logger="gbrs"):
            cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common + args)
        assert any(message in r.getMessage() for r in caplog.records), message
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]


def test_scan_with_the_option(tmp_path, tables):
    """gbrs scan on the exported tables of the six samples, against a scan of those tables by hand."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import read_dosage_table
    from gbrs_amd.postproc import read_grid
    from gbrs_amd.scan import GenomeScan, rankz
    rng = np.random.default_rng(36)
    names = [f"gene{p}" for p in range(4)]
    values = rng.normal(size=(N_FILES, 4))
    ids = [str(tmp_path / f"with{s}") for s in range(N_FILES)]
    pheno = write_table(tmp_path / "pheno.tsv", ids, names, values)
    covar = write_table(tmp_path / "covar.tsv", ids, ["sex", "age"], np.column_stack([SEX, AGE]))
    assert cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "with"), "-t", tables["tprob"], "-x", tables["avecs"], "-g",
                     tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]) == 0
    listing = tmp_path / "list.tsv"
    listing.write_text("".join(f"{i}\t{i}.interpolated.genoprobs.tsv\n" for i in ids))
    command = ["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar, "--scan-rankz",
               "--scan-min-lod", str(MIN_LOD)]
    assert cli.main(command + ["--scan-out", str(tmp_path / "tables"), "--scan-intcovar", "sex"]) == 0
    file_grid = read_grid(tables["grid"])
    order = list(file_grid)
    with open(f"{ids[0]}.interpolated.genoprobs.tsv") as fh:
        haplotypes = fh.readline().rstrip("\n")[2:].split("\t")
    counts = [len(file_grid[c]) for c in order]
    again = GenomeScan(len(haplotypes), counts)
    for i in ids:
        again.append(read_dosage_table(f"{i}.interpolated.genoprobs.tsv", haplotypes, sum(counts)))
    again.prepare_int(np.column_stack([np.ones(N_FILES), SEX, AGE]), [1])
    want = again.run_int(np.column_stack([rankz(values[:, p]) for p in range(4)]))
    info = again.int_info()
    again.close()
    assert_files(tmp_path / "tables", names, ids, [str(c) for c in order],
                 np.concatenate([np.asarray(file_grid[c], dtype=np.float64) for c in order]), want, info)
    assert cli.main(command + ["--scan-out", str(tmp_path / "bare")]) == 0
    assert_the_plain_files_are_untouched(str(tmp_path / "tables"), str(tmp_path / "bare"))
