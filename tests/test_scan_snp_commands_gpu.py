"""`gbrs reconstruct --scan-snps` and `gbrs scan --snp-file` over the SNP association scan (needs an
MI355X): a SNP file with shuffled chromosomes and a foreign one, against GenomeScan.run_snps driven by hand; runs without
the new options write what they wrote."""
import os

import numpy as np
import pytest

import grid_cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401

pytestmark = pytest.mark.gpu


def write_snp_file(path, grid_points, gene_positions, rng):
    """Six SNPs per grid chromosome, within its grid and within its genes (the per-sample SNP dosages of --snp-file refuse
    a SNP outside the genes), and three on a chromosome nobody has; the lines shuffled."""
    rows = []
    for c, g in grid_points.items():
        genes = np.asarray(gene_positions.get(c, g), dtype=np.float64)
        for k, x in enumerate(rng.uniform(max(g[0], genes.min()), min(g[-1], genes.max()), size=6)):
            rows.append((f"snp_{c}_{k}", c, 1000 * (k + 1), repr(float(x)), "".join(rng.choice(["0", "1"], size=H_FILES))))
    rows += [(f"snp_far_{k}", "Zz", 5 * k, "1.5", "10") for k in range(3)]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    with open(path, "w") as fh:
        fh.write("id\tchr\tbp\tcM\tpattern\n")
        for r in rows:
            fh.write("\t".join(str(v) for v in r) + "\n")
    return str(path), rows


def test_the_commands_against_run_snps(tmp_path, tables, caplog, monkeypatch):
    from gbrs_amd import cli
    from gbrs_amd.hmm import DiplotypeHMM
    from gbrs_amd.scan import GenomeScan
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self.grid_points, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    rng = np.random.default_rng(29)
    names = [f"gene{p}" for p in range(4)]
    values = rng.normal(size=(N_FILES, 4))
    sex = np.array([0, 1, 1, 0, 0, 1], dtype=float)
    ids = lambda stem: [str(tmp_path / f"{stem}{s}") for s in range(N_FILES)]
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    snp_file, rows = write_snp_file(tmp_path / "snps.tsv", grid_b.points, grid_b.positions, rng)
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]

    def reconstruct(stem, extra):
        sample_file = cohort_files(tmp_path, stem)
        pheno = write_table(tmp_path / f"{stem}.pheno.tsv", ids(stem), names, values)
        covar = write_table(tmp_path / f"{stem}.covar.tsv", ids(stem), ["sex"], sex[:, None])
        return cli.main(["reconstruct", "--sample-file", sample_file] + common +
                        ["--scan-pheno", pheno, "--scan-covar", covar, "--scan-out", str(tmp_path / stem), "--snp-file", snp_file,
                         "--scan-lod-matrix"] + extra), pheno, covar

    with caplog.at_level("WARNING", logger="gbrs"):
        status, pheno, covar = reconstruct("with", ["--scan-snps", "--scan-min-lod", "0.05"])
    assert status == 0
    messages = [r.getMessage() for r in caplog.records]
    assert not any(r.levelname == "ERROR" for r in caplog.records), messages
    n_foreign = sum(r[1] not in p0.chroms for r in rows)
    assert n_foreign >= 3 and sum(f"{n_foreign} SNPs on chromosomes" in m for m in messages) == 1      # one warning counts them
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    z = np.load(tmp_path / "with.scan.snps.npz")
    assert z["snp_id"].tolist() == [r[0] for r in rows] and z["chrom"].tolist() == [r[1] for r in rows]
    assert z["pattern"].tolist() == [r[4] for r in rows] and z["phenotypes"].tolist() == names
    assert z["samples"].tolist() == ids("with") and z["covariates"].tolist() == ["intercept", "sex"]
    chrom = np.array([r[1] for r in rows])
    by = [np.flatnonzero(chrom == c) if m else np.zeros(0, dtype=int) for c, m in zip(p0.chroms, points)]
    order = np.concatenate(by)
    mask = np.array([sum(1 << h for h, ch in enumerate(r[4]) if ch == "1") for r in rows], dtype=np.uint32)
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare(np.column_stack([np.ones(N_FILES), sex]))
    scan.set_snps([grid_b.points[c] if m else None for c, m in zip(p0.chroms, points)], [z["cM"][b] for b in by], [mask[b] for b in by])
    want = scan.run_snps(values)
    scan.close()
    foreign = np.setdiff1d(np.arange(len(rows)), order)
    assert len(foreign) == n_foreign
    np.testing.assert_array_equal(z["lod"][:, order], want["lod"])
    np.testing.assert_array_equal(z["used"][order], want["used"])
    assert np.isnan(z["lod"][:, foreign]).all() and not z["used"][foreign].any()
    np.testing.assert_array_equal(z["peak_lod"], want["peak_lod"])
    np.testing.assert_array_equal(z["peak_snp"], np.where(want["peak_index"] >= 0, order[np.maximum(want["peak_index"], 0)], -1))
    lines = open(tmp_path / "with.scan.snps.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max"
    table = [line.split("\t") for line in lines[1:]]
    expected = [(p, ci) for p in range(4) for ci in range(len(points)) if want["peak_index"][p, ci] >= 0 and want["peak_lod"][p, ci] >= 0.05]
    assert len(table) == len(expected) > 0
    for fields, (p, ci) in zip(table, expected):
        j = z["peak_snp"][p, ci]
        assert fields[:3] == [names[p], p0.chroms[ci], rows[j][0]] and fields[5] == rows[j][4]
        assert float(fields[6]) == want["peak_lod"][p, ci] and float(fields[4]) == z["cM"][j]
    assert sum(int(f[7]) for f in table) <= 4
    # without --scan-snps: the scan files and the per-sample SNP dosages are what they are with it, and no SNP scan files
    status, _, _ = reconstruct("plain", [])
    assert status == 0
    assert not [f for f in os.listdir(tmp_path) if f.startswith("plain.scan.snps")]
    with open(tmp_path / "with.scan.peaks.tsv", "rb") as fa, open(tmp_path / "plain.scan.peaks.tsv", "rb") as fb:
        assert fa.read() == fb.read()
    a, b = np.load(tmp_path / "with.scan.npz"), np.load(tmp_path / "plain.scan.npz")
    assert sorted(a.files) == sorted(b.files)
    for key in a.files:
        if key != "samples":
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for s in range(N_FILES):
        a, b = np.load(tmp_path / f"with{s}.snp_dosage.npz"), np.load(tmp_path / f"plain{s}.snp_dosage.npz")
        for key in a.files:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    # every violation is refused before any device work
    caplog.clear()
    for drop, named in (("--snp-file", "--snp-file"), ("--scan-pheno", "--scan-pheno")):
        args = ["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common + \
               ["--scan-pheno", pheno, "--snp-file", snp_file, "--scan-snps"]
        k = args.index(drop)
        with caplog.at_level("ERROR", logger="gbrs"):
            cli.main(args[:k] + args[k + 2:])
        assert any(f"--scan-snps needs {named}" in r.getMessage() for r in caplog.records), named
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]
    # gbrs scan --snp-file on the exported tables of the same samples: the same SNPs, to the rounding of the %.6f tables
    listing = tmp_path / "list.tsv"
    listing.write_text("".join(f"{i}\t{i}.interpolated.genoprobs.tsv\n" for i in ids("with")))
    assert cli.main(["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar,
                     "--scan-out", str(tmp_path / "tables"), "--scan-lod-matrix", "--snp-file", snp_file]) == 0
    t = np.load(tmp_path / "tables.scan.snps.npz")
    assert t["snp_id"].tolist() == z["snp_id"].tolist()
    on_both = order[np.isin(chrom[order], list(grid_b.points))]
    np.testing.assert_array_equal(t["used"][on_both], z["used"][on_both])
    assert np.isnan(t["lod"][:, chrom == "Zz"]).all() and not t["used"][chrom == "Zz"].any()
    # the bound of test_scan_gpu's table comparison: a table rounds a dosage by up to 5e-7, a relative change of the
    # design of a few 1e-6; a LOD moves by (n / 2 / ln 10) e rss0 / rss1 with e = 2e-5
    ratio = 10.0 ** (2.0 * z["lod"][:, on_both] / N_FILES)
    moved = np.abs(t["lod"][:, on_both] - z["lod"][:, on_both])
    print(f"DEVIATION gbrs scan --snp-file on the exported tables against the in-run SNP scan: worst {moved.max():.3g}")
    assert (moved <= N_FILES / 2 / np.log(10) * 2e-5 * ratio).all()
    assert os.path.getsize(tmp_path / "tables.scan.snps.peaks.tsv") > 0
