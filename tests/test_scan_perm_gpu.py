"""Permutation thresholds of the genome scan on the device (gbrs_scan_permute, GenomeScan.permute) and the
commands over them (needs an MI355X).  The rule in numpy: tests/scan_perm_restate.py; cohorts and the two host routes:
tests/scan_cases.py.

The permutations equal the restatement's exactly.  perm_max is held against both host routes to
scan_cases.DEVICE_FACTOR times the floor the two have between themselves on the permuted columns
(scan_perm_restate.MEASURED_FLOOR_PERM); everything else is bit equality."""
import json
import os

import numpy as np
import pytest

import grid_cases
import scan_cases as cases
import scan_perm_restate as restate
from test_scan_gpu import scan_of, write_table

pytestmark = pytest.mark.gpu

TOL = cases.DEVICE_FACTOR * restate.MEASURED_FLOOR_PERM
BITS = (8, 70, 4, 130, (1, 65, 9))


@pytest.mark.parametrize("n", [3, 31, 32, 33, 63, 64, 65, 70, 300, 256, 257, 512, 513])
def test_the_permutations_equal_the_restatement(n):
    """Both sides of the K chunk (32), of a wavefront (64) and of the rank kernel's 256-sample tile - exactly one tile,
    one sample past it, exactly two and one past two; B = 1 and 7; a seed whose upper word is in use."""
    from gbrs_amd.scan import GenomeScan
    rng = np.random.default_rng(n)
    scan = GenomeScan(2, [3])
    scan.append(rng.dirichlet(np.ones(2), size=(n, 3)))
    scan.prepare()
    Y = rng.normal(size=(n, 2))
    for seed in (restate.SEED, restate.SEED_HIGH):
        for B in (1, 7):
            got = scan.permute(Y, B, seed=seed, want_index=True)
            assert got["perm_index"].dtype == np.int32 and got["perm_max"].shape == (2, B)
            np.testing.assert_array_equal(got["perm_index"], restate.permutations(seed, B, n), err_msg=f"seed {seed}, B {B}")
    scan.close()


@pytest.mark.parametrize("case", restate.ORDINARY + restate.ORDINARY_LARGE, ids=cases.case_id)
def test_perm_max_against_both_host_routes(case):
    """A case of ORDINARY within TOL, a large case within the device factor of its own recorded floor (measured_floor_perm
    is MEASURED_FLOOR_PERM for every case of ORDINARY)."""
    _, _, Y, _ = cases.build(case)
    perm = restate.expected(case)[0]
    by_rule, by_lstsq = restate.expected_max(case)
    scan = scan_of(case)
    got = scan.permute(Y, restate.N_PERM, seed=restate.SEED, want_index=True)
    timing, info = scan.perm_info(), scan.info()
    scan.close()
    np.testing.assert_array_equal(got["perm_index"], perm)
    tol = cases.DEVICE_FACTOR * restate.measured_floor_perm(case)
    assert tol == TOL or case in restate.ORDINARY_LARGE
    worst, worst_ls = cases.deviation(got["perm_max"], by_rule), cases.deviation(got["perm_max"], by_lstsq)
    print(f"DEVIATION device perm_max against scan_rule {worst:.3g}, against scan_lstsq {worst_ls:.3g}, tolerance {tol:.3g}, "
          f"{cases.case_id(case)}")
    assert worst <= tol and worst_ls <= tol
    assert (timing["P"], timing["B"]) == (case[3], restate.N_PERM)
    assert timing["permute_ms"] >= timing["product_ms"] > 0 and timing["peak_device_bytes"] > info["device_bytes"]
    assert info["run_ms"] == 0.0                                   # the pass is not a run: gbrs_scan_info_t is as it was


def test_a_column_has_the_same_bits_wherever_it_stands():
    """130 phenotypes x 9 permutations are 1170 columns in three chunks of 512: phenotype 56 (columns 504 .. 512) and 113
    (1017 .. 1025) straddle a chunk boundary.  A phenotype alone, the first 65 phenotypes (585 columns), the first 4 of
    the 9 permutations and one (p, b) asked for alone carry the bits they have in the whole pass; run() before and after
    the pass returns the same bits and the handle's info is as it was."""
    _, _, Y, _ = cases.build(BITS)
    scan = scan_of(BITS)
    before, info_before = scan.run(Y), scan.info()
    full = scan.permute(Y, 9, seed=restate.SEED)["perm_max"]
    after, info_after = scan.run(Y), scan.info()
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    for key in ("n", "M", "H", "c", "device_bytes"):
        assert info_after[key] == info_before[key], key
    np.testing.assert_array_equal(info_after["rank"], info_before["rank"])
    assert full.shape == (130, 9)
    np.testing.assert_array_equal(scan.permute(Y, 9, seed=restate.SEED)["perm_max"], full)
    for p in (0, 56, 113, 129):
        np.testing.assert_array_equal(scan.permute(Y[:, p], 9, seed=restate.SEED)["perm_max"][0], full[p], err_msg=f"phenotype {p} alone")
    np.testing.assert_array_equal(scan.permute(Y[:, :65], 9, seed=restate.SEED)["perm_max"], full[:65])
    np.testing.assert_array_equal(scan.permute(Y, 4, seed=restate.SEED)["perm_max"], full[:, :4])
    assert scan.permute(Y[:, 56], 9, seed=restate.SEED)["perm_max"][0, 8] == full[56, 8]
    assert scan.permute(Y[:, 113], 8, seed=restate.SEED)["perm_max"][0, 7] == full[113, 7]
    assert not np.array_equal(scan.permute(Y[:, :2], 9, seed=restate.SEED + 1)["perm_max"], full[:2])
    wide = scan.permute(np.tile(Y, (1, 5))[:, :600], 2, seed=restate.SEED)["perm_max"]      # the phenotypes arrive in two uploads of 512 and 88
    np.testing.assert_array_equal(wide, np.tile(full[:, :2], (5, 1))[:600])
    scan.close()
    for size in (1, 3):
        pieces = [size] * (70 // size) + ([70 % size] if 70 % size else [])
        cut = scan_of(BITS, pieces)
        np.testing.assert_array_equal(cut.permute(Y, 4, seed=restate.SEED)["perm_max"], full[:, :4], err_msg=f"pieces of {size}")
        cut.close()


def test_the_chromosome_mask():
    """Only the last chromosome: the maximum the restatement takes there.  The maxima over single chromosomes combine to
    the maximum over all, exactly.  A chromosome without points adds nothing, and a mask of nothing else is refused."""
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    _, _, Y, _ = cases.build(BITS)
    scan = scan_of(BITS)
    everywhere = scan.permute(Y, restate.N_PERM, seed=restate.SEED)["perm_max"]
    single = [scan.permute(Y, restate.N_PERM, seed=restate.SEED, chromosomes=np.arange(3) == c)["perm_max"] for c in range(3)]
    with pytest.raises(ValueError, match="mask has shape"):
        scan.permute(Y, 2, chromosomes=[True, False])
    scan.close()
    for route in restate.expected_max(BITS, mask=(False, False, True)):
        assert cases.deviation(single[2], route) <= TOL
    np.testing.assert_array_equal(np.maximum(np.maximum(single[0], single[1]), single[2]), everywhere)
    assert (single[2] < everywhere).any()
    rng = np.random.default_rng(2)
    holes = GenomeScan(2, [5, 0, 4])
    holes.append(rng.dirichlet(np.ones(2), size=(6, 9)))
    holes.prepare()
    y = rng.normal(size=(6, 3))
    with pytest.raises(_lib.GbrsHipError, match="the chromosome mask selects no grid point"):
        holes.permute(y, 4, chromosomes=[False, True, False])
    with pytest.raises(_lib.GbrsHipError, match="selects no grid point"):
        holes.permute(y, 4, chromosomes=[False, False, False])
    first = holes.permute(y, 4, chromosomes=[True, False, False])["perm_max"]
    np.testing.assert_array_equal(holes.permute(y, 4, chromosomes=[True, True, False])["perm_max"], first)
    assert np.isfinite(holes.permute(y, 4)["perm_max"]).all()                    # the empty chromosome's NaN stays out
    holes.close()


def test_edge_columns():
    """A constant phenotype scores 0.0 under every permutation, next to a phenotype that keeps its bits.  With three
    samples of two founders one residual degree of freedom is left: the result is what the restatement gives, the
    infinities at the same places, the finite values within the device factor of what the two host routes differ by on
    these very columns (their floor depends on the column: scan_cases.MEASURED_SATURATED)."""
    _, _, Y, _ = cases.build(BITS)
    scan = scan_of(BITS)
    alone = scan.permute(Y[:, 0], 6, seed=restate.SEED)["perm_max"]
    got = scan.permute(np.column_stack([np.full(70, 3.7), Y[:, 0], np.zeros(70), np.full(70, -1e6)]), 6, seed=restate.SEED)["perm_max"]
    scan.close()
    assert (got[[0, 2, 3]] == 0.0).all()
    np.testing.assert_array_equal(got[1:2], alone)
    tiny = (2, 3, 1, 1, cases.POINTS)
    _, _, y, _ = cases.build(tiny)
    by_rule, by_lstsq = restate.expected_max(tiny)
    scan = scan_of(tiny)
    got = scan.permute(y, restate.N_PERM, seed=restate.SEED, want_index=True)
    scan.close()
    np.testing.assert_array_equal(got["perm_index"], restate.expected(tiny)[0])
    own = cases.DEVICE_FACTOR * max(restate.MEASURED_FLOOR_PERM, cases.deviation(by_rule, by_lstsq))
    worst, worst_ls = cases.deviation(got["perm_max"], by_rule), cases.deviation(got["perm_max"], by_lstsq)
    print(f"DEVIATION one residual degree: device against scan_rule {worst:.3g}, against scan_lstsq {worst_ls:.3g}, tolerance "
          f"{own:.3g}; perm_max {got['perm_max'].tolist()}")
    assert worst <= own and worst_ls <= own


def test_refusals_leave_the_outputs_and_the_handle_as_they_were():
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    lib = _lib.load()
    case = (3, 33, 1, 65, cases.POINTS)
    D, Z, Y, _ = cases.build(case)
    Yc = np.ascontiguousarray(Y)
    perm_max, index = np.full((65, 4), -1.0), np.full((4, 33), -7, dtype=np.int32)
    call = lambda h, P, y, B, mask=None: lib.gbrs_scan_permute(h, P, _lib.ptr(y), B, 5, _lib.ptr(mask), _lib.ptr(perm_max), _lib.ptr(index))
    untouched = lambda: (perm_max == -1.0).all() and (index == -7).all()
    scan = GenomeScan(3, case[4])
    scan.append(D)
    assert call(scan._h, 65, Yc, 4) == _lib.GBRS_ERR_INVALID and b"call gbrs_scan_prepare first" in lib.gbrs_last_error() and untouched()
    with pytest.raises(_lib.GbrsHipError, match="call gbrs_scan_prepare first"):
        scan.permute(Y, 4)
    scan.prepare(Z)
    want = scan.run(Y)
    assert call(scan._h, 65, Yc, 0) == _lib.GBRS_ERR_INVALID and b"at least 1 permutation, got 0" in lib.gbrs_last_error() and untouched()
    assert call(scan._h, 65, Yc, -2) == _lib.GBRS_ERR_INVALID and untouched()
    assert call(scan._h, 0, Yc, 4) == _lib.GBRS_ERR_INVALID and b"at least 1 phenotype, got 0" in lib.gbrs_last_error() and untouched()
    bad = Yc.copy()
    bad[30, 2] = np.nan
    assert call(scan._h, 65, bad, 4) == _lib.GBRS_ERR_INVALID and untouched()
    assert b"phenotype 2 holds a value that is not finite (sample 30)" in lib.gbrs_last_error()
    assert call(scan._h, 65, Yc, 4, np.zeros(3, dtype=np.uint8)) == _lib.GBRS_ERR_INVALID and untouched()
    assert b"selects no grid point" in lib.gbrs_last_error()
    assert call(None, 65, Yc, 4) == _lib.GBRS_ERR_INVALID and untouched()
    assert lib.gbrs_scan_permute(scan._h, 65, _lib.ptr(Yc), 4, 5, None, None, None) == _lib.GBRS_ERR_INVALID
    for n_perm in (0, -1):
        with pytest.raises(_lib.GbrsHipError, match="at least 1 permutation"):
            scan.permute(Y, n_perm)
    with pytest.raises(ValueError, match="phenotypes have shape"):
        scan.permute(Y[:-1], 4)
    raw = _lib.ScanPermInfo()
    assert lib.gbrs_scan_perm_info(scan._h, C.byref(raw)) == _lib.GBRS_OK and (raw.P, raw.B, raw.last_permute_ms) == (0, 0, 0.0)
    assert call(scan._h, 65, Yc, 4) == _lib.GBRS_OK and not untouched()
    np.testing.assert_array_equal(index, restate.permutations(5, 4, 33))
    np.testing.assert_array_equal(perm_max, scan.permute(Y, 4, seed=5)["perm_max"])
    again = scan.run(Y)
    for key in want:
        np.testing.assert_array_equal(again[key], want[key], err_msg=key)
    scan.close()


# ---- the commands --------------------------------------------------------------------------------------------------------

COMMAND = (3, 33, 1, 65, cases.POINTS)
COMMAND_CHROMS = ("1", "2", "X")
COMMAND_PHENO = 6


@pytest.fixture
def exported(tmp_path):
    """The cohort of COMMAND as `gbrs scan` reads it: a grid file, one dosage table per sample with every digit, a
    phenotype table of six phenotypes (the last one constant) and the dosage list."""
    D, _, Y, _ = cases.build(COMMAND)
    rng = np.random.default_rng(44)
    points = {c: np.sort(rng.uniform(1.0, 90.0, size=m)) for c, m in zip(COMMAND_CHROMS, COMMAND[4])}
    paths = {"grid": grid_cases.write_grid_file(tmp_path / "grid.txt", points), "ids": [f"mouse{s}" for s in range(len(D))]}
    lines = []
    for s, sample_id in enumerate(paths["ids"]):
        with open(tmp_path / f"{sample_id}.tsv", "w") as fh:
            fh.write("# A\tB\tC\n")
            for row in D[s]:
                fh.write("\t".join(repr(float(v)) for v in row) + "\n")
        lines.append(f"{sample_id}\t{tmp_path / f'{sample_id}.tsv'}\n")
    (tmp_path / "list.tsv").write_text("".join(lines))
    paths["list"] = str(tmp_path / "list.tsv")
    values = np.array(Y[:, :COMMAND_PHENO])
    values[:, -1] = 2.5
    paths["names"] = [f"trait{p}" for p in range(COMMAND_PHENO)]
    paths["values"] = values
    paths["pheno"] = write_table(tmp_path / "pheno.tsv", paths["ids"], paths["names"], values)
    paths["pos"] = np.concatenate([points[c] for c in COMMAND_CHROMS])
    return paths


def by_hand(exported):
    from gbrs_amd.scan import GenomeScan
    D = cases.build(COMMAND)[0]
    scan = GenomeScan(3, COMMAND[4])
    scan.append(D)
    scan.prepare()
    return scan


def test_gbrs_scan_with_permutations(tmp_path, exported, monkeypatch):
    """`gbrs scan --scan-perms 20` on chromosomes 2 and X for three of the six phenotypes: the .npz holds what
    GenomeScan.permute and the two host functions give, the peaks file's two columns agree with them and hold NA for the
    other phenotypes and for chromosome 1; the stage times name the pass.  Unknown names are refused and write nothing."""
    from gbrs_amd import cli
    from gbrs_amd.scan import perm_pvalues, perm_thresholds
    (tmp_path / "permute.txt").write_text("trait4\ntrait0\n\ntrait5\n")
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(tmp_path / "stages.json"))
    base = ["scan", "--dosage-list", exported["list"], "--grid-file", exported["grid"], "--pheno", exported["pheno"]]
    assert cli.main(base + ["--scan-out", str(tmp_path / "out"), "--scan-perms", "20", "--scan-perm-seed", str(restate.SEED_HIGH),
                            "--scan-perm-chromosomes", "2,X", "--scan-perm-alpha", "0.1,0.25",
                            "--scan-perm-pheno", str(tmp_path / "permute.txt")]) == 0
    stages = json.load(open(tmp_path / "stages.json"))
    assert "error" not in stages and stages["scan_perm"] > 0
    columns, mask = [0, 4, 5], np.array([False, True, True])
    scan = by_hand(exported)
    want = scan.run(exported["values"])
    perm_max = scan.permute(exported["values"][:, columns], 20, seed=restate.SEED_HIGH, chromosomes=mask)["perm_max"]
    scan.close()
    z = np.load(tmp_path / "out.scan.npz")
    for key in ("lod", "peak_lod", "peak_index"):
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    np.testing.assert_array_equal(z["perm_max"], perm_max)
    assert (z["perm_max"][2] == 0.0).all()                                           # the constant phenotype
    assert z["perm_phenotypes"].tolist() == ["trait0", "trait4", "trait5"] and z["perm_chromosomes"].tolist() == ["2", "X"]
    assert z["perm_seed"] == restate.SEED_HIGH and z["perm_alpha"].tolist() == [0.1, 0.25]
    threshold = perm_thresholds(perm_max, [0.1, 0.25])
    np.testing.assert_array_equal(z["perm_threshold"], threshold)
    np.testing.assert_array_equal(threshold[:, 0], np.sort(perm_max, axis=1)[:, 17])  # the 18th smallest of 20
    pvalue = perm_pvalues(perm_max, want["peak_lod"][columns], selected=mask)
    lines = open(tmp_path / "out.scan.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tpvalue\tthreshold_0.1"
    rows = [line.split("\t") for line in lines[1:]]
    assert len(rows) == COMMAND_PHENO * 3
    for k, row in enumerate(rows):
        p, c = divmod(k, 3)
        assert row[:2] == [f"trait{p}", COMMAND_CHROMS[c]] and float(row[3]) == want["peak_lod"][p, c]
        if p in columns and mask[c]:
            assert float(row[5]) == pvalue[columns.index(p), c] and float(row[6]) == threshold[columns.index(p), 0]
            assert 1 / 21 <= float(row[5]) <= 1.0
        else:
            assert row[5:] == ["NA", "NA"]
    for extra, message in ((["--scan-perm-chromosomes", "2,Y"], "Y is no chromosome of the grid"),
                           (["--scan-perm-alpha", "0.05,1"], "every level must lie in (0, 1)"),
                           (["--scan-perm-seed", "3"], "--scan-perm-seed needs --scan-perms")):
        perms = [] if "needs" in message else ["--scan-perms", "5"]
        assert cli.main(base + ["--scan-out", str(tmp_path / "refused")] + perms + extra) == 0
        assert message in json.load(open(tmp_path / "stages.json"))["error"]
    (tmp_path / "permute.txt").write_text("trait9\n")
    assert cli.main(base + ["--scan-out", str(tmp_path / "refused"), "--scan-perms", "5", "--scan-perm-pheno", str(tmp_path / "permute.txt")]) == 0
    assert "trait9 is no phenotype of the table" in json.load(open(tmp_path / "stages.json"))["error"]
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused")]


def test_gbrs_scan_without_permutations_writes_what_it_wrote_before(tmp_path, exported, monkeypatch):
    """The command without `--scan-perms`: the peaks file is, byte for byte, the text put together here from
    GenomeScan.run in the format the files had before the permutations existed, and the .npz holds the same entries in
    the same order with the same bits (its bytes carry the archive's time stamps, so they are not compared); the stage
    times name no permutation pass."""
    from gbrs_amd import cli
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(tmp_path / "stages.json"))
    assert cli.main(["scan", "--dosage-list", exported["list"], "--grid-file", exported["grid"], "--pheno", exported["pheno"],
                     "--scan-out", str(tmp_path / "plain")]) == 0
    stages = json.load(open(tmp_path / "stages.json"))
    assert "error" not in stages and "scan_perm" not in stages
    scan = by_hand(exported)
    want = scan.run(exported["values"])
    rank = scan.info()["rank"]
    scan.close()
    text = "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\n"
    for p, name in enumerate(exported["names"]):
        top = max(range(3), key=lambda c: (want["peak_lod"][p, c], -c))
        for c in range(3):
            text += (f"{name}\t{COMMAND_CHROMS[c]}\t{repr(float(exported['pos'][want['peak_index'][p, c]]))}\t"
                     f"{repr(float(want['peak_lod'][p, c]))}\t{int(c == top)}\n")
    assert open(tmp_path / "plain.scan.peaks.tsv", "rb").read() == text.encode()
    z = np.load(tmp_path / "plain.scan.npz")
    assert z.files == ["phenotypes", "samples", "covariates", "chrom", "pos", "rank", "peak_lod", "peak_index", "lod"]
    expected = dict(phenotypes=np.array(exported["names"]), samples=np.array(exported["ids"]), covariates=np.array(["intercept"]),
                    chrom=np.repeat(COMMAND_CHROMS, COMMAND[4]), pos=exported["pos"], rank=rank, peak_lod=want["peak_lod"],
                    peak_index=want["peak_index"], lod=want["lod"])
    for key, value in expected.items():
        assert z[key].dtype == value.dtype and z[key].shape == value.shape, key
        np.testing.assert_array_equal(z[key], value, err_msg=key)


def test_reconstruct_with_scan_perms(tmp_path, monkeypatch):
    """Twelve samples of the eight-founder "do" family on grid "a" (its chromosome X holds no grid point) through
    `reconstruct --sample-file ... --scan-pheno ... --scan-perms 5`: the files hold the permutation results of the scan's
    own phenotypes, consistent with the host functions, and the stage times name the pass apart from the scan."""
    from gbrs_amd import cli
    from gbrs_amd.scan import perm_pvalues, perm_thresholds
    H, style, n = 8, "do", 12
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(tmp_path / "stages.json"))
    p0 = grid_cases.problem(H, style)
    grid = grid_cases.grids()["a"]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    grid_file = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    lines, outbases = [], [str(tmp_path / f"do{s}") for s in range(n)]
    for s in range(n):
        tpm = grid_cases.write_genes_tpm(tmp_path / f"s{s}.genes.tpm", grid_cases.sample_problem(H, style, s))
        lines.append(f"{tpm}\t{outbases[s]}")
    (tmp_path / "samples.txt").write_text("\n".join(lines) + "\n")
    pheno = write_table(tmp_path / "pheno.tsv", outbases, ["a", "b", "c"], np.random.default_rng(77).normal(size=(n, 3)))
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "-t", paths["tprob"], "-x", paths["avecs"],
                     "-g", paths["gpos"], "--grid-file", grid_file, "--scan-pheno", pheno, "--scan-out", str(tmp_path / "cohort"),
                     "--scan-perms", "5"]) == 0
    stages = json.load(open(tmp_path / "stages.json"))
    assert "error" not in stages and stages["scan_perm"] > 0 and stages["scan"] > 0
    z = np.load(tmp_path / "cohort.scan.npz")
    chroms = [c for c in p0.chroms]
    assert z["perm_max"].shape == (3, 5) and np.isfinite(z["perm_max"]).all() and (z["perm_max"] > 0).all()
    assert z["perm_phenotypes"].tolist() == ["a", "b", "c"] and z["perm_chromosomes"].tolist() == chroms and z["perm_seed"] == 0
    assert z["perm_alpha"].tolist() == [0.05, 0.1]
    np.testing.assert_array_equal(z["perm_threshold"], perm_thresholds(z["perm_max"], [0.05, 0.1]))
    np.testing.assert_array_equal(z["perm_threshold"][:, 0], z["perm_max"].max(axis=1))
    pvalue = perm_pvalues(z["perm_max"], z["peak_lod"])
    assert np.isnan(pvalue[:, -1]).all() and np.isnan(z["peak_lod"][:, -1]).all()       # X is off the grid
    lines = open(tmp_path / "cohort.scan.peaks.tsv").read().splitlines()
    assert lines[0].endswith("\tgenome_wide_max\tpvalue\tthreshold_0.05")
    rows = [line.split("\t") for line in lines[1:]]
    assert len(rows) == 3 * (len(chroms) - 1)
    for row in rows:
        p, c = "abc".index(row[0]), chroms.index(row[1])
        assert float(row[5]) == pvalue[p, c] and float(row[6]) == z["perm_threshold"][p, 0]
