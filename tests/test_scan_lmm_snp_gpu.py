"""SNP association under the mixed model on the device (gbrs_scan_lmm_snps, GenomeScan.run_snps_lmm; needs
an MI355X) against the two host routes of tests/scan_lmm_snp_cases.py, each fed the device's own heritabilities, at ten
times each case's recorded figure; `used`, `n_used` and the peaks exactly; the bit equalities, the refusals, the other entry
points before and after a call, and both commands."""
import functools
import os

import numpy as np
import pytest

import grid_cases
import scan_lmm_cases as lmm
import scan_lmm_snp_cases as cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401
from test_scan_lmm_gpu import kinship_argument, open_scan, write_cohort
from test_scan_snp_commands_gpu import write_snp_file

pytestmark = pytest.mark.gpu

BITS = cases.CASES[1]                      # H8-n70-c2-P65: the case of the bit equalities
SMALL = cases.CASES[0]                     # H8-n33-c2-P63: the 33-sample cohort of the chunk crossing
KEYS = ("lod", "used", "peak_lod", "peak_index", "n_used", "hsq", "sigma2")


def scan_of(case, snps=None, split=None):
    """The case's cohort with the mixed model prepared and a SNP set (default: the main set) on the handle."""
    scan = open_scan(case, split)
    scan.prepare_lmm(lmm.build(case)[1], kinship_argument(case))
    grid, pos, masks, _ = snps if snps is not None else cases.snp_set(case)
    scan.set_snps(grid, pos, masks)
    return scan


@functools.lru_cache(maxsize=None)
def device(case):
    """run_snps_lmm's dict of a case's main set and its phenotypes, computed once."""
    scan = scan_of(case)
    got = scan.run_snps_lmm(cases.phenotypes(case))
    info = scan.lmm_snp_info()
    scan.close()
    P, M_snp = cases.phenotypes(case).shape[1], sum(len(x) for x in cases.snp_set(case)[1])
    assert (info["M_snp"], info["P"]) == (M_snp, P) and info["chunk"] >= 64 and info["chunk"] % 64 == 0
    assert info["pass_ms"] >= info["null_ms"] > 0 and info["rotate_ms"] > 0 and info["product_ms"] > 0
    assert info["peak_device_bytes"] > info["column_bytes"] >= 8 * (case[2] + 2) * case[1] * P
    for a in got.values():
        a.setflags(write=False)
    return got


def same(a, b, keys=KEYS, rows=slice(None), note=""):
    for key in keys:
        np.testing.assert_array_equal(a[key][rows], b[key], err_msg=f"{key} {note}")


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_the_device_against_both_host_routes_at_its_own_heritabilities(case):
    """LODs within DEVICE_FACTOR x the case's recorded figure of the restatement and of dense GLS; `used` equal to the
    restatement's and to lstsq's rank; n_used and the peaks exactly those of the device's own LODs and flags; unused pairs
    and the flat SNPs score exactly 0.0; the main set in descending order gives every SNP the same bits."""
    D, Z, _, kinships, kin_of_chrom, _ = lmm.build(case)
    Y = cases.phenotypes(case)
    X, counts = cases.dosages(case)
    got = device(case)
    P, M_snp, nc = Y.shape[1], X.shape[1], len(case[4])
    assert got["lod"].shape == got["used"].shape == (P, M_snp)
    assert got["peak_lod"].shape == got["peak_index"].shape == got["n_used"].shape == got["hsq"].shape == (P, nc)
    hsq = cases.per_decomposition(case, got["hsq"])
    np.testing.assert_array_equal(got["hsq"], hsq[:, list(kin_of_chrom)])
    rule = cases.snp_lmm_rule(X, counts, Z, Y, lmm.decompositions(case), kin_of_chrom, hsq=hsq)
    gls, rank = cases.snp_lmm_gls(X, counts, Z, Y, kinships, kin_of_chrom, hsq)
    cases.check_ratios(rule, rank)
    for name, want in (("rule", rule["lod"]), ("gls", gls)):
        measured = cases.deviation(got["lod"], want)
        print(f"DEVIATION device SNP LODs under the mixed model against {name}: {measured:.3g}, tolerance "
              f"{cases.device_tol(case):.3g}, {cases.case_id(case)}")
        assert measured <= cases.device_tol(case), name
    np.testing.assert_array_equal(got["used"], rule["used"])
    np.testing.assert_array_equal(got["used"], rank == 1)
    assert (got["lod"] >= 0.0).all() and (got["lod"][~got["used"]] == 0.0).all()
    flat = cases.flat_snps(case)
    assert len(flat) >= 2 and not got["used"][:, flat].any()
    peak, index, count = cases.snp_lmm_peaks(got["lod"], got["used"], counts)
    np.testing.assert_array_equal(got["peak_index"], index)
    np.testing.assert_array_equal(got["peak_lod"], peak)
    np.testing.assert_array_equal(got["n_used"], count)
    np.testing.assert_array_equal(got["n_used"], cases.snp_lmm_peaks(rule["lod"], rule["used"], counts)[2])
    labels = cases.snp_set(case)[3]
    flipped = cases.snp_set(case, "descending")
    back = scan_of(case, snps=flipped)
    turned = back.run_snps_lmm(Y)
    back.close()
    np.testing.assert_array_equal(turned["hsq"], got["hsq"])
    for j, label in enumerate(labels):                     # the same SNP, another place: the same bits
        if labels.count(label) == 1:
            k = flipped[3].index(label)
            assert np.array_equal(turned["lod"][:, k], got["lod"][:, j]) and np.array_equal(turned["used"][:, k], got["used"][:, j]), label


def test_a_snp_has_the_same_bits_alone_and_around_the_row_tile():
    """SNP 77 of 130 on one chromosome, set alone and at the last row of sets of 63, 64 and 65 and among the 130; a second
    run; without the LOD matrix."""
    Y = cases.phenotypes(BITS)
    grid, pos, masks, _ = cases.snp_set(BITS, "sized", 130)
    scan = scan_of(BITS, snps=(grid, pos, masks, None))
    full = scan.run_snps_lmm(Y)
    same(scan.run_snps_lmm(Y), full, note="of a second run")
    lean = scan.run_snps_lmm(Y, want_lod=False)
    assert "lod" not in lean and "used" not in lean
    same(lean, full, keys=("peak_lod", "peak_index", "n_used", "hsq", "sigma2"), note="without the LOD matrix")
    assert (full["peak_index"][:, [0, 2]] == -1).all() and np.isnan(full["peak_lod"][:, [0, 2]]).all() and (full["n_used"][:, [0, 2]] == 0).all()
    chosen = 77
    for place, total in ((0, 1), (62, 63), (63, 64), (64, 65), (0, 65)):
        x, m = pos[1][:total].copy(), masks[1][:total].copy()
        x[place], m[place] = pos[1][chosen], masks[1][chosen]
        scan.set_snps(grid, [None, x, None], [None, m, None])                      # set_snps keeps the preparation
        moved = scan.run_snps_lmm(Y)
        assert np.array_equal(moved["lod"][:, place], full["lod"][:, chosen]), (place, total)
        assert np.array_equal(moved["used"][:, place], full["used"][:, chosen]), (place, total)
        others = [k for k in range(total) if k != place]
        assert np.array_equal(moved["lod"][:, others], full["lod"][:, others]), (place, total)
    scan.close()


def test_the_snp_chunk_boundary():
    """65,536 + 65 SNPs on the 33-sample cohort, the chunk's end inside the second chromosome and the third chromosome's
    first SNP in the middle of a row tile: the SNPs around the chunk's end and those at both ends have the bits they have
    as short sets, and the peaks carried across the chunks are those of the whole LOD rows."""
    case = SMALL
    Y = np.ascontiguousarray(cases.phenotypes(case)[:, [0, 3, 64]])
    grid = cases.snp_set(case)[0]
    scan = scan_of(case)
    L = scan.lmm_snp_info()["chunk"]
    assert L == 65536
    rng = np.random.default_rng(33)
    counts = [100, L - 86, 51]
    assert sum(counts) == L + 65
    pos = [np.sort(rng.uniform(g[0] - 1.0, g[-1] + 1.0, size=k)) for g, k in zip(grid, counts)]
    masks = [rng.integers(1, 255, size=k).astype(np.uint32) for k in counts]
    scan.set_snps(grid, pos, masks)
    full = scan.run_snps_lmm(Y)
    assert full["lod"].shape == (3, L + 65)
    peak, index, count = cases.snp_lmm_peaks(full["lod"], full["used"], counts)
    np.testing.assert_array_equal(full["peak_index"], index)
    np.testing.assert_array_equal(full["peak_lod"], peak)
    np.testing.assert_array_equal(full["n_used"], count)
    none, no_mask = np.zeros(0), np.zeros(0, dtype=np.uint32)
    windows = (([pos[0], pos[1][:100], none], [masks[0], masks[1][:100], no_mask], 0),
               ([none, pos[1][-114:], pos[2]], [no_mask, masks[1][-114:], masks[2]], L - 100),
               ([none, pos[1][L - 300:L - 90], none], [no_mask, masks[1][L - 300:L - 90], no_mask], L - 200))
    for x, m, first in windows:
        scan.set_snps(grid, x, m)
        short = scan.run_snps_lmm(Y)
        width = short["lod"].shape[1]
        np.testing.assert_array_equal(full["lod"][:, first:first + width], short["lod"], err_msg=str(first))
        np.testing.assert_array_equal(full["used"][:, first:first + width], short["used"], err_msg=str(first))
    scan.close()
    X, cs = cases.dosages(case, (grid, [none, pos[1][-114:], pos[2]], [no_mask, masks[1][-114:], masks[2]], None))
    rule = cases.snp_lmm_rule(X, cs, lmm.build(case)[1], Y, lmm.decompositions(case), lmm.build(case)[4],
                              hsq=cases.per_decomposition(case, full["hsq"]))
    assert cases.deviation(full["lod"][:, L - 100:], rule["lod"]) <= cases.device_tol(case)
    np.testing.assert_array_equal(full["used"][:, L - 100:], rule["used"])


def test_a_phenotype_has_the_same_bits_alone_at_any_column_and_in_any_chunk():
    Y = cases.phenotypes(BITS)[:, :65]
    scan = scan_of(BITS)
    full = scan.run_snps_lmm(Y)
    same(full, {k: v[:65] for k, v in device(BITS).items()}, note="of the first 65 of 69 columns")
    for p in (0, 17, 64):
        alone = scan.run_snps_lmm(Y[:, p])
        for key in KEYS:
            np.testing.assert_array_equal(alone[key][0], full[key][p], err_msg=f"{key} of column {p}")
    wide = np.tile(Y, (1, 8))[:, :513]                                              # column 512 is column 512 % 65
    given = np.random.default_rng(7).uniform(0.0, 1.0, size=(513, 3))
    far = scan.run_snps_lmm(wide, hsq=given)
    np.testing.assert_array_equal(far["hsq"], given)
    alone = scan.run_snps_lmm(wide[:, 512], hsq=given[512:513])
    scan.close()
    for key in KEYS:
        np.testing.assert_array_equal(alone[key][0], far[key][512], err_msg=f"{key} of column 512 of 513")
    assert (far["lod"][512] != full["lod"][512 % 65]).any()                         # another heritability, other LODs


def test_the_cohorts_appends_do_not_change_a_bit():
    Y = cases.phenotypes(BITS)[:, :9]
    scan = scan_of(BITS, split=lambda d: [d[:1], d[1:]])
    out = scan.run_snps_lmm(Y)
    scan.close()
    same(out, {k: v[:9] for k, v in device(BITS).items()}, note="appended as 1 + rest")


def test_the_heritabilities_of_the_grid_scan_handed_back():
    """run_lmm's hsq given to the SNP pass, as the commands do: the bits of the pass that fits them itself."""
    Y = cases.phenotypes(BITS)
    scan = scan_of(BITS)
    grid_scan = scan.run_lmm(Y, want_lod=False)
    handed = scan.run_snps_lmm(Y, hsq=grid_scan["hsq"])
    scan.close()
    same(handed, device(BITS), note="with run_lmm's heritabilities")


def test_refusals_leave_the_outputs_and_the_handle():
    from gbrs_amd import _lib
    case = cases.CASES[8]
    H, n, cz, P, points, _ = case
    Z = lmm.build(case)[1]
    Y = cases.phenotypes(case)
    P = Y.shape[1]
    M_snp = sum(len(x) for x in cases.snp_set(case)[1])
    lib = _lib.load()
    y = np.ascontiguousarray(lmm.centred(Y))
    outs = [np.full((P, M_snp), 7.0), np.full((P, M_snp), 7, dtype=np.uint8), np.full((P, 3), 7.0), np.full((P, 3), 7, dtype=np.int64),
            np.full((P, 3), 7, dtype=np.int64), np.full((P, 3), 7.0), np.full((P, 3), 7.0)]

    def call(scan, p=P, table=y, hsq_in=None):
        status = lib.gbrs_scan_lmm_snps(scan._h, p, _lib.ptr(table), _lib.ptr(hsq_in), *[_lib.ptr(a) for a in outs])
        text = lib.gbrs_last_error().decode()
        assert all((a == 7).all() for a in outs), text
        return status, text

    scan = open_scan(case)
    scan.prepare_lmm(Z)
    status, text = call(scan)
    assert status == _lib.GBRS_ERR_INVALID and "gbrs_scan_set_snps first" in text
    with pytest.raises(_lib.GbrsHipError, match="no SNPs on the handle"):
        scan.run_snps_lmm(Y)
    scan.close()
    scan = open_scan(case)
    scan.set_snps(*cases.snp_set(case)[:3])
    status, text = call(scan)
    assert status == _lib.GBRS_ERR_INVALID and "gbrs_scan_lmm_prepare first" in text
    with pytest.raises(_lib.GbrsHipError, match="prepare_lmm first"):
        scan.run_snps_lmm(Y)
    scan.prepare_lmm(Z)
    status, text = call(scan, p=0)
    assert status == _lib.GBRS_ERR_INVALID and "at least 1 phenotype" in text
    bad = np.where((np.arange(n)[:, None] == 4) & (np.arange(P) == 2), np.nan, y)
    status, text = call(scan, table=np.ascontiguousarray(bad))
    assert status == _lib.GBRS_ERR_INVALID and "phenotype 2 holds a value that is not finite (sample 4)" in text
    for value in (1.5, -0.25, np.nan):
        hsq_in = np.full((P, 3), 0.5)
        hsq_in[3, 1] = value
        status, text = call(scan, hsq_in=hsq_in)
        assert status == _lib.GBRS_ERR_INVALID and "phenotype 3 and decomposition 1" in text and "outside [0, 1]" in text
    with pytest.raises(ValueError, match="hsq has shape"):
        scan.run_snps_lmm(Y, hsq=np.zeros((P, 2)))
    same(scan.run_snps_lmm(Y), device(case), note="after the refusals")
    scan.append(lmm.build(case)[0][:2])                                             # an append drops the preparation, not the SNPs
    with pytest.raises(_lib.GbrsHipError, match="prepare_lmm first"):
        scan.run_snps_lmm(np.ones((n + 2, 1)))
    scan.close()


def test_the_other_entry_points_give_the_same_bits_before_and_after():
    case = SMALL
    D, Z, _, _, _, _ = lmm.build(case)
    Y = cases.phenotypes(case)
    scan = scan_of(case)
    scan.prepare(Z)
    before = (scan.run(Y), scan.run_snps(Y), scan.run_lmm(Y))
    info = (scan.info(), scan.snp_info()["device_bytes"], scan.lmm_info()["device_bytes"])
    got = scan.run_snps_lmm(Y)
    after = (scan.run(Y), scan.run_snps(Y), scan.run_lmm(Y))
    assert scan.info()["device_bytes"] == info[0]["device_bytes"] and scan.snp_info()["device_bytes"] == info[1]
    assert scan.lmm_info()["device_bytes"] == info[2]
    again = scan.run_snps_lmm(Y)
    scan.close()
    for a, b in zip(before, after):
        assert sorted(a) == sorted(b)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    same(got, device(case), note="beside the other passes")
    same(again, device(case), note="after the other passes")
    # under zero heritability the weights are 1 and the model is §29's: dense GLS at h = 0 is least squares on [Z | x], and
    # `used` is run_snps' for every phenotype
    zero = scan_of(case)
    flat = zero.run_snps_lmm(Y, hsq=np.zeros((Y.shape[1], 3)))
    zero.close()
    X, counts = cases.dosages(case)
    gls = cases.snp_lmm_gls(X, counts, Z, Y, lmm.build(case)[3], lmm.build(case)[4], np.zeros((Y.shape[1], 3)))[0]
    assert cases.deviation(flat["lod"], gls) <= cases.device_tol(case)
    np.testing.assert_array_equal(flat["used"], np.broadcast_to(before[1]["used"], flat["used"].shape))


# ---- the commands ----------------------------------------------------------------------------------------------------------

def write_case_snps(path, case, chrom_names, pos_of_grid):
    """The case's main SNP set as a SNP file on write_cohort's grid positions (the main set's positions are rescaled to
    the command's grid), the lines shuffled, three SNPs on a chromosome nobody has."""
    H = case[0]
    rng = np.random.default_rng(5)
    rows = []
    for c, g in zip(chrom_names, pos_of_grid):
        for k, x in enumerate(rng.uniform(g[0] - 0.5, g[-1] + 0.5, size=9)):
            pattern = "".join(rng.choice(["0", "1"], size=H)) if k else "1" * H
            rows.append((f"snp_{c}_{k}", c, 1000 * (k + 1), repr(float(x)), pattern))
    rows += [(f"snp_far_{k}", "Zz", 5 * k, "1.5", "1" + "0" * (H - 1)) for k in range(3)]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    with open(path, "w") as fh:
        fh.write("id\tchr\tbp\tcM\tpattern\n")
        for r in rows:
            fh.write("\t".join(str(v) for v in r) + "\n")
    return str(path), rows


def test_gbrs_scan_with_kinship_snps(tmp_path, caplog):
    """`gbrs scan --scan-kinship loco --scan-kinship-snps FILE`: the scan's files are what they are without the option,
    byte for byte; the SNP files hold run_snps_lmm at run_lmm's heritabilities, in the file's order."""
    from gbrs_amd import cli
    case = cases.CASES[8]
    D, Z, Y, _, _, _ = lmm.build(case)
    points = case[4]
    command, ids, names, chrom_names, pos = write_cohort(tmp_path, case)
    off = np.concatenate(([0], np.cumsum(points)))
    grids = [pos[a:b] for a, b in zip(off[:-1], off[1:])]
    snp_file, rows = write_case_snps(tmp_path / "snps.tsv", case, chrom_names, grids)
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(command + ["--scan-out", str(tmp_path / "with"), "--scan-kinship", "loco", "--scan-kinship-snps", snp_file,
                                   "--scan-min-lod", "0.05"]) == 0
        assert cli.main(command + ["--scan-out", str(tmp_path / "plain"), "--scan-kinship", "loco", "--scan-min-lod", "0.05"]) == 0
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("with.")) == ["with.scan.npz", "with.scan.peaks.tsv", "with.scan.snps.npz",
                                                                               "with.scan.snps.peaks.tsv"]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("plain.")) == ["plain.scan.npz", "plain.scan.peaks.tsv"]
    assert open(tmp_path / "with.scan.peaks.tsv", "rb").read() == open(tmp_path / "plain.scan.peaks.tsv", "rb").read()
    a, b = np.load(tmp_path / "with.scan.npz"), np.load(tmp_path / "plain.scan.npz")
    assert a.files == b.files
    for key in b.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    chrom = np.array([r[1] for r in rows])
    by = [np.flatnonzero(chrom == c) for c in chrom_names]
    order = np.concatenate(by)
    mask = np.array([sum(1 << h for h, ch in enumerate(r[4]) if ch == "1") for r in rows], dtype=np.uint32)
    cm = np.array([float(r[3]) for r in rows])
    scan = open_scan(case)
    scan.prepare_lmm(Z)
    grid_scan = scan.run_lmm(Y)
    scan.set_snps(grids, [cm[k] for k in by], [mask[k] for k in by])
    want = scan.run_snps_lmm(Y, hsq=grid_scan["hsq"])
    scan.close()
    z = np.load(tmp_path / "with.scan.snps.npz")
    assert sorted(z.files) == sorted(["phenotypes", "samples", "covariates", "snp_id", "chrom", "bp", "cM", "pattern", "used", "peak_lod",
                                      "peak_snp", "lod", "hsq", "n_used", "kinship_mode"])
    assert z["snp_id"].tolist() == [r[0] for r in rows] and str(z["kinship_mode"]) == "loco" and z["samples"].tolist() == ids
    foreign = np.setdiff1d(np.arange(len(rows)), order)
    assert len(foreign) == 3 and np.isnan(z["lod"][:, foreign]).all() and not z["used"][:, foreign].any()
    np.testing.assert_array_equal(z["lod"][:, order], want["lod"])
    np.testing.assert_array_equal(z["used"][:, order], want["used"])
    np.testing.assert_array_equal(z["peak_lod"], want["peak_lod"])
    np.testing.assert_array_equal(z["n_used"], want["n_used"])
    np.testing.assert_array_equal(z["hsq"], grid_scan["hsq"])
    np.testing.assert_array_equal(z["peak_snp"], np.where(want["peak_index"] >= 0, order[np.maximum(want["peak_index"], 0)], -1))
    assert (z["n_used"] >= 7).all() and (z["n_used"] <= 9).all()                    # the all-ones SNP is flat where the rows add up to 1
    # without the option: byte for byte what write_scan makes of run_lmm, the scan as it was
    from gbrs_amd.scan import write_scan
    write_scan(str(tmp_path / "hand"), names, ids, ["intercept", "sex"], np.repeat(chrom_names, points), pos, chrom_names, grid_scan, None,
               0.05, kinship_mode="loco")
    assert open(tmp_path / "plain.scan.peaks.tsv", "rb").read() == open(tmp_path / "hand.scan.peaks.tsv", "rb").read()
    hand = np.load(tmp_path / "hand.scan.npz")
    assert hand.files == b.files
    for key in b.files:
        assert hand[key].dtype == b[key].dtype and hand[key].tobytes() == b[key].tobytes(), key
    lines = open(tmp_path / "with.scan.snps.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max\thsq"
    table = [line.split("\t") for line in lines[1:]]
    expected = [(p, ci) for p in range(len(names)) for ci in range(3) if want["peak_lod"][p, ci] >= 0.05]
    assert len(table) == len(expected) > 0
    for fields, (p, ci) in zip(table, expected):
        j = z["peak_snp"][p, ci]
        assert fields[:3] == [names[p], chrom_names[ci], rows[j][0]] and float(fields[6]) == want["peak_lod"][p, ci]
        assert float(fields[8]) == grid_scan["hsq"][p, ci]
    # the option without the kinship is refused before a file is read, and --scan-snps stays refused beside the kinship
    caplog.clear()
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(command + ["--scan-out", str(tmp_path / "refused"), "--scan-kinship-snps", snp_file])
        cli.main(command + ["--scan-out", str(tmp_path / "refused"), "--scan-kinship", "loco", "--snp-file", snp_file])
    messages = [r.getMessage() for r in caplog.records]
    assert any("--scan-kinship-snps needs --scan-kinship" in m for m in messages)
    assert any("--scan-snps cannot be combined with --scan-kinship" in m for m in messages)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused.")]


def test_gbrs_reconstruct_with_kinship_snps(tmp_path, tables, caplog, monkeypatch):
    """`gbrs reconstruct --scan-pheno --scan-kinship overall --scan-kinship-snps FILE` on six samples: the SNP files hold
    run_snps_lmm driven by hand on the dosages that went through the handle; without the option every file of the run is
    byte for byte what it is with it, and there are no SNP files."""
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
    rng = np.random.default_rng(33)
    names = [f"gene{p}" for p in range(4)]
    values = rng.normal(size=(N_FILES, 4))
    ids = lambda stem: [str(tmp_path / f"{stem}{s}") for s in range(N_FILES)]
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    snp_file, rows = write_snp_file(tmp_path / "snps.tsv", grid_b.points, grid_b.positions, rng)
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]

    def reconstruct(stem, extra):
        sample_file = cohort_files(tmp_path, stem)
        pheno = write_table(tmp_path / f"{stem}.pheno.tsv", ids(stem), names, values)
        return cli.main(["reconstruct", "--sample-file", sample_file] + common +
                        ["--scan-pheno", pheno, "--scan-out", str(tmp_path / stem), "--scan-kinship", "overall", "--scan-lod-matrix"] + extra)

    with caplog.at_level("ERROR", logger="gbrs"):
        assert reconstruct("with", ["--scan-kinship-snps", snp_file]) == 0
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    first = len(seen)
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    assert reconstruct("plain", []) == 0
    assert len(seen) == 2 * first
    assert not [f for f in os.listdir(tmp_path) if f.startswith("plain.scan.snps")]
    made = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain") and not f.startswith("plain.pheno") and f != "plain.txt")
    assert made == sorted(f[len("with"):] for f in os.listdir(tmp_path)
                          if f.startswith("with") and not f.startswith(("with.pheno", "with.scan.snps")) and f != "with.txt")
    assert open(tmp_path / "with.scan.peaks.tsv", "rb").read() == open(tmp_path / "plain.scan.peaks.tsv", "rb").read()
    a, b = np.load(tmp_path / "with.scan.npz"), np.load(tmp_path / "plain.scan.npz")
    assert a.files == b.files
    for key in a.files:
        if key != "samples":                                                        # the outbases carry the stem
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    for s in range(N_FILES):
        for tail in [f for f in made if f.startswith(str(s))]:
            if tail.endswith(".npz"):                                               # a zip archive carries its members' times
                fa, fb = np.load(tmp_path / f"with{tail}"), np.load(tmp_path / f"plain{tail}")
                assert fa.files == fb.files
                for key in fa.files:
                    assert fa[key].dtype == fb[key].dtype and fa[key].tobytes() == fb[key].tobytes(), (tail, key)
                continue
            with open(tmp_path / f"with{tail}", "rb") as fa, open(tmp_path / f"plain{tail}", "rb") as fb:
                assert fa.read() == fb.read(), tail
    chrom = np.array([r[1] for r in rows])
    by = [np.flatnonzero(chrom == c) if m else np.zeros(0, dtype=int) for c, m in zip(p0.chroms, points)]
    order = np.concatenate(by)
    mask = np.array([sum(1 << h for h, ch in enumerate(r[4]) if ch == "1") for r in rows], dtype=np.uint32)
    z = np.load(tmp_path / "with.scan.snps.npz")
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare_lmm(None, "overall")
    grid_scan = scan.run_lmm(values)
    scan.set_snps([grid_b.points[c] if m else None for c, m in zip(p0.chroms, points)], [z["cM"][k] for k in by], [mask[k] for k in by])
    want = scan.run_snps_lmm(values, hsq=grid_scan["hsq"])
    scan.close()
    assert z["snp_id"].tolist() == [r[0] for r in rows] and str(z["kinship_mode"]) == "overall" and z["samples"].tolist() == ids("with")
    np.testing.assert_array_equal(z["lod"][:, order], want["lod"])
    np.testing.assert_array_equal(z["used"][:, order], want["used"])
    np.testing.assert_array_equal(z["peak_lod"], want["peak_lod"])
    np.testing.assert_array_equal(z["n_used"], want["n_used"])
    np.testing.assert_array_equal(z["hsq"], grid_scan["hsq"])
    np.testing.assert_array_equal(a["hsq"], grid_scan["hsq"])
    assert want["used"].any() and os.path.getsize(tmp_path / "with.scan.snps.peaks.tsv") > 0
    caplog.clear()
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common +
                 ["--scan-pheno", str(tmp_path / "with.pheno.tsv"), "--scan-kinship-snps", snp_file])
    assert any("--scan-kinship-snps needs --scan-kinship" in r.getMessage() for r in caplog.records)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]
