"""The three host computations the SNP association scan is held against (tests/scan_snp_cases.py): no GPU."""
import numpy as np
import pytest

import scan_cases as base
import scan_snp_cases as cases


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_the_rule_agrees_with_lstsq(case):
    """snp_rule against np.linalg.lstsq, which knows nothing of it: the LODs within the case's measured figure (with
    headroom), `used` equal to lstsq's rank; the all-zeros and the all-ones pattern are unused with LOD exactly 0.0; a
    pattern and its complement share the flag and, within the bound, the LODs."""
    X, lod, used, _, lod_ls, rank = cases.expected(case)
    labels = cases.main_set(case)[3]
    worst = cases.deviation(lod, lod_ls)
    print(f"DEVIATION snp_rule against snp_lstsq, {cases.case_id(case)}: {worst:.3g}, largest LOD {lod[np.isfinite(lod)].max():.3g}")
    assert worst <= cases.cpu_bound(case)
    np.testing.assert_array_equal(used, rank == 1)
    flat = cases.flat_snps(case)
    assert len(flat) >= 3                  # both on the second chromosome, and the all-zeros pattern on the third
    assert not used[flat].any() and (lod[:, flat] == 0.0).all()
    pairs = cases.complement_pairs(case)
    assert pairs
    for a, b in pairs:                     # two computations, each with its own rounding: twice the bound
        assert used[a] == used[b]
        assert cases.deviation(lod[:, a], lod[:, b]) <= 2 * cases.cpu_bound(case)


def test_the_direct_cohort_on_the_host():
    """The cohort past the LDS (scan_snp_cases.DIRECT): the two host routes within its own measured figure, `used` equal to
    lstsq's rank, no undecided ratio."""
    _, lod, used, ratio, lod_ls, rank = cases.expected(cases.DIRECT)
    worst = cases.deviation(lod, lod_ls)
    print(f"DEVIATION snp_rule against snp_lstsq, {cases.case_id(cases.DIRECT)}: {worst:.3g}")
    assert 2 * cases.DIRECT[0] * cases.DIRECT[1] * 8 > 160 * 1024
    assert worst <= cases.cpu_bound(cases.DIRECT)
    np.testing.assert_array_equal(used, rank == 1)
    with np.errstate(invalid="ignore"):
        assert not ((ratio >= cases.UNDECIDED[0]) & (ratio <= cases.UNDECIDED[1])).any()


def test_no_fixture_has_an_undecided_ratio():
    """A ratio G / raw in [1e-13, 1e-7] could flip `used` by rounding: no SNP of any main set has one."""
    lo, hi = cases.UNDECIDED
    smallest_kept, largest_skipped, total = np.inf, 0.0, 0
    for case in cases.ALL_CASES:
        _, _, used, ratio, _, _ = cases.expected(case)
        with np.errstate(invalid="ignore"):
            assert not ((ratio >= lo) & (ratio <= hi)).any(), cases.case_id(case)
        total += len(used)
        smallest_kept = min(smallest_kept, ratio[used].min())
        largest_skipped = max(largest_skipped, np.nanmax(ratio[~used], initial=0.0))
    print(f"ratios G / raw over {total} SNPs: smallest kept {smallest_kept:.3g}, largest skipped {largest_skipped:.3g}")
    assert smallest_kept > hi and largest_skipped < lo


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_the_dosage_rule_agrees_with_interp(case):
    """The rule's dosages against 2 sum_h bit_h np.interp(x, g, D[s, :, h]) within (4 H + 24) 2^-53 of the largest value, 2
    (DESIGN.md §29 counts the roundings); clamped SNPs take the end point's dosage exactly."""
    H, points = case[0], case[4]
    D = base.build(case)[0]
    grid, pos, masks, labels = cases.main_set(case)
    X = cases.expected(case)[0]
    worst = np.abs(X - cases.snp_dosage_interp(D, points, grid, pos, masks)).max()
    bound = 2.0 * (4 * H + 24) * 2.0 ** -53
    print(f"DEVIATION snp_dosage_rule against np.interp, {cases.case_id(case)}: {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound
    assert (X >= 0.0).all()
    off = np.concatenate(([0], np.cumsum(points)))
    flat = np.concatenate(masks)
    for ci, k in enumerate(points):
        for name, point in ((f"{ci}:before", off[ci]), (f"{ci}:after", off[ci + 1] - 1)):
            j = labels.index(name)
            bits = [h for h in range(H) if flat[j] >> h & 1]
            want = np.zeros(len(D))
            for h in bits:
                want = want + D[:, point, h]
            np.testing.assert_array_equal(X[:, j], 2.0 * want)


def test_locate_follows_the_rule_at_the_edges():
    g = np.array([1.0, 2.0, 2.0, 4.0])
    lo, hi, t = cases.locate(g, np.array([0.0, 1.0, 1.5, 2.0, 3.0, 4.0, 9.0]))
    assert lo.tolist() == [0, 0, 0, 2, 2, 3, 3] and hi.tolist() == [1, 1, 1, 3, 3, 3, 3]
    assert t.tolist() == [0.0, 0.0, 0.5, 0.0, 0.5, 0.0, 0.0]
    lo, hi, t = cases.locate(np.array([5.0]), np.array([4.0, 5.0, 6.0]))
    assert lo.tolist() == hi.tolist() == [0, 0, 0] and t.tolist() == [0.0, 0.0, 0.0]


def test_the_one_hot_snp_on_a_grid_point_is_the_founder_scan():
    """H = 2 and the pattern `10` on a grid point m: the column spans what the founder scan's only column spans, so the LOD
    is scan_rule's at m within the case's bound, and `used` is its rank."""
    case = (2, 32, 2, 64, base.POINTS)
    D, Z, Y, _ = base.build(case)
    lod_points, rank = base.expected(case)[:2]
    grid = cases.grid_of(case)
    keep = [np.flatnonzero(np.concatenate(([True], g[1:] > g[:-1])) & np.concatenate((g[:-1] < g[1:], [True]))) for g in grid]
    pos = [g[k] for g, k in zip(grid, keep)]
    X = cases.snp_dosage_rule(D, case[4], grid, pos, [np.ones(len(x), dtype=np.uint32) for x in pos])
    off = np.concatenate(([0], np.cumsum(case[4])))
    points = np.concatenate([o + k for o, k in zip(off, keep)])
    np.testing.assert_array_equal(X, 2.0 * D[:, points, 0])
    lod, used, _ = cases.snp_rule(X, Z, Y)
    np.testing.assert_array_equal(used, rank[points] == 1)
    assert cases.deviation(lod, lod_points[:, points]) <= max(cases.cpu_bound(case), base.cpu_bound(case))


def test_peaks_skip_unused_snps():
    lod = np.array([[1.0, 9.0, 3.0, 3.0, 0.0]])
    used = np.array([True, False, True, True, False])
    peak, index = cases.snp_peaks(lod, used, [2, 2, 1, 0])
    assert index.tolist() == [[0, 2, -1, -1]] and peak[0, :2].tolist() == [1.0, 3.0] and np.isnan(peak[0, 2:]).all()


# ---- the commands' host side --------------------------------------------------------------------------------------------

def test_check_scan_snp_args():
    from gbrs_amd.scan import check_scan_snp_args
    check_scan_snp_args()                                                         # nothing asked for
    check_scan_snp_args(False, None, None, None, cohort=False)
    check_scan_snp_args(True, "snps.tsv", "pheno.tsv", "grid.txt", cohort=True)
    for kwargs, named in ((dict(snp_file=None), "--snp-file"), (dict(scan_pheno=None), "--scan-pheno"),
                          (dict(grid_file=None), "--grid-file"), (dict(cohort=False), "--sample-file")):
        full = dict(scan_snps=True, snp_file="snps.tsv", scan_pheno="pheno.tsv", grid_file="grid.txt", cohort=True)
        with pytest.raises(RuntimeError, match=f"--scan-snps needs {named}"):
            check_scan_snp_args(**dict(full, **kwargs))


def test_the_options_reach_the_check_before_any_file(tmp_path):
    """ReconstructOptions carries scan_snps, refuses it without its three companions and keeps it out of the
    single-sample call's keywords; both parsers know the new options."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import ReconstructOptions
    options = ReconstructOptions.of({"scan_snps": True, "snp_file": "snps.tsv"})
    assert options.scan_snps and "scan_snps" in options.keywords(cohort=True) and "scan_snps" not in options.keywords(cohort=False)
    with pytest.raises(RuntimeError, match="--scan-snps needs --scan-pheno"):
        options.check(True, "grid.txt", "tprob.npz")
    ReconstructOptions.of({}).check(True, None, "tprob.npz")
    for name in ("t.npz", "s.tsv", "g.txt", "p.tsv", "snps.tsv", "list.tsv"):
        (tmp_path / name).write_text("x\n")
    path = lambda name: str(tmp_path / name)
    parser = cli.build_parser()
    args = parser.parse_args(["reconstruct", "-t", path("t.npz"), "--sample-file", path("s.tsv"), "--grid-file", path("g.txt"),
                              "--scan-pheno", path("p.tsv"), "--snp-file", path("snps.tsv"), "--scan-snps"])
    assert args.scan_snps and args.snp_file == path("snps.tsv")
    args = parser.parse_args(["scan", "--dosage-list", path("list.tsv"), "--grid-file", path("g.txt"), "--pheno", path("p.tsv"),
                              "--snp-file", path("snps.tsv")])
    assert args.snp_file == path("snps.tsv")
    assert parser.parse_args(["scan", "--dosage-list", path("list.tsv"), "--grid-file", path("g.txt"), "--pheno",
                              path("p.tsv")]).snp_file is None


def snp_table(tmp_path):
    """A SNP file of seven lines on the chromosomes 2, 1, Q (foreign) and 3 (no grid points), shuffled, one cM NA."""
    from gbrs_amd.hmm import read_snp_file
    (tmp_path / "grid.txt").write_text("marker\tchr\tbp\tcM\n" + "".join(
        f"m{c}{k}\t{c}\t{1000 * k}\t{float(k)}\n" for c in ("1", "2") for k in range(4)))
    lines = [("a", "2", "500", "0.5", "10"), ("b", "Q", "1", "1.0", "11"), ("c", "1", "1500", "NA", "01"), ("d", "2", "100", "0.1", "01"),
             ("e", "3", "7", "0.7", "10"), ("f", "1", "10", "0.01", "11"), ("g", "2", "2900", "2.9", "00")]
    (tmp_path / "snps.tsv").write_text("id\tchr\tbp\tcM\tpattern\n" + "".join("\t".join(r) + "\n" for r in lines))
    return read_snp_file(str(tmp_path / "snps.tsv"), ["A", "B"], ["1", "2", "3"], str(tmp_path / "grid.txt"))


def test_the_snp_plan_and_the_file_order(tmp_path, caplog):
    """read_snp_file's rows as set_snps takes them: per chromosome of the scan in file order, the NA cM filled from bp, the
    SNPs of a chromosome without grid points left out with one warning; run_snps' arrays go back to the file's order
    with NaN / used = 0 / -1 for the SNPs that were not on the handle."""
    from gbrs_amd.scan import snp_plan, snps_in_file_order
    snps = snp_table(tmp_path)
    assert snps["foreign"] == 1 and snps["cM"][2] == 1.5
    grid = {"1": np.arange(4.0), "2": np.arange(4.0)}
    with caplog.at_level("WARNING", logger="gbrs"):
        grid_pos, snp_pos, masks, rows = snp_plan(snps, ["1", "2", "3"], [4, 4, 0], grid)
    assert sum("1 SNPs on chromosomes without grid points" in r.getMessage() for r in caplog.records) == 1
    assert rows.tolist() == [2, 5, 0, 3, 6] and [len(g) for g in grid_pos] == [4, 4, 0]
    assert [x.tolist() for x in snp_pos] == [[1.5, 0.01], [0.5, 0.1, 2.9], []]
    assert [m.tolist() for m in masks] == [[2, 3], [1, 2, 0], []]
    result = {"used": np.array([True, False, True, True, False]), "lod": np.arange(10.0).reshape(2, 5),
              "peak_lod": np.array([[0.0, 3.0, np.nan], [5.0, 8.0, np.nan]]), "peak_index": np.array([[0, 3, -1], [0, 3, -1]])}
    out = snps_in_file_order(result, rows, 7)
    assert out["used"].tolist() == [True, False, True, True, False, False, False]
    assert out["peak_snp"].tolist() == [[2, 3, -1], [2, 3, -1]]
    assert np.isnan(out["lod"][:, [1, 4]]).all() and out["lod"][0, [2, 5, 0, 3, 6]].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    lean = snps_in_file_order({k: v for k, v in result.items() if k != "lod"}, rows, 7)
    assert "lod" not in lean and lean["peak_snp"].tolist() == out["peak_snp"].tolist()


def test_the_snp_scan_files(tmp_path):
    """.scan.snps.npz in the SNP file's order and .scan.snps.peaks.tsv: one line per (phenotype, chromosome) with a used
    SNP whose peak reaches the minimum, the genome-wide maximum marked once per phenotype."""
    from gbrs_amd.scan import write_scan_snps
    snps = snp_table(tmp_path)
    result = {"used": np.array([True, False, True, True, False, False, False]),
              "peak_lod": np.array([[0.5, 3.0, np.nan], [5.0, 0.25, np.nan]]), "peak_snp": np.array([[2, 3, -1], [2, 0, -1]]),
              "lod": np.zeros((2, 7))}
    write_scan_snps(str(tmp_path / "out"), ["p0", "p1"], ["s0", "s1", "s2"], ["intercept"], snps, ["1", "2", "3"], result, 0.4)
    z = np.load(tmp_path / "out.scan.snps.npz")
    assert sorted(z.files) == sorted(["phenotypes", "samples", "covariates", "snp_id", "chrom", "bp", "cM", "pattern", "used",
                                      "peak_lod", "peak_snp", "lod"])
    assert z["snp_id"].tolist() == list("abcdefg") and z["pattern"][2] == "01" and z["cM"][2] == 1.5 and z["bp"][0] == 500.0
    np.testing.assert_array_equal(z["peak_snp"], result["peak_snp"])
    lines = open(tmp_path / "out.scan.snps.peaks.tsv").read().splitlines()
    assert lines == ["#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max",
                     "p0\t1\tc\t1500.0\t1.5\t01\t0.5\t0", "p0\t2\td\t100.0\t0.1\t01\t3.0\t1", "p1\t1\tc\t1500.0\t1.5\t01\t5.0\t1"]
    del result["lod"]
    write_scan_snps(str(tmp_path / "lean"), ["p0", "p1"], ["s0", "s1", "s2"], ["intercept"], snps, ["1", "2", "3"], result)
    assert "lod" not in np.load(tmp_path / "lean.scan.snps.npz").files
    assert len(open(tmp_path / "lean.scan.snps.peaks.tsv").read().splitlines()) == 5
