"""The host side of the SNP association under the mixed model (no GPU): the two host routes of
tests/scan_lmm_snp_cases.py against each other, flat SNPs and complement pairs, the `--scan-kinship-snps` option's checks in
both parsers, the file order and the writers on a made-up result."""
import numpy as np
import pytest

import scan_lmm_cases as lmm
import scan_lmm_snp_cases as cases


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_the_two_host_routes_agree(case):
    """Within CPU_HEADROOM x the recorded figure; `used` equals lstsq's rank and no ratio lies in the undecided band
    (expected() asserts both); the ratios stay on the recorded sides."""
    X, counts, rule, gls, rank = cases.expected(case)
    measured = cases.deviation(rule["lod"], gls)
    kept, skipped = cases.check_ratios(rule, rank)
    print(f"DEVIATION snp_lmm_rule against snp_lmm_gls, {cases.case_id(case)}: {measured:.3g}, recorded "
          f"{cases.measured_floor(case):.3g}; smallest kept ratio {kept:.3g}, largest skipped {skipped:.3g}")
    assert measured <= cases.cpu_bound(case)
    assert X.shape[1] == sum(counts) and rule["lod"].shape == (case[3] + cases.EXTRA, X.shape[1])
    assert kept >= cases.SMALLEST_KEPT * (1 - 1e-2) and skipped <= cases.LARGEST_SKIPPED * (1 + 1e-2)
    assert np.isfinite(rule["lod"]).all() and (rule["lod"] >= 0.0).all()


def test_some_lods_are_well_above_six():
    above = [case for case in cases.ALL_CASES if cases.expected(case)[2]["lod"].max() > 6.0]
    assert len(above) >= 10
    assert cases.expected(cases.LARGE_CASES[0])[2]["lod"].max() > 20.0


@pytest.mark.parametrize("case", [cases.CASES[0], cases.CASES[4], cases.CASES[7], cases.CASES[10]], ids=cases.case_id)
def test_flat_snps_are_unused_for_every_phenotype(case):
    _, _, rule, gls, rank = cases.expected(case)
    flat = cases.flat_snps(case)
    assert len(flat) >= 2
    assert not rule["used"][:, flat].any() and (rule["lod"][:, flat] == 0.0).all() and (rank[:, flat] == 0).all()
    assert rule["used"][:, [j for j in range(rule["used"].shape[1]) if j not in flat]].all()


@pytest.mark.parametrize("case", [cases.CASES[0], cases.CASES[4], cases.CASES[7], cases.CASES[10]], ids=cases.case_id)
def test_complement_pairs_give_equal_lods(case):
    """x and 2 - x span the same space beside the intercept: equal LODs up to the case's figure, in either route."""
    _, _, rule, gls, _ = cases.expected(case)
    pairs = cases.complement_pairs(case)
    assert pairs
    for a, b in pairs:
        assert cases.deviation(rule["lod"][:, a], rule["lod"][:, b]) <= cases.cpu_bound(case)
        assert cases.deviation(gls[:, a], gls[:, b]) <= cases.cpu_bound(case)
        assert rule["used"][:, [a, b]].all()


def test_zero_heritability_is_the_unweighted_snp_test():
    """h = 0 for every pair: the weights are 1, the rotation is orthogonal, and the rule is §29's test."""
    import scan_snp_cases as snp
    case = cases.CASES[0]
    D, Z, _, _, kin_of_chrom, _ = lmm.build(case)
    X, counts = cases.dosages(case)
    Y = lmm.centred(cases.phenotypes(case))
    rule = cases.snp_lmm_rule(X, counts, Z, Y, lmm.decompositions(case), kin_of_chrom, hsq=np.zeros((Y.shape[1], 3)))
    plain, used, _ = snp.snp_rule(X, Z, Y)
    assert cases.deviation(rule["lod"], plain) <= cases.cpu_bound(case)
    np.testing.assert_array_equal(rule["used"], np.broadcast_to(used, rule["used"].shape))


def test_peaks_skip_unused_pairs_and_count_the_used():
    lod = np.array([[1.0, 9.0, 3.0, 3.0, 0.0], [2.0, 9.0, 0.0, 4.0, 0.0]])
    used = np.array([[True, False, True, True, False], [True, True, False, True, False]])
    peak, index, count = cases.snp_lmm_peaks(lod, used, [2, 2, 1, 0])
    assert index.tolist() == [[0, 2, -1, -1], [1, 3, -1, -1]] and count.tolist() == [[1, 2, 0, 0], [2, 1, 0, 0]]
    assert peak[:, :2].tolist() == [[1.0, 3.0], [9.0, 4.0]] and np.isnan(peak[:, 2:]).all()


# ---- the commands' host side --------------------------------------------------------------------------------------------

def test_the_option_needs_the_kinship():
    from gbrs_amd.scan import check_scan_args, kinship_snp_options
    assert kinship_snp_options() is None and kinship_snp_options("snps.tsv", "loco") == "snps.tsv"
    with pytest.raises(RuntimeError, match="--scan-kinship-snps needs --scan-kinship"):
        kinship_snp_options("snps.tsv", None)
    full = dict(scan_pheno="pheno.tsv", grid_file="grid.txt", cohort=True)
    check_scan_args(**full, scan_kinship="loco", scan_kinship_snps="snps.tsv")
    with pytest.raises(RuntimeError, match="--scan-kinship-snps needs --scan-kinship"):
        check_scan_args(**full, scan_kinship_snps="snps.tsv")
    with pytest.raises(RuntimeError, match="--scan-kinship-snps needs --scan-pheno|--scan-kinship needs --scan-pheno"):
        check_scan_args(scan_kinship="loco", scan_kinship_snps="snps.tsv")
    with pytest.raises(RuntimeError, match="--scan-snps cannot be combined with --scan-kinship"):      # the refusal that stays
        check_scan_args(**full, scan_kinship="loco", scan_snps=True, scan_kinship_snps="snps.tsv")


def test_the_option_reaches_the_check_before_any_file(tmp_path):
    """ReconstructOptions carries scan_kinship_snps, refuses it without the kinship and keeps it out of the single-sample
    call's keywords; both parsers know the option, and `gbrs scan` refuses it before the grid file is read."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import ReconstructOptions
    from gbrs_amd.scan import scan_tables
    options = ReconstructOptions.of({"scan_kinship_snps": "snps.tsv", "scan_pheno": "p.tsv"})
    assert options.scan_kinship_snps == "snps.tsv" and "scan_kinship_snps" in options.keywords(cohort=True)
    assert "scan_kinship_snps" not in options.keywords(cohort=False)
    with pytest.raises(RuntimeError, match="--scan-kinship-snps needs --scan-kinship"):
        options.check(True, "grid.txt", "tprob.npz")
    ReconstructOptions.of({"scan_kinship_snps": "snps.tsv", "scan_pheno": "p.tsv", "scan_kinship": "loco"}).check(True, "grid.txt", "tprob.npz")
    assert ReconstructOptions.of({}).scan_kinship_snps is None
    for name in ("t.npz", "s.tsv", "g.txt", "p.tsv", "snps.tsv", "list.tsv"):
        (tmp_path / name).write_text("x\n")
    path = lambda name: str(tmp_path / name)
    parser = cli.build_parser()
    args = parser.parse_args(["reconstruct", "-t", path("t.npz"), "--sample-file", path("s.tsv"), "--grid-file", path("g.txt"),
                              "--scan-pheno", path("p.tsv"), "--scan-kinship", "loco", "--scan-kinship-snps", path("snps.tsv")])
    assert args.scan_kinship_snps == path("snps.tsv") and args.snp_file is None and not args.scan_snps
    args = parser.parse_args(["scan", "--dosage-list", path("list.tsv"), "--grid-file", path("g.txt"), "--pheno", path("p.tsv"),
                              "--scan-kinship", "overall", "--scan-kinship-snps", path("snps.tsv")])
    assert args.scan_kinship_snps == path("snps.tsv") and args.snp_file is None
    assert parser.parse_args(["scan", "--dosage-list", path("list.tsv"), "--grid-file", path("g.txt"), "--pheno",
                              path("p.tsv")]).scan_kinship_snps is None
    with pytest.raises(SystemExit):
        parser.parse_args(["scan", "--dosage-list", path("list.tsv"), "--grid-file", path("g.txt"), "--pheno", path("p.tsv"),
                           "--scan-kinship-snps", path("missing.tsv")])
    with pytest.raises(RuntimeError, match="--scan-kinship-snps needs --scan-kinship"):     # g.txt is no grid file: not read yet
        scan_tables(path("list.tsv"), path("g.txt"), path("p.tsv"), scan_kinship_snps=path("snps.tsv"))


def snp_table(tmp_path):
    """test_scan_snp_cpu.py's SNP file: seven lines on the chromosomes 2, 1, Q (foreign) and 3 (no grid points)."""
    from gbrs_amd.hmm import read_snp_file
    (tmp_path / "grid.txt").write_text("marker\tchr\tbp\tcM\n" + "".join(
        f"m{c}{k}\t{c}\t{1000 * k}\t{float(k)}\n" for c in ("1", "2") for k in range(4)))
    lines = [("a", "2", "500", "0.5", "10"), ("b", "Q", "1", "1.0", "11"), ("c", "1", "1500", "NA", "01"), ("d", "2", "100", "0.1", "01"),
             ("e", "3", "7", "0.7", "10"), ("f", "1", "10", "0.01", "11"), ("g", "2", "2900", "2.9", "00")]
    (tmp_path / "snps.tsv").write_text("id\tchr\tbp\tcM\tpattern\n" + "".join("\t".join(r) + "\n" for r in lines))
    return read_snp_file(str(tmp_path / "snps.tsv"), ["A", "B"], ["1", "2", "3"], str(tmp_path / "grid.txt"))


def test_the_file_order_of_a_result():
    from gbrs_amd.scan import snps_lmm_in_file_order
    rows = np.array([2, 5, 0, 3, 6])
    result = {"used": np.array([[True, False, True, True, False], [True, True, True, False, False]]),
              "lod": np.arange(10.0).reshape(2, 5), "peak_lod": np.array([[0.0, 3.0, np.nan], [6.0, 7.0, np.nan]]),
              "peak_index": np.array([[0, 3, -1], [1, 2, -1]]), "n_used": np.array([[1, 2, 0], [2, 1, 0]]),
              "hsq": np.array([[0.25, 0.5, 0.75], [0.0, 1.0, 0.5]])}
    out = snps_lmm_in_file_order(result, rows, 7)
    assert out["used"].tolist() == [[True, False, True, True, False, False, False], [True, False, True, False, False, True, False]]
    assert out["peak_snp"].tolist() == [[2, 3, -1], [5, 0, -1]]
    assert np.isnan(out["lod"][:, [1, 4]]).all() and out["lod"][0, [2, 5, 0, 3, 6]].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert out["n_used"] is result["n_used"] and out["hsq"] is result["hsq"]
    lean = snps_lmm_in_file_order({k: v for k, v in result.items() if k not in ("lod", "used")}, rows, 7)
    assert "lod" not in lean and "used" not in lean and lean["peak_snp"].tolist() == out["peak_snp"].tolist()


def test_the_writers_on_a_made_up_result(tmp_path):
    """write_scan_snps' members plus hsq, n_used and kinship_mode; `used` only beside the LOD matrix; the peaks file has
    the column hsq."""
    from gbrs_amd.scan import write_scan_snps_lmm
    snps = snp_table(tmp_path)
    result = {"peak_lod": np.array([[0.5, 3.0, np.nan], [5.0, 0.25, np.nan]]), "peak_snp": np.array([[2, 3, -1], [2, 0, -1]]),
              "n_used": np.array([[2, 2, 0], [2, 3, 0]]), "hsq": np.array([[0.25, 0.5, 0.75], [0.0, 1.0, 0.125]]),
              "lod": np.zeros((2, 7)), "used": np.ones((2, 7), dtype=bool)}
    write_scan_snps_lmm(str(tmp_path / "out"), ["p0", "p1"], ["s0", "s1", "s2"], ["intercept"], snps, ["1", "2", "3"], result, 0.4,
                        "loco")
    z = np.load(tmp_path / "out.scan.snps.npz")
    assert sorted(z.files) == sorted(["phenotypes", "samples", "covariates", "snp_id", "chrom", "bp", "cM", "pattern", "used",
                                      "peak_lod", "peak_snp", "lod", "hsq", "n_used", "kinship_mode"])
    assert z["snp_id"].tolist() == list("abcdefg") and str(z["kinship_mode"]) == "loco" and z["used"].shape == (2, 7)
    np.testing.assert_array_equal(z["hsq"], result["hsq"])
    np.testing.assert_array_equal(z["n_used"], result["n_used"])
    lines = open(tmp_path / "out.scan.snps.peaks.tsv").read().splitlines()
    assert lines == ["#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max\thsq",
                     "p0\t1\tc\t1500.0\t1.5\t01\t0.5\t0\t0.25", "p0\t2\td\t100.0\t0.1\t01\t3.0\t1\t0.5",
                     "p1\t1\tc\t1500.0\t1.5\t01\t5.0\t1\t0.0"]
    del result["lod"], result["used"]
    write_scan_snps_lmm(str(tmp_path / "lean"), ["p0", "p1"], ["s0", "s1", "s2"], ["intercept"], snps, ["1", "2", "3"], result, 0.0,
                        "overall")
    lean = np.load(tmp_path / "lean.scan.snps.npz")
    assert "lod" not in lean.files and "used" not in lean.files and str(lean["kinship_mode"]) == "overall"
