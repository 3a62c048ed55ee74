"""The two host routes of the founder effects under the mixed model against each other (tests/scan_lmm_effects_cases.py;
DESIGN.md §34), the condition under which they may be compared, the consequences of the rule on the restatement, and the
options of the two commands.  No GPU."""
import numpy as np
import pytest

import scan_lmm_cases as lmm
import scan_lmm_effects_cases as cases


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_two_routes_agree(case):
    """Within CPU_HEADROOM times the recorded figure; at every target the ranks agree and no singular value lies in the
    undecided band; the figure recorded for the case is the one measured (printed for the record)."""
    rule, gls, shares = cases.expected(case)
    assert not ((shares > cases.SVD_UNDECIDED[0]) & (shares < cases.SVD_UNDECIDED[1])).any()
    np.testing.assert_array_equal(rule["rank"], gls["rank"])
    measured = cases.measure([case])[cases.case_id(case)]
    print(f"'{cases.case_id(case)}': ({', '.join(f'{v:.3g}' for v in measured)}),")
    for key, value in zip(cases.KEYS, measured):
        assert value <= cases.cpu_bound(case, key), key
    T = {cases.CHUNK: cases.CHUNK_T}.get(case)
    assert T is None or len(rule["rank"]) == T


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_consequences_of_the_rule(case):
    H, n, cz, P, points, _ = case
    pheno, columns, at, planted = cases.build(case)
    rule, gls, _ = cases.expected(case)
    full = rule["rank"] == H - 1
    assert full.any()
    for route in (rule, gls):                                                       # zero-sum at full rank
        assert np.abs(route["effect"][full].sum(axis=1)).max() <= cases.cpu_bound(case, "effect") * H * max(1.0, np.abs(route["effect"][full]).max())
    t = planted["zero"]                                                             # a founder without dosage: exactly zero
    assert rule["rank"][t] == H - 2 and rule["effect"][t, 0] == 0.0 and rule["se"][t, 0] == 0.0
    assert abs(gls["effect"][t, 0]) <= cases.cpu_bound(case, "effect") and rule["effect"][t].any() == (H > 2)
    if "equal" in planted:                                                          # identical dosages: identical bits
        t = planted["equal"]
        assert rule["rank"][t] == H - 2
        assert rule["effect"][t, 0] == rule["effect"][t, 1] and rule["se"][t, 0] == rule["se"][t, 1] and rule["effect"][t, 0] != 0.0
    else:                                                                           # H = 2: r = 0
        assert rule["rank"][t] == 0 and not rule["effect"][t].any() and not rule["se"][t].any() and rule["lod"][t] == 0.0
        assert not gls["effect"][t].any() and not gls["se"][t].any() and abs(gls["lod"][t]) <= cases.cpu_bound(case, "lod")
    t = planted["exact"]
    for route in (rule, gls):
        assert np.isfinite(route["se"][t]).all() and route["lod"][t] >= cases.exact_lod_bound(n)
        assert route["sigma2"][t] <= cases.EXACT_SHARE * cases.whitened_size(case)
    assert np.abs(rule["effect"][t] - gls["effect"][t]).max() <= cases.cpu_bound(case, "effect") * max(1.0, np.abs(gls["effect"][t]).max())


def test_a_constant_column_and_sigma2s_scale():
    """A column of zeros gives hsq 0, effects 0.0 and lod 0.0 in either route; with the heritability held at zero the rule is
    §31's on the rotated cohort, and sigma2 is §32's s2 at the alternative: rss1 / (n - cz - r) on the whitened scale."""
    case = lmm.CASES[8]
    H, n, cz, P, points, _ = case
    D, Z, _, kinships, kin_of_chrom, _ = lmm.build(case)
    pheno = np.column_stack([cases.build(case)[0], np.full(n, 2.5)])
    hsq = np.vstack([cases.rule_hsq(case), np.full(3, 0.4)])
    col, at = np.array([P + 1, 0], dtype=np.int64), np.array([3, 3], dtype=np.int64)
    rule = cases.effects_lmm_rule(D, Z, pheno, points, lmm.decompositions(case), kin_of_chrom, col, at, hsq)
    gls = cases.effects_lmm_gls(D, Z, pheno, points, kinships, kin_of_chrom, col, at, hsq)
    for route in (rule, gls):
        assert not route[0][0].any() and not route[1][0].any() and route[2][0] == 0.0 and route[3][0] == 0.0
    e = kin_of_chrom[cases.chrom_of(points, 3)]
    h = hsq[0, e]
    C = np.linalg.cholesky(h * kinships[e] + (1.0 - h) * np.eye(n))
    A = np.linalg.solve(C, np.column_stack([Z, D[:, 3, :H - 1], lmm.centred(pheno)[:, 0]]))
    res = A[:, -1] - A[:, :-1] @ np.linalg.lstsq(A[:, :-1], A[:, -1], rcond=None)[0]
    np.testing.assert_allclose(rule[3][1], res @ res / (n - cz - (H - 1)), rtol=1e-10)


def test_the_option_checks():
    from gbrs_amd.scan import DEFAULT_EFFECTS_MIN_LOD, check_scan_args, kinship_effects_options
    assert kinship_effects_options() is None
    assert kinship_effects_options(False, None, None, "loco") is None
    assert kinship_effects_options(True, None, None, "loco") == {"min_lod": DEFAULT_EFFECTS_MIN_LOD, "lod_drop": None}
    assert kinship_effects_options(True, 2.5, 1.5, "overall") == {"min_lod": 2.5, "lod_drop": 1.5}
    assert kinship_effects_options(False, None, 0, "loco") == {"min_lod": None, "lod_drop": 0.0}
    for args, message in (((True,), "--scan-kinship-effects needs --scan-kinship"),
                          ((False, 3.0), "--scan-kinship-effects-min-lod needs --scan-kinship"),
                          ((False, None, 1.5), "--scan-kinship-lod-drop needs --scan-kinship"),
                          ((False, 3.0, None, "loco"), "--scan-kinship-effects-min-lod needs --scan-kinship-effects"),
                          ((True, -1.0, None, "loco"), "--scan-kinship-effects-min-lod must be"),
                          ((True, float("nan"), None, "loco"), "--scan-kinship-effects-min-lod must be"),
                          ((True, float("inf"), None, "loco"), "--scan-kinship-effects-min-lod must be"),
                          ((False, None, -0.5, "loco"), "--scan-kinship-lod-drop must be"),
                          ((False, None, float("inf"), "loco"), "--scan-kinship-lod-drop must be"),
                          ((False, None, float("nan"), "loco"), "--scan-kinship-lod-drop must be")):
        with pytest.raises(RuntimeError, match=message):
            kinship_effects_options(*args)
    check_scan_args("p.tsv", grid_file="g.txt", cohort=True, scan_kinship="loco", scan_kinship_effects=True,
                    scan_kinship_effects_min_lod=3.0, scan_kinship_lod_drop=1.5)
    check_scan_args("p.tsv", grid_file="g.txt", cohort=True, scan_kinship="loco", scan_kinship_lod_drop=1.5)
    for how, message in ((dict(scan_kinship="loco", scan_kinship_effects=True), "--scan-kinship needs --scan-pheno"),
                         (dict(scan_pheno="p.tsv", scan_kinship_effects=True), "--scan-kinship-effects needs --scan-kinship"),
                         (dict(scan_pheno="p.tsv", scan_kinship_lod_drop=1.5), "--scan-kinship-lod-drop needs --scan-kinship"),
                         (dict(scan_pheno="p.tsv", scan_kinship="loco", scan_kinship_effects_min_lod=3.0),
                          "--scan-kinship-effects-min-lod needs --scan-kinship-effects"),
                         (dict(scan_pheno="p.tsv", scan_kinship="loco", scan_kinship_lod_drop=-1.0), "--scan-kinship-lod-drop must be"),
                         (dict(scan_pheno="p.tsv", scan_kinship="loco", scan_kinship_effects=True, scan_kinship_effects_min_lod=-2.0),
                          "--scan-kinship-effects-min-lod must be"),
                         # the passes of the unweighted W stay refused next to the kinship
                         (dict(scan_pheno="p.tsv", scan_kinship="loco", scan_effects=True), "--scan-effects cannot be combined with --scan-kinship"),
                         (dict(scan_pheno="p.tsv", scan_kinship="overall", scan_lod_drop=1.5, scan_kinship_lod_drop=1.5),
                          "--scan-lod-drop cannot be combined with --scan-kinship")):
        with pytest.raises(RuntimeError, match=message):
            check_scan_args(grid_file="g.txt", cohort=True, **how)


def test_the_commands_take_the_options_and_refuse_before_a_file_is_read(tmp_path, caplog):
    from gbrs_amd import cli
    f = str(tmp_path / "file")
    open(f, "w").close()
    missing = str(tmp_path / "missing")                                             # never opened: the refusal comes first
    for command in (["reconstruct", "--sample-file", f, "-t", f, "--grid-file", f, "--scan-pheno", f],
                    ["scan", "--dosage-list", f, "--grid-file", f, "--pheno", f]):
        args = cli.build_parser().parse_args(command + ["--scan-kinship", "loco", "--scan-kinship-effects", "--scan-kinship-effects-min-lod",
                                                        "2", "--scan-kinship-lod-drop", "1.5"])
        assert args.scan_kinship_effects and args.scan_kinship_effects_min_lod == 2.0 and args.scan_kinship_lod_drop == 1.5
        args = cli.build_parser().parse_args(command)
        assert not args.scan_kinship_effects and args.scan_kinship_effects_min_lod is None and args.scan_kinship_lod_drop is None
        for extra, message in ((["--scan-kinship-effects"], "--scan-kinship-effects needs --scan-kinship"),
                               (["--scan-kinship", "loco", "--scan-kinship-lod-drop", "-1"], "--scan-kinship-lod-drop must be"),
                               (["--scan-kinship", "loco", "--scan-effects"], "--scan-effects cannot be combined with --scan-kinship")):
            caplog.clear()
            with caplog.at_level("ERROR", logger="gbrs"):
                cli.main(command + ["--scan-out", missing] + extra)
            assert any(message in r.getMessage() for r in caplog.records), (command[0], extra, [r.getMessage() for r in caplog.records])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["file"]


PEAK = np.array([[1.0, 5.0, np.nan], [0.5, 0.5, np.nan]])
INDEX = np.array([[0, 2, -1], [1, 3, -1]])
WRITE = (["a", "b"], ["s0", "s1"], ["intercept"], ["1", "1", "2", "2"], [0.5, 1.5, 0.25, 2.0], ["1", "2", "3"])


def test_the_files_with_and_without_the_options(tmp_path):
    """write_scan under a kinship: with a drop the two support columns follow hsq and the archive gains three members;
    without one the files are what they were, whatever the result holds.  write_scan_effects: hsq after rank."""
    from gbrs_amd.scan import write_scan, write_scan_effects
    lo, hi = np.array([[0, 2, -1], [0, 2, -1]]), np.array([[1, 3, -1], [1, 3, -1]])
    result = {"peak_lod": PEAK, "peak_index": INDEX, "lod": np.zeros((2, 4)), "hsq": np.full((2, 3), 0.25), "sigma2": np.ones((2, 3)),
              "rank_min": np.ones(2, dtype=np.int32), "rank_max": np.ones(2, dtype=np.int32), "support_lo": lo, "support_hi": hi}
    write_scan(str(tmp_path / "x"), *WRITE, result, None, min_lod=0.75, lod_drop=1.5, kinship_mode="loco")
    assert open(tmp_path / "x.scan.peaks.tsv").read().splitlines() == [
        "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\thsq\tsupport_lo\tsupport_hi", "a\t1\t0.5\t1.0\t0\t0.25\t0.5\t1.5",
        "a\t2\t0.25\t5.0\t1\t0.25\t0.25\t2.0"]
    z = np.load(tmp_path / "x.scan.npz")
    assert z["lod_drop"] == 1.5 and z.files[-3:] == ["support_lo", "support_hi", "lod_drop"]
    np.testing.assert_array_equal(z["support_hi"], hi)
    write_scan(str(tmp_path / "y"), *WRITE, result, None, min_lod=0.75, kinship_mode="loco")
    assert open(tmp_path / "y.scan.peaks.tsv", "rb").read() == (b"#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\thsq\n"
                                                                b"a\t1\t0.5\t1.0\t0\t0.25\na\t2\t0.25\t5.0\t1\t0.25\n")
    assert np.load(tmp_path / "y.scan.npz").files == ["phenotypes", "samples", "covariates", "chrom", "pos", "peak_lod", "peak_index", "hsq",
                                                      "sigma2", "rank_min", "rank_max", "kinship_mode", "lod"]
    got = {"effect": np.array([[1.0, -1.0]]), "se": np.array([[0.5, 0.5]]), "lod": np.array([5.0]), "sigma2": np.array([2.0]),
           "rank": np.array([1], dtype=np.int32), "hsq": np.array([0.25])}
    args = (["a", "b"], ["A", "B"], ["s0", "s1"], ["intercept"], ["1", "2", "3"], [0.5, 1.5, 0.25, 2.0], [[0, 1]], [2], got, 3.0)
    write_scan_effects(str(tmp_path / "m"), *args, kinship_mode="loco")
    assert open(tmp_path / "m.scan.effects.tsv").read().splitlines() == [
        "#phenotype\tchromosome\tposition\tlod\trank\thsq\teffect_A\tse_A\teffect_B\tse_B", "a\t2\t0.25\t5.0\t1\t0.25\t1.0\t0.5\t-1.0\t0.5"]
    z = np.load(tmp_path / "m.scan.effects.npz")
    assert z.files[-2:] == ["hsq", "kinship_mode"] and str(z["kinship_mode"]) == "loco"
    write_scan_effects(str(tmp_path / "p"), *args)
    assert open(tmp_path / "p.scan.effects.tsv").read().splitlines() == [
        "#phenotype\tchromosome\tposition\tlod\trank\teffect_A\tse_A\teffect_B\tse_B", "a\t2\t0.25\t5.0\t1\t1.0\t0.5\t-1.0\t0.5"]
    assert "hsq" not in np.load(tmp_path / "p.scan.effects.npz").files
