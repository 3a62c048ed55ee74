"""The host side of the founder effects and the LOD support intervals (no GPU): the two host computations of
tests/scan_effects_cases.py against each other, the properties of the rule, the interval rule on hand-made LOD rows, the
option checks and the writers."""
import zipfile

import numpy as np
import pytest

import scan_cases as base
import scan_effects_cases as cases


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_rule_agrees_with_the_svd(case):
    """The restatement of the rule against the SVD route, which knows nothing of W: every output within the case's measured
    floor (with headroom), the ranks equal, no singular value where rounding could move the rank, the effects of a
    full-rank point adding up to zero, and what the planted targets are there to show."""
    H, n, c, T = case
    D, Z, pheno, columns, points, planted = cases.build(case)
    rule, svd, shares = cases.expected(case)
    np.testing.assert_array_equal(rule["rank"], svd["rank"])
    assert not ((shares >= cases.SVD_UNDECIDED[0]) & (shares <= cases.SVD_UNDECIDED[1])).any()
    figures = {}
    for key in cases.KEYS:
        on = cases.judged(case, key)
        figures[key] = cases.deviation(rule[key][on], svd[key][on])
    print(f"DEVIATION effects_rule against effects_svd " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()) +
          f"; {cases.case_id(case)}")
    for key, worst in figures.items():
        assert worst <= cases.cpu_bound(case, key), key
    full = rule["rank"] == H - 1
    assert full.any()
    for route in (rule, svd):
        total = np.abs(route["effect"][full].sum(axis=1)) / np.maximum(1.0, np.abs(route["effect"][full]).max(axis=1))
        assert total.max() <= H * cases.cpu_bound(case, "effect")
        assert np.isfinite(route["se"]).all() and (route["se"] >= 0).all() and (route["sigma2"] >= 0).all()
    if planted:
        t = planted["zero"]                                                         # founder 0 has no dosage there
        assert rule["effect"][t, 0] == 0.0 and rule["se"][t, 0] == 0.0
        assert abs(svd["effect"][t, 0]) <= cases.cpu_bound(case, "effect") and abs(svd["se"][t, 0]) <= cases.cpu_bound(case, "se")
        if H >= 3:
            t = planted["equal"]                                                    # founders 0 and 1 are the same column
            for route in (rule, svd):
                assert abs(route["effect"][t, 0] - route["effect"][t, 1]) <= cases.cpu_bound(case, "effect") * max(1.0, np.abs(route["effect"][t]).max())
                assert abs(route["se"][t, 0] - route["se"][t, 1]) <= cases.cpu_bound(case, "se") * max(1.0, route["se"][t].max())
        else:
            assert rule["rank"][planted["zero"]] == 0 and not rule["effect"][planted["zero"]].any() and not rule["se"][planted["zero"]].any()
        t = planted["constant"]
        for route in (rule, svd):
            assert not route["effect"][t].any() and not route["se"][t].any() and route["lod"][t] == 0.0 and route["sigma2"][t] == 0.0
        for key in ("effect", "se", "lod", "sigma2"):
            np.testing.assert_array_equal(rule[key][planted["twice"]], rule[key][0])
        t = planted["exact"]
        for route in (rule, svd):
            assert np.isfinite(route["se"][t]).all() and route["lod"][t] >= cases.exact_lod_bound(n)
            assert route["sigma2"][t] <= cases.EXACT_SHARE * (pheno[:, columns[t]] ** 2).sum()


def test_the_minimum_norm_solution_is_the_pseudo_inverse():
    """effect = R' C^-1 a is pinv(X~_full) y~: against np.linalg.pinv on the tile case, at every target."""
    case = cases.TILE
    D, Z, pheno, columns, points, _ = cases.build(case)
    rule = cases.expected(case)[0]
    Q = np.linalg.qr(Z)[0]
    for t in range(0, case[3], 7):
        X = D[:, points[t], :] - Q @ (Q.T @ D[:, points[t], :])
        X[:, -1] = -X[:, :-1].sum(axis=1)
        y = cases.zeroed(pheno)[:, columns[t]]
        want = np.linalg.pinv(X, rcond=1e-8) @ (y - Q @ (Q.T @ y))
        assert np.abs(rule["effect"][t] - want).max() <= cases.cpu_bound(case, "effect") * max(1.0, np.abs(want).max())


def test_the_interval_rule_on_hand_made_rows():
    inf = np.inf
    rule = lambda rows, points, drop: tuple(a.tolist() for a in cases.support_rule(np.array(rows, dtype=float), points, drop))
    # a one-point chromosome, then five points with the peak inside: the nearest fallen points on either side
    assert rule([[3.0, 1.0, 3.9, 5.0, 4.0, 1.0]], (1, 5), 1.5) == ([[0, 3]], [[0, 1]], [[0, 5]])
    # a peak at either end: the missing side is the chromosome's end, the peak itself
    assert rule([[5.0, 4.0, 3.0, 1.0]], (4,), 1.5) == ([[0]], [[0]], [[2]])
    assert rule([[1.0, 3.0, 4.0, 5.0]], (4,), 1.5) == ([[3]], [[1]], [[3]])
    # ties: the peak is the first of the largest; an equal point has not fallen unless the drop is 0
    assert rule([[1.0, 5.0, 5.0, 5.0, 1.0]], (5,), 1.5) == ([[1]], [[0]], [[4]])
    assert rule([[1.0, 5.0, 5.0, 5.0, 1.0]], (5,), 0.0) == ([[1]], [[0]], [[2]])
    # drop = 0: the neighbours, whatever they hold (they cannot be above the peak)
    assert rule([[1.0, 4.9, 5.0, 4.9, 1.0]], (5,), 0.0) == ([[2]], [[1]], [[3]])
    # a drop larger than the peak: LODs are not negative, nothing has fallen, the chromosome's ends
    assert rule([[1.0, 4.0, 5.0, 4.0, 1.0]], (5,), 1e6) == ([[2]], [[0]], [[4]])
    # a +inf peak: the bound is +inf and every neighbour has fallen, another +inf included
    assert rule([[1.0, inf, 2.0, inf]], (4,), 1.5) == ([[1]], [[0]], [[2]])
    # an all-zero row: the peak is the first point; with a drop nothing has fallen, with none the neighbour has
    assert rule([[0.0, 0.0, 0.0]], (3,), 1.5) == ([[0]], [[0]], [[2]])
    assert rule([[0.0, 0.0, 0.0]], (3,), 0.0) == ([[0]], [[0]], [[1]])
    # a chromosome without points
    assert rule([[2.0, 1.0]], (0, 2), 0.5) == ([[-1, 0]], [[-1, 0]], [[-1, 1]])
    # the fixture of the long walk: the LOD has fallen 73 points from the peak, one short of the chromosome's end, and nowhere nearer
    for side, (k, lo, hi) in cases.PLATEAU_WANT.items():
        D, Z, Y = cases.plateau(side)
        assert rule(base.scan_rule(D, Z, Y)[0], cases.PLATEAU_POINTS, cases.PLATEAU_DROP) == ([[k]], [[lo]], [[hi]])


def test_the_option_checks():
    from gbrs_amd.scan import DEFAULT_MEDIATE_MIN_LOD, check_scan_args, effects_options
    assert effects_options() is None
    assert effects_options(True) == {"min_lod": DEFAULT_MEDIATE_MIN_LOD, "lod_drop": None}
    assert effects_options(True, 2.5, 1.5) == {"min_lod": 2.5, "lod_drop": 1.5}
    assert effects_options(False, None, 0) == {"min_lod": None, "lod_drop": 0.0}
    for args, message in (((False, 3.0), "--scan-effects-min-lod needs --scan-effects"),
                          ((True, -1.0), "--scan-effects-min-lod must be"), ((True, float("nan")), "--scan-effects-min-lod must be"),
                          ((False, None, -0.5), "--scan-lod-drop must be"), ((False, None, float("inf")), "--scan-lod-drop must be"),
                          ((False, None, float("nan")), "--scan-lod-drop must be")):
        with pytest.raises(RuntimeError, match=message):
            effects_options(*args)
    check_scan_args("p.tsv", grid_file="g.txt", cohort=True, scan_effects=True, scan_effects_min_lod=3.0, scan_lod_drop=1.5)
    for how, message in ((dict(scan_effects=True), "--scan-effects needs --scan-pheno"),
                         (dict(scan_lod_drop=1.5), "--scan-lod-drop needs --scan-pheno"),
                         (dict(scan_pheno="p.tsv", scan_effects_min_lod=3.0), "--scan-effects-min-lod needs --scan-effects"),
                         (dict(scan_pheno="p.tsv", scan_lod_drop=-1.0), "--scan-lod-drop must be")):
        with pytest.raises(RuntimeError, match=message):
            check_scan_args(grid_file="g.txt", cohort=True, **how)


def test_the_commands_take_the_options(tmp_path):
    from gbrs_amd.cli import build_parser
    f = str(tmp_path / "file")
    open(f, "w").close()
    for command in (["reconstruct", "--sample-file", f, "-t", f, "--grid-file", f, "--scan-pheno", f],
                    ["scan", "--dosage-list", f, "--grid-file", f, "--pheno", f]):
        args = build_parser().parse_args(command + ["--scan-effects", "--scan-effects-min-lod", "2", "--scan-lod-drop", "1.5"])
        assert args.scan_effects and args.scan_effects_min_lod == 2.0 and args.scan_lod_drop == 1.5
        args = build_parser().parse_args(command)
        assert not args.scan_effects and args.scan_effects_min_lod is None and args.scan_lod_drop is None


PEAK = np.array([[1.0, 5.0, np.nan], [0.5, 0.5, np.nan]])
INDEX = np.array([[0, 2, -1], [1, 3, -1]])
WRITE = (["a", "b"], ["s0", "s1"], ["intercept"], ["1", "1", "2", "2"], [0.5, 1.5, 0.25, 2.0], ["1", "2", "3"])


def test_the_support_columns_of_the_peak_file(tmp_path):
    from gbrs_amd.scan import write_scan
    lo, hi = np.array([[0, 2, -1], [0, 2, -1]]), np.array([[1, 3, -1], [1, 3, -1]])
    result = {"peak_lod": PEAK, "peak_index": INDEX, "lod": np.zeros((2, 4)), "support_lo": lo, "support_hi": hi}
    write_scan(str(tmp_path / "x"), *WRITE, result, [1, 1, 1, 1], min_lod=0.75, lod_drop=1.5)
    lines = open(tmp_path / "x.scan.peaks.tsv").read().splitlines()
    assert lines == ["#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tsupport_lo\tsupport_hi", "a\t1\t0.5\t1.0\t0\t0.5\t1.5",
                     "a\t2\t0.25\t5.0\t1\t0.25\t2.0"]
    z = np.load(tmp_path / "x.scan.npz")
    assert z["lod_drop"] == 1.5
    np.testing.assert_array_equal(z["support_lo"], lo)
    np.testing.assert_array_equal(z["support_hi"], hi)
    # with permutations the two columns come after the permutation columns
    perm = {"perm_max": np.array([[0.5, 2.0, 6.0]]), "columns": [0], "mask": [True, True, False], "alphas": [0.5], "seed": 3}
    write_scan(str(tmp_path / "p"), *WRITE, result, [1, 1, 1, 1], min_lod=0.75, perm=perm, lod_drop=1.5)
    lines = open(tmp_path / "p.scan.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tpvalue\tthreshold_0.5\tsupport_lo\tsupport_hi"
    assert lines[1] == "a\t1\t0.5\t1.0\t0\t0.75\t2.0\t0.5\t1.5" and lines[2] == "a\t2\t0.25\t5.0\t1\t0.5\t2.0\t0.25\t2.0"
    for line in lines[1:]:
        assert [repr(float(v)) for v in line.split("\t")[-2:]] == line.split("\t")[-2:]


def test_without_the_options_the_scan_files_are_what_they_were(tmp_path):
    """write_scan called the way the existing tests call it, with and without permutations: the peaks file byte for byte what
    the format says, the archive's members those it had, and a result that holds intervals changes neither."""
    from gbrs_amd.scan import write_scan
    result = {"peak_lod": PEAK, "peak_index": INDEX, "lod": np.zeros((2, 4))}
    write_scan(str(tmp_path / "x"), *WRITE, result, [1, 1, 1, 1], min_lod=0.75)
    more = dict(result, support_lo=INDEX, support_hi=INDEX)
    write_scan(str(tmp_path / "y"), *WRITE, more, [1, 1, 1, 1], min_lod=0.75)
    text = "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\na\t1\t0.5\t1.0\t0\na\t2\t0.25\t5.0\t1\n"
    for name in "xy":
        assert open(tmp_path / f"{name}.scan.peaks.tsv", "rb").read() == text.encode()
        with zipfile.ZipFile(tmp_path / f"{name}.scan.npz") as archive:
            assert archive.namelist() == [f"{k}.npy" for k in ("phenotypes", "samples", "covariates", "chrom", "pos", "rank", "peak_lod",
                                                               "peak_index", "lod")]
    a, b = np.load(tmp_path / "x.scan.npz"), np.load(tmp_path / "y.scan.npz")
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes()
    perm = {"perm_max": np.array([[0.5, 2.0, 6.0]]), "columns": [0], "mask": [True, True, False], "alphas": [0.5], "seed": 3}
    write_scan(str(tmp_path / "p"), *WRITE, result, [1, 1, 1, 1], min_lod=0.75, perm=perm)
    assert open(tmp_path / "p.scan.peaks.tsv").read() == ("#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tpvalue\tthreshold_0.5\n"
                                                           "a\t1\t0.5\t1.0\t0\t0.75\t2.0\na\t2\t0.25\t5.0\t1\t0.5\t2.0\n")


def test_the_effects_files(tmp_path):
    from gbrs_amd.scan import write_scan_effects
    result = {"effect": np.array([[0.1, -0.3, 0.2], [1e-17, 2.5, -2.5]]), "se": np.array([[0.01, 0.02, 1 / 3], [0.0, 1.5, 1.5]]),
              "lod": np.array([7.25, np.inf]), "sigma2": np.array([0.5, 0.0]), "rank": np.array([2, 1], dtype=np.int32)}
    targets, points = np.array([[0, 1], [1, 0]]), np.array([2, 1])
    write_scan_effects(str(tmp_path / "x"), ["a", "b"], ["A", "B", "C"], ["s0", "s1"], ["intercept"], ["1", "2", "3"],
                       [0.5, 1.5, 0.25, 2.0], targets, points, result, 6.0)
    lines = open(tmp_path / "x.scan.effects.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\trank\teffect_A\tse_A\teffect_B\tse_B\teffect_C\tse_C"
    assert lines[1] == "a\t2\t0.25\t7.25\t2\t0.1\t0.01\t-0.3\t0.02\t0.2\t0.3333333333333333"
    assert lines[2] == "b\t1\t1.5\tinf\t1\t1e-17\t0.0\t2.5\t1.5\t-2.5\t1.5"
    for line in lines[1:]:
        fields = line.split("\t")
        assert [repr(float(v)) for v in fields[2:4] + fields[5:]] == fields[2:4] + fields[5:]
    z = np.load(tmp_path / "x.scan.effects.npz")
    assert sorted(z.files) == ["covariates", "effect", "founders", "lod", "min_lod", "phenotypes", "points", "position", "rank", "samples",
                               "se", "sigma2", "target_chromosome", "target_phenotype", "targets"]
    assert z["founders"].tolist() == ["A", "B", "C"] and z["targets"].tolist() == ["a", "b"] and z["target_chromosome"].tolist() == ["2", "1"]
    np.testing.assert_array_equal(z["position"], [0.25, 1.5])
    for key in result:
        np.testing.assert_array_equal(z[key], result[key])
    # no labels: the founders' indices; no target: the header alone
    empty = {"effect": np.zeros((0, 3)), "se": np.zeros((0, 3)), "lod": np.zeros(0), "sigma2": np.zeros(0), "rank": np.zeros(0, dtype=np.int32)}
    write_scan_effects(str(tmp_path / "e"), ["a", "b"], range(3), ["s0", "s1"], ["intercept"], ["1", "2", "3"], [0.5, 1.5, 0.25, 2.0],
                       np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), empty, 6.0)
    assert open(tmp_path / "e.scan.effects.tsv").read() == "#phenotype\tchromosome\tposition\tlod\trank\teffect_0\tse_0\teffect_1\tse_1\teffect_2\tse_2\n"
    assert np.load(tmp_path / "e.scan.effects.npz")["effect"].shape == (0, 3)
