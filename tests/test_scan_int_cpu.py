"""The two host routes of the scan with interactive covariates against each other (tests/scan_int_cases.py),
the condition under which they may be compared, the options of the two commands and the writers on a rule-made result.
No GPU."""
import numpy as np
import pytest

import scan_cases as base
import scan_int_cases as cases


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_two_routes_agree(case):
    """Within CPU_HEADROOM times the recorded figure per output; the ranks agree at every grid point and no pivot ratio lies
    in the undecided band; lod_int by the rule is never negative and never NaN, and the full model explains no less than
    the additive one.  The figures are printed for the record."""
    (rule, rank_full, rank_add, ratios), (lstsq, lstsq_full, lstsq_add) = cases.expected(case)
    assert not ((ratios > base.UNDECIDED[0]) & (ratios < base.UNDECIDED[1])).any()
    np.testing.assert_array_equal(rank_full, lstsq_full)
    np.testing.assert_array_equal(rank_add, lstsq_add)
    measured = [cases.deviation(rule[key], lstsq[key]) for key in cases.KEYS]
    print(f"'{cases.case_id(case)}': ({', '.join(f'{v:.3g}' for v in measured)}),")
    for key, value in zip(cases.KEYS, measured):
        assert value <= cases.cpu_bound(case, key), key
    assert (rule["lod_int"] >= 0.0).all()
    assert (rule["lod_full"] >= rule["lod_add"]).all()


def test_the_cases_cover_what_they_are_there_for():
    assert {cases.hpi_of(c) for c in cases.CASES} == {16, 32, 64}
    rows = lambda c: (8 if c[0] <= 9 else 16) + c[3] * (c[0] - 1)
    assert {16, 32, 64} <= {rows(c) for c in cases.CASES}                          # each HPI once exactly full
    assert sum(cases.one_degree(c) for c in cases.CASES) == 4
    assert set(cases.MEASURED_INT) == {cases.case_id(c) for c in cases.CASES}
    for key in cases.KEYS:                                                          # the floor is the worst of the ordinary cases
        k = cases.KEYS.index(key)
        assert cases.MEASURED_FLOOR[key] == max(cases.MEASURED_INT[cases.case_id(c)][k] for c in cases.CASES
                                                if not cases.one_degree(c) and c[1] <= 256)


def test_the_special_points_lose_a_column_in_each_block():
    """At `zero` founder 0's column and its products are zero; at `last` the additive columns add up to the intercept and
    each block of products to its covariate, which is in the covariates' span."""
    case = cases.CASES[5]
    H, n, c, k, P, points = case
    special = cases.build(case)[4]
    _, rank_full, rank_add, _ = cases.expected(case)[0]
    for name in ("zero", "equal", "last"):
        assert rank_add[special[name]] == H - 2 and rank_full[special[name]] == (H - 2) * (1 + k)
    assert rank_add[0] == H - 1 and rank_full[0] == (H - 1) * (1 + k)


def test_the_option_checks():
    from gbrs_amd.scan import check_scan_args, intcovar_options, intcovar_plan
    assert intcovar_options() is None
    assert intcovar_options(None, "c.tsv", "loco") is None
    assert intcovar_options("sex", "c.tsv") == ["sex"]
    assert intcovar_options("sex, diet", "c.tsv") == ["sex", "diet"]
    for args, message in ((("sex",), "--scan-intcovar needs --scan-covar"),
                          (("sex", "c.tsv", "loco"), "--scan-intcovar cannot be combined with --scan-kinship"),
                          (("sex,sex", "c.tsv"), "--scan-intcovar names sex twice"),
                          (("sex,,diet", "c.tsv"), "--scan-intcovar must be covariate names"),
                          (("", "c.tsv"), "--scan-intcovar must be covariate names")):
        with pytest.raises(RuntimeError, match=message):
            intcovar_options(*args)
    assert intcovar_plan(["diet", "sex"], ["sex", "batch", "diet"]) == [3, 1]
    with pytest.raises(RuntimeError, match="--scan-intcovar: age is not a column of --scan-covar"):
        intcovar_plan(["sex", "age"], ["sex", "batch"])
    check_scan_args("p.tsv", "c.tsv", grid_file="g.txt", cohort=True, scan_intcovar="sex", scan_perms=10, scan_effects=True)
    for how, message in ((dict(scan_intcovar="sex", scan_covar="c.tsv"), "--scan-covar needs --scan-pheno"),
                         (dict(scan_pheno="p.tsv", scan_intcovar="sex"), "--scan-intcovar needs --scan-covar"),
                         (dict(scan_pheno="p.tsv", scan_covar="c.tsv", scan_intcovar="sex,sex"), "--scan-intcovar names sex twice"),
                         (dict(scan_pheno="p.tsv", scan_covar="c.tsv", scan_intcovar="sex", scan_kinship="loco"),
                          "--scan-intcovar cannot be combined with --scan-kinship")):
        with pytest.raises(RuntimeError, match=message):
            check_scan_args(grid_file="g.txt", cohort=True, **how)


def test_the_commands_take_the_option_and_refuse_before_a_file_is_read(tmp_path, caplog):
    from gbrs_amd import cli
    f = str(tmp_path / "file")
    open(f, "w").close()
    missing = str(tmp_path / "missing")                                             # never opened: the refusal comes first
    for command, covar in ((["reconstruct", "--sample-file", f, "-t", f, "--grid-file", f, "--scan-pheno", f], "--scan-covar"),
                           (["scan", "--dosage-list", f, "--grid-file", f, "--pheno", f], "--covar")):
        args = cli.build_parser().parse_args(command + [covar, f, "--scan-intcovar", "sex,diet"])
        assert args.scan_intcovar == "sex,diet"
        assert cli.build_parser().parse_args(command).scan_intcovar is None
        for extra, message in ((["--scan-intcovar", "sex"], "--scan-intcovar needs --scan-covar"),
                               ([covar, f, "--scan-intcovar", "sex,sex"], "--scan-intcovar names sex twice"),
                               ([covar, f, "--scan-intcovar", "sex", "--scan-kinship", "loco"],
                                "--scan-intcovar cannot be combined with --scan-kinship")):
            caplog.clear()
            with caplog.at_level("ERROR", logger="gbrs"):
                cli.main(command + ["--scan-out", missing] + extra)
            assert any(message in r.getMessage() for r in caplog.records), (command[0], extra, [r.getMessage() for r in caplog.records])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["file"]


def test_an_unknown_name_is_refused_before_a_dosage_table_is_read(tmp_path, caplog):
    """`gbrs scan`: the covariate table's header is needed to know the names, so this refusal follows the tables of
    phenotypes and covariates - and comes before any dosage table (the list names none that exists) and before the device."""
    from gbrs_amd import cli
    (tmp_path / "grid.txt").write_text("marker\tchr\tbp\tcM\nm0\t1\t0\t0.0\nm1\t1\t1\t1.0\nm2\t1\t2\t2.0\n")
    (tmp_path / "list.tsv").write_text(f"a\t{tmp_path / 'nowhere.tsv'}\n")
    (tmp_path / "pheno.tsv").write_text("id\ty\na\t1.0\n")
    (tmp_path / "covar.tsv").write_text("id\tsex\na\t1.0\n")
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(["scan", "--dosage-list", str(tmp_path / "list.tsv"), "--grid-file", str(tmp_path / "grid.txt"), "--pheno",
                  str(tmp_path / "pheno.tsv"), "--covar", str(tmp_path / "covar.tsv"), "--scan-intcovar", "age",
                  "--scan-out", str(tmp_path / "out")])
    assert any("--scan-intcovar: age is not a column of --scan-covar" in r.getMessage() for r in caplog.records), \
        [r.getMessage() for r in caplog.records]
    assert not list(tmp_path.glob("out*"))


def test_the_writers_on_a_rule_made_result(tmp_path):
    """write_scan_int on int_rule's numbers: the archive's members and the peaks file line by line."""
    from gbrs_amd.scan import write_scan_int
    case = cases.CASES[1]
    H, n, c, k, P, points = case
    rule, rank_full, rank_add, _ = cases.expected(case)[0]
    result = dict(rule)
    result["peak_full"], result["peak_full_index"] = base.peaks(rule["lod_full"], points)
    result["peak_int"], result["peak_int_index"] = base.peaks(rule["lod_int"], points)
    rows = np.arange(P)[:, None]
    result["peak_full_add"] = rule["lod_add"][rows, result["peak_full_index"]]
    result["peak_full_int"] = rule["lod_int"][rows, result["peak_full_index"]]
    M = sum(points)
    phenotypes, samples = [f"y{p}" for p in range(P)], [f"s{i}" for i in range(n)]
    chrom_names = ["1", "2", "X"]
    chrom, pos = np.repeat(chrom_names, points), np.arange(M) * 0.5
    min_lod = float(np.median(result["peak_full"]))
    write_scan_int(str(tmp_path / "x"), phenotypes, samples, ["intercept", "sex"], ["sex"], chrom, pos, chrom_names, result,
                   rank_full, rank_add, min_lod)
    z = np.load(tmp_path / "x.scan.int.npz")
    assert z.files == ["phenotypes", "samples", "covariates", "intcovar", "chrom", "pos", "rank_full", "rank_add", "peak_full",
                       "peak_full_index", "peak_full_add", "peak_int", "peak_int_index", "lod_full", "lod_add", "lod_int"]
    assert list(z["intcovar"]) == ["sex"] and list(z["covariates"]) == ["intercept", "sex"]
    for key in ("rank_full", "rank_add"):
        np.testing.assert_array_equal(z[key], {"rank_full": rank_full, "rank_add": rank_add}[key])
    for key in cases.KEYS + ("peak_full", "peak_full_index", "peak_full_add", "peak_int", "peak_int_index"):
        np.testing.assert_array_equal(z[key], result[key])
    lines = open(tmp_path / "x.scan.int.peaks.tsv").read().splitlines()
    assert lines[0] == ("#phenotype\tchromosome\tposition\tlod_full\tlod_add\tlod_int\tdf_full\tdf_add\tint_peak_position"
                        "\tint_peak_lod")
    want = []
    for p in range(P):
        for ci in range(3):
            if result["peak_full"][p, ci] >= min_lod:
                m, mi = result["peak_full_index"][p, ci], result["peak_int_index"][p, ci]
                want.append("\t".join([phenotypes[p], chrom_names[ci], repr(float(pos[m])), repr(float(rule["lod_full"][p, m])),
                                       repr(float(rule["lod_add"][p, m])), repr(float(rule["lod_int"][p, m])),
                                       str(int(rank_full[m])), str(int(rank_add[m])), repr(float(pos[mi])),
                                       repr(float(rule["lod_int"][p, mi]))]))
    assert 0 < len(want) < 3 * P and lines[1:] == want
    del result["lod_full"], result["lod_add"], result["lod_int"]
    write_scan_int(str(tmp_path / "y"), phenotypes, samples, ["intercept", "sex"], ["sex"], chrom, pos, chrom_names, result,
                   rank_full, rank_add, min_lod)
    assert np.load(tmp_path / "y.scan.int.npz").files == z.files[:-3]
    assert open(tmp_path / "y.scan.int.peaks.tsv").read().splitlines() == lines
