"""The host side of the mixed-model genome scan (no GPU): the two host routes of tests/scan_lmm_cases.py
against each other within the recorded floors, the conditions the cases must meet, rotation invariance against §27's rule,
the kinship's scale, and the options of the commands."""
import numpy as np
import pytest

import scan_cases as base
import scan_lmm_cases as cases

ALL = cases.CASES + cases.LARGE_CASES


@pytest.mark.parametrize("case", ALL, ids=cases.case_id)
def test_the_two_host_routes_agree_within_the_recorded_floor(case):
    rule, gls = cases.expected(case)
    measured = cases.deviation(rule["lod"], gls)
    print(f"{cases.case_id(case)}: measured {measured:.3g}, recorded {cases.measured_floor(case):.3g}")
    assert measured <= cases.cpu_bound(case)
    assert np.isfinite(rule["lod"]).all() and rule["lod"].max() > 3.0


@pytest.mark.parametrize("case", ALL, ids=cases.case_id)
def test_the_cases_meet_their_conditions(case):
    """Every kinship well conditioned, no weighted pivot ratio that rounding could flip, the zero founder and the equal
    founders skipped under every weight vector."""
    D, Z, Y, kinships, kin_of_chrom, special = cases.build(case)
    H = case[0]
    for K in kinships:
        lam = np.linalg.eigvalsh(K)
        assert lam.min() > cases.CASE_LAMBDA * lam.max()
        assert (K == K.T).all()
    rule, _ = cases.expected(case)
    ratios = rule["ratios"][np.isfinite(rule["ratios"])]
    assert not ((ratios > base.UNDECIDED[0]) & (ratios < base.UNDECIDED[1])).any()
    assert (rule["rank_max"] == H - 1).all()
    assert (rule["rank_min"] == (H - 2 if H >= 3 else 0)).all()         # at `zero` and `equal` one column goes
    assert set(special) == ({"zero", "equal"} if H >= 3 else {"zero"})


def test_the_case_set_has_boundary_and_interior_heritabilities():
    """At least one fitted heritability that is exactly 0.0 and at least two interior ones; every boundary optimum's
    margin f(midpoint) - f(endpoint) is printed.  With 48 golden-section steps the midpoint lies 5e-12 from the endpoint, so
    the margin is f' x 5e-12: at the usual scale of the kinship between 4e-14 and 1.1e-10, below ENDPOINT_MARGIN for every
    one of the 143 boundary pairs (more than the one in ten that was expected to fall below it); the `scaled` case, whose
    f is 1,024 times as steep at the ends, has 10 of its 14 boundary pairs above it, and those are the pairs the device
    test compares with ==.  Every pair, decided or not, is held to MEASURED_HSQ."""
    hsq = np.concatenate([cases.expected(case)[0]["hsq"].ravel() for case in cases.CASES])
    margin = np.concatenate([cases.expected(case)[0]["margin"].ravel() for case in cases.CASES])
    print(f"{(hsq == 0.0).sum()} at 0.0, {(hsq == 1.0).sum()} at 1.0, {((hsq > 0.0) & (hsq < 1.0)).sum()} interior; margins "
          f"{np.nanmin(margin):.3g} .. {np.nanmax(margin):.3g}")
    assert (hsq == 0.0).sum() >= 1 and ((hsq > 0.0) & (hsq < 1.0)).sum() >= 2
    scaled = cases.expected(cases.CASES[-1])[0]
    assert cases.CASES[-1][5] == "scaled" and (scaled["margin"] > cases.ENDPOINT_MARGIN).sum() >= 5
    interior = hsq[(hsq > 0.0) & (hsq < 1.0)]
    assert interior.min() > 1e-6 and interior.max() < 1.0 - 1e-6       # an interior optimum is not a boundary one in disguise


@pytest.mark.parametrize("case", cases.CASES[2:6], ids=cases.case_id)
def test_with_heritability_zero_the_rule_is_the_plain_scan(case):
    """h = 0: every weight is 1 and U is orthogonal, so the rotated regression is §27's.  Two restatements meet here, so
    the bound is the larger of their recorded floors: this case's and scan_cases.MEASURED_FLOOR."""
    D, Z, Y, _, kin_of_chrom, _ = cases.build(case)
    zeros = np.zeros((Y.shape[1], len(cases.decompositions(case))))
    rule = cases.lmm_rule(D, Z, Y, case[4], cases.decompositions(case), kin_of_chrom, hsq=zeros)
    plain, rank, _ = base.scan_rule(D, Z, cases.centred(Y))
    assert cases.deviation(rule["lod"], plain) <= base.CPU_HEADROOM * max(cases.measured_floor(case), base.MEASURED_FLOOR)
    assert rule["rank_min"].min() == rank.min() and rule["rank_max"].max() == rank.max()
    assert (rule["sigma2"] > 0).all()


def test_lods_do_not_depend_on_the_kinships_scale():
    worst = 0.0
    for case in cases.CASES:
        D, Z, Y, _, kin_of_chrom, _ = cases.build(case)
        scaled = [(U, 4.0 * lam) for U, lam in cases.decompositions(case)]
        got = cases.lmm_rule(D, Z, Y, case[4], scaled, kin_of_chrom)
        worst = max(worst, cases.deviation(got["lod"], cases.expected(case)[0]["lod"]))
    print(f"measured {worst:.3g}, recorded {cases.MEASURED_SCALE:.3g}")
    assert worst <= base.CPU_HEADROOM * cases.MEASURED_SCALE


def test_the_recorded_heritability_bound():
    """MEASURED_HSQ is ten times what the three perturbations move the heritability (on the two largest case sets)."""
    measured = cases.measure_hsq(cases.CASES[:2])
    print(f"measured {measured:.3g}, recorded {cases.MEASURED_HSQ:.3g}")
    assert 0.0 < measured <= cases.MEASURED_HSQ / 10 * base.CPU_HEADROOM


def test_kinship_restatement_against_the_long_double_sums():
    case = cases.CASES[3]
    D = cases.build(case)[0]
    for leave_out in (None, 0, 2):
        K, exact = cases.kinship(D, case[4], leave_out), cases.kinship_longdouble(D, case[4], leave_out)
        assert (K == K.T).all() and np.abs(K - exact).max() <= 8 * np.finfo(float).eps * np.abs(exact).max()


def test_options():
    from gbrs_amd.scan import check_scan_args, kinship_options
    assert kinship_options() is None
    assert kinship_options("loco") == {"mode": "loco", "out": False}
    assert kinship_options("overall", True) == {"mode": "overall", "out": True}
    for kwargs, message in ((dict(scan_kinship="pedigree"), "--scan-kinship must be one of loco, overall"),
                            (dict(scan_kinship_out=True), "--scan-kinship-out needs --scan-kinship"),
                            (dict(scan_kinship="loco", scan_perms=10), "--scan-perms cannot be combined with --scan-kinship"),
                            (dict(scan_kinship="loco", scan_snps=True), "--scan-snps cannot be combined with --scan-kinship"),
                            (dict(scan_kinship="loco", scan_mediate=True), "--scan-mediate cannot be combined with --scan-kinship"),
                            (dict(scan_kinship="loco", scan_effects=True), "--scan-effects cannot be combined with --scan-kinship"),
                            (dict(scan_kinship="overall", scan_lod_drop=1.5), "--scan-lod-drop cannot be combined with --scan-kinship")):
        with pytest.raises(RuntimeError, match=message):
            kinship_options(**kwargs)
    with pytest.raises(RuntimeError, match="--scan-kinship needs --scan-pheno"):
        check_scan_args(scan_kinship="loco")
    with pytest.raises(RuntimeError, match="--scan-lod-drop cannot be combined"):
        check_scan_args(scan_pheno="p.tsv", grid_file="g", cohort=True, scan_kinship="loco", scan_lod_drop=1.0)
    check_scan_args(scan_pheno="p.tsv", grid_file="g", cohort=True, scan_kinship="loco", scan_kinship_out=True)


def test_the_commands_take_the_options(tmp_path, caplog):
    """Both parsers know the two options, and a refusal comes before any file is read or any device is opened."""
    from gbrs_amd import cli
    parser = cli.build_parser()
    empty = str(tmp_path / "empty")
    open(empty, "w").close()
    files = ["--dosage-list", empty, "--grid-file", empty, "--pheno", empty]
    args = parser.parse_args(["scan"] + files + ["--scan-kinship", "loco", "--scan-kinship-out"])
    assert args.scan_kinship == "loco" and args.scan_kinship_out is True
    args = parser.parse_args(["reconstruct", "-t", empty, "--sample-file", empty, "--scan-kinship", "overall"])
    assert args.scan_kinship == "overall" and args.scan_kinship_out is False
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(["scan"] + files + ["--scan-kinship", "loco", "--scan-perms", "5"])
    assert any("--scan-perms cannot be combined with --scan-kinship" in r.getMessage() for r in caplog.records)
