"""The host side of the genome scan (gbrs_amd/scan.py) and the two host computations the device is held
against (tests/scan_cases.py): no GPU."""
import numpy as np
import pytest

import scan_cases as cases


@pytest.mark.parametrize("case", cases.CASES + cases.LARGE_CASES, ids=cases.case_id)
def test_the_rule_agrees_with_lstsq(case):
    """The restatement of the rule against np.linalg.lstsq, which knows nothing of it: the LODs within the case's measured floor (with headroom), the
    ranks equal, and the constructed points have the ranks their construction says."""
    H = case[0]
    _, _, _, special = cases.build(case)
    lod, rank, _, lod_ls, rank_ls = cases.expected(case)
    worst = cases.deviation(lod, lod_ls)
    print(f"DEVIATION scan_rule against scan_lstsq, {cases.case_id(case)}: {worst:.3g}, largest LOD {lod[np.isfinite(lod)].max():.3g}")
    assert worst <= cases.cpu_bound(case)
    np.testing.assert_array_equal(rank, rank_ls)
    ordinary = np.ones(len(rank), dtype=bool)
    for name in ("zero", "equal", "last"):
        if name in special:
            assert rank[special[name]] == H - 2, name
            ordinary[special[name]] = False
    assert (rank[ordinary] == H - 1).all()
    assert rank[special["twin"]] == rank[special["twin"] - 1]
    np.testing.assert_array_equal(lod[:, special["twin"]], lod[:, special["twin"] - 1])
    if case[1] > case[2] + H:             # with one residual degree of freedom every full-rank point has a large LOD
        assert cases.peaks(lod, case[4])[1][0, -1] == special["twin"] - 1         # phenotype 0: the first of the tie


def test_no_fixture_has_an_undecided_pivot():
    """A pivot ratio in [1e-13, 1e-7] could flip a rank by rounding: the share of such grid points is 0, the exact-zero
    and exact-duplicate constructions give G_jj = 0 or ratios near 1e-16."""
    lo, hi = cases.UNDECIDED
    undecided = total = 0
    smallest_kept, largest_skipped = np.inf, 0.0
    for case in cases.CASES + cases.LARGE_CASES:
        ratios = cases.expected(case)[2]
        with np.errstate(invalid="ignore"):
            undecided += int(((ratios >= lo) & (ratios <= hi)).any(axis=1).sum())
            kept = ratios[ratios > cases.PIVOT]
            skipped = np.abs(ratios[ratios <= cases.PIVOT])
        total += len(ratios)
        smallest_kept = min(smallest_kept, kept.min(initial=np.inf))
        largest_skipped = max(largest_skipped, skipped.max(initial=0.0))
    print(f"pivot ratios over {total} grid points: smallest kept {smallest_kept:.3g}, largest skipped {largest_skipped:.3g}")
    assert undecided == 0 and smallest_kept > hi and largest_skipped < lo


def test_factor_skips_what_the_rule_says():
    G = np.array([[4.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 0.0]])           # column 1 = column 0 / 2, column 2 absent
    L, keep, ratio = cases.factor(G)
    assert keep.tolist() == [True, False, False] and ratio[1] == 0.0 and np.isnan(ratio[2])
    np.testing.assert_array_equal(L, [[2.0, 0, 0], [0, 0, 0], [0, 0, 0]])
    L, keep, _ = cases.factor(np.array([[0.0, 0.0], [0.0, 9.0]]))                 # a skipped column takes no part later
    assert keep.tolist() == [False, True] and L[1, 1] == 3.0 and L[1, 0] == 0.0


def test_rankz():
    from gbrs_amd.scan import rankz
    from statistics import NormalDist
    inv = NormalDist().inv_cdf
    got = rankz([3.0, 1.0, 2.0, 1.0, 5.0])                                        # the two 1.0 share rank 1.5
    np.testing.assert_array_equal(got, [inv(3.5 / 5), inv(1.0 / 5), inv(2.5 / 5), inv(1.0 / 5), inv(4.5 / 5)])
    assert got[1] == got[3] and got[2] == 0.0
    np.testing.assert_array_equal(rankz([7.0, 7.0, 7.0]), [0.0, 0.0, 0.0])        # all tied: the middle rank, Phi^-1(1/2)
    x = np.random.default_rng(0).normal(size=50)
    z = rankz(x)
    assert (np.argsort(z) == np.argsort(x)).all() and abs(z.sum()) < 1e-12
    np.testing.assert_array_equal(rankz(np.exp(x)), z)                            # it sees the order alone


def test_covariate_basis_and_its_refusals():
    from gbrs_amd.scan import covariate_basis
    rng = np.random.default_rng(1)
    z = np.column_stack([np.ones(12), rng.normal(size=(12, 2))])
    q = covariate_basis(z)
    assert q.shape == (12, 3) and q.flags.c_contiguous
    np.testing.assert_allclose(q.T @ q, np.eye(3), atol=1e-14)
    np.testing.assert_allclose(q @ (q.T @ z), z, atol=1e-13)
    dup = np.column_stack([z, z[:, 1] - 2.0 * z[:, 0]])
    with pytest.raises(ValueError, match=r"covariate column 3 \(batch\) is a linear combination"):
        covariate_basis(dup, ["intercept", "sex", "age", "batch"])
    with pytest.raises(ValueError, match="covariate column 2 is a linear combination"):
        covariate_basis(np.column_stack([np.ones(12), z[:, 1], 3.0 * np.ones(12)]))
    with pytest.raises(ValueError, match="first covariate column must be the intercept"):
        covariate_basis(z[:, 1:])
    bad = z.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match=r"covariate column 2 \(age\) holds a value that is not finite \(sample 5\)"):
        covariate_basis(bad, ["intercept", "sex", "age"])
    with pytest.raises(ValueError, match="too few"):
        covariate_basis(z[:2])


def test_check_scan_args():
    from gbrs_amd.scan import check_scan_args
    check_scan_args()
    check_scan_args("p.tsv", "c.tsv", True, "out", 3.0, True, grid_file="g.txt", cohort=True)
    for kw, name in ((dict(scan_covar="c.tsv"), "--scan-covar"), (dict(scan_rankz=True), "--scan-rankz"),
                     (dict(scan_out="x"), "--scan-out"), (dict(scan_min_lod=1.0), "--scan-min-lod"),
                     (dict(scan_lod_matrix=True), "--scan-lod-matrix")):
        with pytest.raises(RuntimeError, match=f"{name} needs --scan-pheno"):
            check_scan_args(**kw, grid_file="g.txt", cohort=True)
    with pytest.raises(RuntimeError, match="--scan-pheno needs --sample-file: one sample"):
        check_scan_args("p.tsv", grid_file="g.txt", cohort=False)
    with pytest.raises(RuntimeError, match="--scan-pheno needs --grid-file"):
        check_scan_args("p.tsv", cohort=True)
    for bad in (-1.0, float("nan")):
        with pytest.raises(RuntimeError, match="--scan-min-lod must be"):
            check_scan_args("p.tsv", scan_min_lod=bad, grid_file="g.txt", cohort=True)


def test_the_table_readers(tmp_path):
    from gbrs_amd.scan import read_scan_covar, read_scan_pheno, scan_design
    p = tmp_path / "pheno.tsv"
    p.write_text("id\tg1\tg2\n# a comment\ns0\t1.5\t-2\n\ns1\t3e-1\t4\ns3\t0\t1\n")
    names, rows = read_scan_pheno(str(p))
    assert names == ["g1", "g2"] and list(rows) == ["s0", "s1", "s3"] and rows["s1"].tolist() == [0.3, 4.0]
    c = tmp_path / "covar.tsv"
    c.write_text("id\tsex\ns0\t0\ns1\t1\ns2\t1\n")
    covar = read_scan_covar(str(c))
    kept, y, z, znames = scan_design(["s0", "s1", "s2", "s3"], (names, rows), covar)
    assert kept == [0, 1] and znames == ["intercept", "sex"]                      # s2 has no phenotype row, s3 no covariate row
    np.testing.assert_array_equal(y, [[1.5, -2.0], [0.3, 4.0]])
    np.testing.assert_array_equal(z, [[1.0, 0.0], [1.0, 1.0]])
    kept, y, z, znames = scan_design(["s3", "s0"], (names, rows))
    assert kept == [0, 1] and z.tolist() == [[1.0], [1.0]] and y[:, 0].tolist() == [0.0, 1.5]
    for text, message in (("name\tg1\ns0\t1\n", "header must be id"), ("id\n", "header must be id"),
                          ("id\tg1\tg1\ns0\t1\t2\n", "named twice"), ("id\tg1\ns0\t1\t2\n", "line 2: 2 values for 1 phenotype"),
                          ("id\tg1\ns0\t1\ns0\t2\n", "line 3: id s0 is already on line 2"),
                          ("id\tg1\ns0\tabc\n", "line 2: could not convert")):
        p.write_text(text)
        with pytest.raises(RuntimeError, match=message):
            read_scan_pheno(str(p))


def test_the_peak_file(tmp_path):
    from gbrs_amd.scan import write_scan
    peak = np.array([[1.0, 5.0, np.nan], [0.5, 0.5, np.nan]])
    index = np.array([[0, 2, -1], [1, 3, -1]])
    result = {"peak_lod": peak, "peak_index": index, "lod": np.zeros((2, 4))}
    write_scan(str(tmp_path / "x"), ["a", "b"], ["s0", "s1"], ["intercept"], ["1", "1", "2", "2"], [0.5, 1.5, 0.25, 2.0],
               ["1", "2", "3"], result, [1, 1, 1, 1], min_lod=0.75)
    lines = open(tmp_path / "x.scan.peaks.tsv").read().splitlines()
    assert lines == ["#phenotype\tchromosome\tposition\tlod\tgenome_wide_max", "a\t1\t0.5\t1.0\t0", "a\t2\t0.25\t5.0\t1"]
    z = np.load(tmp_path / "x.scan.npz")
    assert sorted(z.files) == sorted(["phenotypes", "samples", "covariates", "chrom", "pos", "rank", "peak_lod", "peak_index", "lod"])
    assert z["phenotypes"].tolist() == ["a", "b"] and z["peak_index"].tolist() == index.tolist()
