"""The host side of the scan's permutation thresholds (gbrs_amd/scan.py) and the numpy restatement the
device is held against (tests/scan_perm_restate.py): no GPU."""
import numpy as np
import pytest

import scan_cases as cases
import scan_perm_restate as restate


@pytest.mark.parametrize("n", [1, 3, 64, 65, 300, 256, 257, 512, 513])
def test_every_row_is_a_permutation_that_depends_on_seed_row_and_n_alone(n):
    few, many = restate.permutations(restate.SEED, 3, n), restate.permutations(restate.SEED, 8, n)
    assert many.dtype == np.int32 and many.shape == (8, n)
    for row in many:
        np.testing.assert_array_equal(np.sort(row), np.arange(n))
    np.testing.assert_array_equal(many[:3], few)
    if n >= 64:
        other = restate.permutations(restate.SEED_HIGH, 8, n)
        assert not (other == many).all(axis=1).any()
        assert not (restate.permutations(restate.SEED_HIGH & 0xFFFFFFFF, 8, n) == other).all(axis=1).any()      # the upper word counts
        assert len({row.tobytes() for row in many}) == 8


def test_ties_between_keys_go_to_the_lower_sample(monkeypatch):
    """All keys equal: the identity.  Keys that only differ in their lower word are ordered by it."""
    monkeypatch.setattr(restate, "philox4x32_10", lambda counter, key: [np.zeros(5, dtype=np.uint64)] * 4)
    np.testing.assert_array_equal(restate.permutations(0, 2, 5), [np.arange(5)] * 2)
    low = np.array([3, 1, 1, 0, 2], dtype=np.uint64)
    monkeypatch.setattr(restate, "philox4x32_10", lambda counter, key: [np.ones(5, dtype=np.uint64), low, low, low])
    np.testing.assert_array_equal(restate.permutations(0, 1, 5)[0], [4, 1, 2, 0, 3])


@pytest.mark.parametrize("case", [c for c in restate.ORDINARY if c[2] == 1], ids=cases.case_id)
def test_with_the_intercept_alone_it_is_a_plain_scan_of_the_permuted_phenotypes(case):
    D, Z, Y, _ = cases.build(case)
    perm, rule, _ = restate.expected(case)
    plain = np.concatenate([cases.scan_rule(D, Z, Y[row])[0][:, None] for row in perm], axis=1)     # [P, B, M]
    worst = cases.deviation(rule, plain.reshape(rule.shape))
    print(f"DEVIATION permuted columns against scan_rule(Y[perm]), {cases.case_id(case)}: {worst:.3g}")
    assert worst <= cases.CPU_HEADROOM * restate.MEASURED_FLOOR_PERM


@pytest.mark.parametrize("case", restate.ORDINARY + restate.ORDINARY_LARGE, ids=cases.case_id)
def test_the_two_host_routes_agree_on_the_permuted_columns(case):
    """Within the floor over ORDINARY, a large case within its own recorded figure (measured_floor_perm is
    MEASURED_FLOOR_PERM for every case of ORDINARY), with the headroom."""
    perm, rule, lstsq = restate.expected(case)
    assert perm.shape == (restate.N_PERM, case[1]) and rule.shape == lstsq.shape == (case[3] * restate.N_PERM, sum(case[4]))
    worst = cases.deviation(rule, lstsq)
    print(f"DEVIATION scan_rule against scan_lstsq on permuted columns, {cases.case_id(case)}: {worst:.3g}, largest LOD "
          f"{rule[np.isfinite(rule)].max():.3g}")
    assert worst <= cases.CPU_HEADROOM * restate.measured_floor_perm(case)
    by_rule, by_lstsq = restate.expected_max(case)
    assert by_rule.shape == (case[3], restate.N_PERM) and cases.deviation(by_rule, by_lstsq) <= worst


def test_the_two_host_routes_agree_on_the_columns_of_the_event_ring():
    """All 4,608 columns of the pass that wraps the device's event ring, not only their maxima."""
    perm, rule, lstsq = restate.expected_ring()
    assert perm.shape == (restate.RING_PERM, restate.RING[1])
    assert rule.shape == lstsq.shape == (restate.RING_PHENO * restate.RING_PERM, sum(restate.RING[4])) and rule.shape[0] > 8 * 512
    np.testing.assert_array_equal(perm[:restate.N_PERM], restate.expected(restate.RING)[0])
    worst = cases.deviation(rule, lstsq)
    print(f"DEVIATION scan_rule against scan_lstsq on the event ring's columns: {worst:.3g}, largest LOD {rule.max():.3g}")
    assert np.isfinite(rule).all() and worst <= cases.CPU_HEADROOM * restate.MEASURED_RING


def test_the_ordinary_cases_are_those_with_more_than_one_residual_degree():
    left_out = [c for c in cases.CASES if c not in restate.ORDINARY]
    assert all(n == c + H for H, n, c, _, _ in left_out) and len(left_out) == 6 and len(restate.ORDINARY) == 9
    assert {c[0] for c in restate.ORDINARY} == {2, 3, 4, 8, 9, 10, 16} and {c[2] for c in restate.ORDINARY} == {1, 2, 4}
    assert any(65 in c[4] for c in restate.ORDINARY)
    left_out = [c for c in cases.LARGE_CASES if c not in restate.ORDINARY_LARGE]
    assert [(H, n, c) for H, n, c, _, _ in left_out] == [(17, 19, 2), (16, 80, 64)] and len(restate.ORDINARY_LARGE) == 7
    assert sorted(restate.MEASURED_PERM_LARGE) == sorted(cases.case_id(c) for c in restate.ORDINARY_LARGE)
    assert sorted(cases.MEASURED_LARGE) == sorted(cases.case_id(c) for c in cases.LARGE_CASES)
    assert not set(cases.LARGE_CASES) & set(cases.CASES)


def test_thresholds_are_order_statistics():
    from gbrs_amd.scan import perm_thresholds
    rng = np.random.default_rng(3)
    for B, k05, k10 in ((1, 1, 1), (19, 19, 18), (20, 19, 18), (1000, 950, 900)):       # ceil((1 - alpha) B), 1-based
        values = rng.permutation(B).astype(float)                                        # the k-th smallest is k - 1
        got = perm_thresholds(np.stack([values, values + 0.5]), [0.05, 0.1])
        np.testing.assert_array_equal(got, [[k05 - 1, k10 - 1], [k05 - 0.5, k10 - 0.5]])
    assert perm_thresholds([[1.0, np.inf, 0.5, 2.0]], [0.05, 0.3, 0.5, 0.9]).tolist() == [[np.inf, 2.0, 1.0, 0.5]]
    assert perm_thresholds(np.full((1, 20), np.inf), [0.05]).tolist() == [[np.inf]]
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="level"):
            perm_thresholds([[1.0, 2.0]], [bad])
    with pytest.raises(ValueError, match="shape"):
        perm_thresholds(np.zeros((2, 0)), [0.05])


def test_pvalues_count_the_permutations_at_or_above_the_peak():
    from gbrs_amd.scan import perm_pvalues
    perm_max = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, np.inf, 5.0]])
    peak = np.array([[3.0, 0.5, np.nan], [np.inf, 6.0, 0.0]])
    got = perm_pvalues(perm_max, peak)
    np.testing.assert_array_equal(got, [[3 / 5, 5 / 5, np.nan], [2 / 5, 2 / 5, 5 / 5]])   # 3.0 >= 3.0 and inf >= inf count
    assert perm_pvalues(perm_max, np.array([[4.5], [np.inf]])).tolist() == [[1 / 5], [2 / 5]]
    masked = perm_pvalues(perm_max, peak, selected=[True, False, True])
    np.testing.assert_array_equal(masked, [[3 / 5, np.nan, np.nan], [2 / 5, np.nan, 5 / 5]])
    with pytest.raises(ValueError, match="shape"):
        perm_pvalues(perm_max, peak[:1])


def test_the_permutation_options_and_their_refusals(tmp_path):
    from gbrs_amd.scan import check_scan_args, perm_options, perm_plan
    assert perm_options() is None
    assert perm_options(20) == {"n_perm": 20, "seed": 0, "alphas": [0.05, 0.1], "chromosomes": None, "pheno_file": None}
    got = perm_options(5, (1 << 64) - 1, "0.01, 0.2", "1,X", "names.txt")
    assert got == {"n_perm": 5, "seed": (1 << 64) - 1, "alphas": [0.01, 0.2], "chromosomes": ["1", "X"], "pheno_file": "names.txt"}
    assert perm_options(5, scan_perm_alpha=[0.5], scan_perm_chromosomes=[2])["chromosomes"] == ["2"]
    common = dict(grid_file="g.txt", cohort=True)
    check_scan_args("p.tsv", scan_perms=10, scan_perm_seed=4, scan_perm_alpha="0.05", scan_perm_chromosomes="1", **common)
    with pytest.raises(RuntimeError, match="--scan-perms needs --scan-pheno"):
        check_scan_args(scan_perms=10, **common)
    for kw, name in ((dict(scan_perm_seed=1), "--scan-perm-seed"), (dict(scan_perm_alpha="0.05"), "--scan-perm-alpha"),
                     (dict(scan_perm_chromosomes="1"), "--scan-perm-chromosomes"), (dict(scan_perm_pheno="f"), "--scan-perm-pheno")):
        with pytest.raises(RuntimeError, match=f"{name} needs --scan-perms"):
            check_scan_args("p.tsv", **kw, **common)
    for bad in (0, -3, 2.5):
        with pytest.raises(RuntimeError, match="--scan-perms must be a whole number of at least 1"):
            check_scan_args("p.tsv", scan_perms=bad, **common)
    for bad in ("0", "1", "0.05,1.5", "-0.1", "nan", "", "0.05,,0.1", "five"):
        with pytest.raises(RuntimeError, match="--scan-perm-alpha"):
            check_scan_args("p.tsv", scan_perms=10, scan_perm_alpha=bad, **common)
    with pytest.raises(RuntimeError, match="--scan-perm-seed must lie in"):
        perm_options(10, -1)
    with pytest.raises(RuntimeError, match="--scan-perm-chromosomes must be names"):
        perm_options(10, scan_perm_chromosomes="1,,2")
    # names against the table and the grid
    names = tmp_path / "names.txt"
    names.write_text("c\n\na\n")
    phenotypes, chroms = ["a", "b", "c"], ["1", "2", "X"]
    assert perm_plan(perm_options(3), phenotypes) == ([0, 1, 2], None)
    columns, mask = perm_plan(perm_options(3, scan_perm_chromosomes="X,1", scan_perm_pheno=str(names)), phenotypes, chroms)
    assert columns == [0, 2] and mask.tolist() == [True, False, True]                      # the table's order, not the file's
    with pytest.raises(RuntimeError, match="--scan-perm-chromosomes: 7 is no chromosome of the grid"):
        perm_plan(perm_options(3, scan_perm_chromosomes="1,7"), phenotypes, chroms)
    names.write_text("a\nzz\n")
    with pytest.raises(RuntimeError, match="zz is no phenotype of the table"):
        perm_plan(perm_options(3, scan_perm_pheno=str(names)), phenotypes, chroms)
    names.write_text("\n")
    with pytest.raises(RuntimeError, match="no phenotype is named"):
        perm_plan(perm_options(3, scan_perm_pheno=str(names)), phenotypes)


def test_the_files_with_permutations(tmp_path):
    """write_scan with a permutation result: the perm_* arrays and the two columns, NA where nothing was permuted; without
    one, the files of test_scan_cpu.test_the_peak_file byte for byte."""
    from gbrs_amd.scan import perm_pvalues, perm_thresholds, write_scan
    peak = np.array([[1.0, 5.0, np.nan], [0.5, 0.5, np.nan]])
    index = np.array([[0, 2, -1], [1, 3, -1]])
    result = {"peak_lod": peak, "peak_index": index, "lod": np.zeros((2, 4))}
    args = (["a", "b"], ["s0", "s1"], ["intercept"], ["1", "1", "2", "2"], [0.5, 1.5, 0.25, 2.0], ["1", "2", "3"], result, [1, 1, 1, 1])
    perm_max = np.array([[0.25, 6.0, 1.0, 0.75]])
    perm = {"perm_max": perm_max, "columns": [0], "mask": np.array([False, True, True]), "alphas": [0.25, 0.5], "seed": 1 << 63}
    write_scan(str(tmp_path / "x"), *args, min_lod=0.75, perm=perm)
    lines = open(tmp_path / "x.scan.peaks.tsv").read().splitlines()
    assert lines == ["#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tpvalue\tthreshold_0.25",
                     "a\t1\t0.5\t1.0\t0\tNA\tNA", "a\t2\t0.25\t5.0\t1\t0.4\t1.0"]
    z = np.load(tmp_path / "x.scan.npz")
    assert z["perm_phenotypes"].tolist() == ["a"] and z["perm_chromosomes"].tolist() == ["2", "3"] and z["perm_seed"] == 1 << 63
    np.testing.assert_array_equal(z["perm_max"], perm_max)
    np.testing.assert_array_equal(z["perm_alpha"], [0.25, 0.5])
    np.testing.assert_array_equal(z["perm_threshold"], perm_thresholds(perm_max, [0.25, 0.5]))
    assert z["perm_threshold"].tolist() == [[1.0, 0.75]] and perm_pvalues(perm_max, peak[:1])[0, 1] == 0.4
    write_scan(str(tmp_path / "y"), *args, min_lod=0.75)
    write_scan(str(tmp_path / "w"), *args, min_lod=0.75, perm=None)
    assert open(tmp_path / "y.scan.peaks.tsv").read().splitlines() == [line.rsplit("\t", 2)[0] for line in lines]
    assert sorted(np.load(tmp_path / "y.scan.npz").files) == sorted(set(z.files) - {f for f in z.files if f.startswith("perm_")})
    for suffix in ("scan.npz", "scan.peaks.tsv"):
        assert open(tmp_path / f"y.{suffix}", "rb").read() == open(tmp_path / f"w.{suffix}", "rb").read()
