"""The two host computations of the mediation pass against each other (no GPU): tests/scan_mediate_cases.py's numpy
restatement of the rule and np.linalg.lstsq, which knows nothing of the rule.  What they differ by is the
floor of the device tolerance in tests/test_scan_mediate_gpu.py; the guard ratios of every case are shown to lie outside
the band where rounding could flip `used`, so that the device tests exclude nothing."""
import numpy as np
import pytest

import scan_mediate_cases as cases

# the pairs on which lstsq cannot see a guard that the rule applies: none - a mediator in the covariates' span or in the
# span of covariates + founders adds no rank to the fit, and a target in the span of covariates + mediator leaves a
# residual at rounding, all of which mediate_lstsq reads off its fits
LSTSQ_BLIND = {}


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_two_host_routes_agree(case):
    H, n, c, T, Q, K = case
    lod0, lod, used, ratios, lod0_ls, lod_ls, used_ls = cases.expected(case)
    assert lod.shape == used.shape == (T, Q) and lod0.shape == (T,)
    band = cases.undecided(ratios)
    assert not band.any(), np.argwhere(band)[:5].tolist()
    blind = LSTSQ_BLIND.get(cases.case_id(case), [])
    differ = [tuple(p) for p in np.argwhere(used != used_ls).tolist()]
    assert sorted(differ) == sorted(blind)
    assert not np.isinf(lod[used]).any() and not np.isinf(lod_ls[used_ls]).any() and np.isfinite(lod0).all()
    assert np.isnan(lod[~used]).all()
    both = used & used_ls
    worst = max(cases.deviation(np.where(both, lod, np.nan), np.where(both, lod_ls, np.nan)), cases.deviation(lod0, lod0_ls))
    print(f"DEVIATION mediate_rule against mediate_lstsq {worst:.3g}, recorded {cases.measured_floor(case):.3g}, "
          f"{int((~used).sum())} of {used.size} pairs unused, {cases.case_id(case)}")
    assert worst <= cases.cpu_bound(case)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_planted_pairs(case):
    """The guards fire exactly where they were planted: the constant mediator for every target, the mediator in the span
    of covariates + founders at HOME for the targets at HOME alone, a target's own column.  With ten or more residual
    degrees of freedom the true mediator is rank 0 for its target and takes more than half of lod0; at n = c + H + 1 the
    one degree that is left makes every mediated LOD the overfit of H - 1 columns, the true mediator's like any other's,
    so nothing is claimed there."""
    H, n, c, T, Q, K = case
    D, Z, tgt, pts, med, planted = cases.build(case)
    lod0, lod, used, ratios = cases.expected(case)[:4]
    count, mean, sd, index, best = cases.select(lod, used, max(K, 2))
    own = np.array([[np.array_equal(tgt[:, t], med[:, q]) for q in range(Q)] for t in range(T)])
    want = ~own
    if 'constant' in planted:
        want[:, planted['constant']] = False
        want[pts == cases.HOME, planted['span']] = False
        assert own[0, planted['same']] and (pts == cases.HOME).sum() >= 3
        assert used[pts != cases.HOME, planted['span']].all()
    np.testing.assert_array_equal(used, want)
    np.testing.assert_array_equal(count, want.sum(axis=1))
    if n - c - H >= 10:
        assert index[0, 0] == planted['true'] and lod0[0] - best[0, 0] > 0.5 * lod0[0]
        if 'twin' in planted:                                                     # the tie: equal bits, the lower index first
            assert index[0, 1] == planted['twin'] and best[0, 1] == best[0, 0]
    if T >= 8:
        np.testing.assert_array_equal(lod[5], lod[0])                            # the same target twice
        assert lod0[5] == lod0[0]


def test_the_options_and_the_writer(tmp_path):
    """mediate_options' defaults and refusals, check_scan_args' refusal without the phenotypes, the targets of a peak
    table, and the two files of a handmade result: the members, one line per filled place, NA without a spread."""
    from gbrs_amd.scan import check_scan_args, mediate_options, mediation_targets, write_scan_mediation
    assert mediate_options() is None
    assert mediate_options(True) == {"min_lod": 6.0, "top": 5, "mediator_file": None}
    assert mediate_options(True, 0.5, 64, "m.tsv") == {"min_lod": 0.5, "top": 64, "mediator_file": "m.tsv"}
    for args, message in (((False, 3.0), "--scan-mediate-min-lod needs --scan-mediate"), ((False, None, 2), "--scan-mediate-top needs"),
                          ((False, None, None, "m.tsv"), "--scan-mediator-file needs"), ((True, -1.0), "not negative"),
                          ((True, None, 0), "1 .. 64"), ((True, None, 65), "1 .. 64"), ((True, None, 2.5), "whole number")):
        with pytest.raises(RuntimeError, match=message):
            mediate_options(*args)
    with pytest.raises(RuntimeError, match="--scan-mediate needs --scan-pheno"):
        check_scan_args(scan_mediate=True)
    check_scan_args("pheno.tsv", grid_file="grid.txt", cohort=True, scan_mediate=True, scan_mediate_top=3)
    peak = np.array([[7.0, np.nan, 2.0], [6.0, 9.0, 5.9]])
    index = np.array([[4, -1, 9], [0, 7, 8]])
    targets = mediation_targets(peak, index, 6.0)
    assert targets.tolist() == [[0, 0], [1, 0], [1, 1]] and mediation_targets(peak, index, 10.0).shape == (0, 2)
    points = index[targets[:, 0], targets[:, 1]]
    result = {"lod0": np.array([7.0, 6.0, 9.0]), "n_used": np.array([2, 1, 0]), "mean": np.array([4.0, np.nan, np.nan]),
              "sd": np.array([2.0, np.nan, np.nan]), "best_index": np.array([[1, 0], [0, -1], [-1, -1]]),
              "best_lod": np.array([[1.0, 5.0], [5.5, np.nan], [np.nan, np.nan]])}
    prefix = str(tmp_path / "out")
    write_scan_mediation(prefix, ["a", "b"], ["m0", "m1"], ["s0", "s1"], ["intercept"], ["1", "2", "X"], np.arange(10) * 1.5, targets,
                         points, result, 6.0)
    z = np.load(prefix + ".scan.mediation.npz")
    assert z["targets"].tolist() == ["a", "b", "b"] and z["target_chromosome"].tolist() == ["1", "1", "2"]
    assert z["points"].tolist() == [4, 0, 7] and z["position"].tolist() == [6.0, 0.0, 10.5] and "lod_med" not in z.files
    assert open(prefix + ".scan.mediation.tsv").read().splitlines() == [
        "#phenotype\tchromosome\tposition\tlod\tmediator\tlod_mediated\tdrop\tz",
        "a\t1\t6.0\t7.0\tm1\t1.0\t6.0\t-1.5", "a\t1\t6.0\t7.0\tm0\t5.0\t2.0\t0.5", "b\t1\t0.0\t6.0\tm0\t5.5\t0.5\tNA"]


def test_the_selection_restatement():
    lod = np.array([[3.0, np.nan, 1.0, 1.0, 2.0], [np.nan, 5.0, np.nan, np.nan, np.nan], [np.nan] * 5])
    used = ~np.isnan(lod)
    count, mean, sd, index, best = cases.select(lod, used, 3)
    assert count.tolist() == [4, 1, 0]
    assert mean[0] == 1.75 and sd[0] == np.sqrt((1.25 ** 2 + 2 * 0.75 ** 2 + 0.25 ** 2) / 3) and np.isnan(mean[1:]).all() and np.isnan(sd[1:]).all()
    assert index.tolist() == [[2, 3, 4], [1, -1, -1], [-1, -1, -1]]
    assert best[0].tolist() == [1.0, 1.0, 2.0] and best[1, 0] == 5.0 and np.isnan(best[1, 1:]).all() and np.isnan(best[2]).all()
