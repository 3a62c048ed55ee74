"""The outputs built on top of an HMM run at the launch sizes of a cohort (tests/cohort_cases.py; needs an
MI355X): grid dosages, path draws, diagnostics, log-likelihoods, panel matching, SNP dosages and the scan's hand-over at 5,
64 and 65 samples per launch, with the library's defaults - no tuning variable is set anywhere in this file.
tests/test_cohort_sizes_cpu.py holds the rows to their routes and 65 to "one past every partition".

Nothing here is a new comparison or a new number: the restatements, the `assert_*` helpers and the tolerances are those of
the suites of the outputs (tests/test_grid_gpu.py, test_sim_geno_gpu.py, test_diagnostics_gpu.py, test_loglik_gpu.py,
test_match_gpu.py, test_impute_gpu.py, test_scan_gpu.py), imported and named where they are used.  Three kinds of assertion
per output:
  (a) against the restatement on the device's own intermediates, for cohort_cases.EDGE_SAMPLES cut to the launch - the
      first and the last member of every partition of 8, 16 and 64 samples a kernel makes.  This restriction is the only
      one, and every test that makes it says so;
  (b) over the whole launch: the row of EVERY sample equals, bit for bit, the result of the same call with sample=s; no two
      samples' rows are equal; two identical launch-wide calls give the same bytes;
  (c) against the composed CPU oracle end to end where the output's suite has such a test, for the EDGE_SAMPLES.
The sample index of a first wrong row names the partition, by the table in tests/cohort_cases.py."""
import os

import numpy as np
import pytest

import cohort_cases as cases
import grid_cases
import impute_cases
import loglik_cases
import loglik_restate
import match_cases
import small_ops_cases
import test_diagnostics_gpu as diag_suite
import test_impute_gpu as impute_suite
import test_loglik_gpu as loglik_suite
import test_match_gpu as match_suite
import test_sim_geno_gpu as paths_suite
from test_diagnostics_gpu import tables  # noqa: F401  (a fixture)
from test_grid_gpu import dosage_rows, run_samples

pytestmark = pytest.mark.gpu

SMALL_AND_ONE_PAST = [(8, 5), (8, 65)]
FULL_TOO = [(8, 5), (8, 64), (8, 65)]
MATCH_ROWS = [(8, 64), (8, 65), (3, 65)]
M_PANEL = 65                                    # one entry into a second block of 64 panel entries


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_", "GBRS_DIAG_")):
            monkeypatch.delenv(k, raising=False)


def launch(H, n, style):
    """A handle with the first n samples of the family run in one launch; the row must be one of the table's."""
    cases.case(H, n)
    hmm, p0 = run_samples(H, style, range(n))
    assert hmm.n_samples == n
    return hmm, p0


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_all_different(rows, what):
    """rows: [n, ...], one row per sample of the launch."""
    flat = np.ascontiguousarray(rows).reshape(len(rows), -1)
    seen = {}
    for s, r in enumerate(flat):
        assert seen.setdefault(r.tobytes(), s) == s, f"{what}: samples {seen[r.tobytes()]} and {s} have the same row"


def gamma_flat(per_chrom):
    return np.concatenate([a.ravel() for a in per_chrom if a is not None])


# ---- grid ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", SMALL_AND_ONE_PAST)
def test_grid_on_the_devices_own_posteriors_and_over_the_whole_launch(H, n, style):
    """(a) as test_grid_gpu.test_grid_pass_on_the_devices_own_posteriors, for the EDGE_SAMPLES only: gamma_grid equals
    postproc_oracle.interpolate of hmm.get's gamma bit for bit, the dosage is within small_ops_cases.dosage_rtol(H) of the
    oracle's product.  (b) for every sample, dosage and gamma_grid."""
    from oracle import postproc_oracle
    hmm, p0 = launch(H, n, style)
    S = hmm.S
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        hmm.set_grid(grid.positions, grid.points)
        both = hmm.grid(want=("dosage", "gamma_grid"))
        M = sum(len(x) for x in grid.points.values())
        assert hmm.grid_info()[0] == M and both["dosage"].shape == (n, M, H)
        flat = np.stack([gamma_flat(both["gamma_grid"][s]) for s in range(n)])
        # (b)
        again = hmm.grid(want=("dosage", "gamma_grid"))
        assert same_bytes(again["dosage"], both["dosage"]), f"grid {name}: two calls"
        assert same_bytes(np.stack([gamma_flat(again["gamma_grid"][s]) for s in range(n)]), flat), f"grid {name}: two calls"
        assert_all_different(both["dosage"], f"dosage, grid {name}")
        assert_all_different(flat, f"gamma_grid, grid {name}")
        for s in range(n):
            one = hmm.grid(sample=s, want=("dosage", "gamma_grid"))
            assert same_bytes(one["dosage"], both["dosage"][s]), f"dosage, grid {name}: sample {s} alone"
            assert same_bytes(gamma_flat(one["gamma_grid"]), flat[s]), f"gamma_grid, grid {name}: sample {s} alone"
        # (a)
        worst = 0.0
        for s in cases.edge_samples(n):
            for ci, c in enumerate(p0.chroms):
                got = both["gamma_grid"][s][ci]
                if c not in grid.points:
                    assert got is None
                    continue
                gamma = hmm.get(ci, sample=s, want=("gamma",))["gamma"]
                want = postproc_oracle.interpolate(grid.positions[c], gamma, grid.points[c])
                assert got.shape == (S, len(grid.points[c]))
                np.testing.assert_array_equal(got, want, err_msg=f"grid {name} sample {s} chromosome {c}")
                d, dw = dosage_rows(hmm, p0, both["dosage"][s], c), postproc_oracle.dosage(want.T, H)
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(dw != 0, np.abs(d - dw) / np.abs(dw), 0.0))))
                np.testing.assert_allclose(d, dw, rtol=small_ops_cases.dosage_rtol(H), atol=0,
                                           err_msg=f"dosage, grid {name} sample {s} chromosome {c}")
        print(f"DEVIATION dosage against the oracle's product, H={H} n={n} {style} grid {name}: {worst:.3g} "
              f"(bound {small_ops_cases.dosage_rtol(H):.3g})")
    hmm.close()


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", SMALL_AND_ONE_PAST)
def test_grid_against_the_oracle_end_to_end(H, n, style):
    """(c) as test_grid_gpu.test_grid_pass_against_the_oracle_end_to_end, for the EDGE_SAMPLES only: grid_cases.expected_for
    at that test's rtol 1e-8, atol 4 x 2^-53 for an interpolated value and 2 S 2^-53 for a dosage."""
    hmm, p0 = launch(H, n, style)
    S = hmm.S
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        hmm.set_grid(grid.positions, grid.points)
        got = hmm.grid(want=("dosage", "gamma_grid"))
        worst = 0.0
        for s in cases.edge_samples(n):
            on_grid, dosage = grid_cases.expected_for(H, style, s, name)
            row = 0
            for c in grid.points:                                   # the oracle's dosage rows are in grid order
                ci = p0.chroms.index(c)
                at = f"grid {name} sample {s} chromosome {c}"
                np.testing.assert_allclose(got["gamma_grid"][s][ci], on_grid[c], rtol=1e-8, atol=4 * 2.0 ** -53, err_msg=at)
                m = len(grid.points[c])
                d = dosage_rows(hmm, p0, got["dosage"][s], c)
                worst = max(worst, float(np.abs(d - dosage[row:row + m]).max()))
                np.testing.assert_allclose(d, dosage[row:row + m], rtol=1e-8, atol=2 * S * 2.0 ** -53, err_msg=at)
                row += m
        print(f"DEVIATION dosage against the composed oracle, H={H} n={n} {style} grid {name}: worst absolute difference "
              f"{worst:.3g} (rtol 1e-8, atol {2 * S * 2.0 ** -53:.3g})")
    hmm.close()


# ---- path draws ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", cases.PATH_ROWS)
def test_path_draws(H, n, style):
    """(a) test_sim_geno_gpu.assert_equals_the_restatement for the EDGE_SAMPLES only, 1 and 65 draws, with streams that are
    not the slot numbers (cohort_cases.streams: 2 n - slot).  That suite's rule holds: a draw that restate.comparable
    leaves out (a margin below its FLOOR) fails the test, and another seed is chosen on the CPU.  The seed is
    cohort_cases.PATH_SEED - test_sim_geno_gpu's own - because the restatement alone, on the oracle's alpha, decides
    nothing of these samples by less than 1.6e-7 with it (tests/test_cohort_sizes_cpu.py asserts 1e-7).
    (b) for every sample, 65 draws: paths and change counts."""
    hmm, p0 = launch(H, n, style)
    ids, seed, K = cases.streams(n), cases.PATH_SEED, max(cases.PATH_DRAWS)
    smallest = paths_suite.assert_equals_the_restatement(hmm, p0, n, seed, streams=ids, samples=cases.edge_samples(n),
                                                         draws=cases.PATH_DRAWS)
    print(f"DEVIATION smallest decision margin H={H} n={n} {style}: {smallest:.3g} (floor {paths_suite.FLOOR:g})")
    assert smallest >= paths_suite.FLOOR, "a draw was left out of the comparison: pick another seed on the CPU"
    whole = hmm.sample_paths(K, seed=seed, streams=ids)
    again = hmm.sample_paths(K, seed=seed, streams=ids)
    assert whole["degenerate"] == 0 and again["degenerate"] == 0
    flat = paths_suite.flat(whole)
    assert flat.shape == (n, K, sum(grid_cases.LENS))
    assert same_bytes(paths_suite.flat(again), flat) and same_bytes(again["changes"], whole["changes"])
    assert_all_different(flat, "paths")
    for s in range(n):
        one = hmm.sample_paths(K, seed=seed, sample=s, streams=[ids[s]])
        assert one["degenerate"] == 0
        assert same_bytes(paths_suite.flat(one), flat[s]), f"paths: sample {s} alone"
        assert same_bytes(one["changes"], whole["changes"][s]), f"changes: sample {s} alone"
    hmm.close()


# ---- diagnostics -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", FULL_TOO)
def test_diagnostics(H, n, style):
    """(a) test_diagnostics_gpu.assert_equals_the_restatement for the EDGE_SAMPLES only (its tolerances: xo, pswitch and xi
    rtol 1e-9 and atol 1e-15, errlod rtol 1e-9 and atol 1e-9, maxprob and maxmarg equal); xi for the samples 0, 63 and 64
    only - the first sample, the last of the last full slab and the lone sample of the fifth.  (b) for every sample and all
    five arrays."""
    hmm, p0 = launch(H, n, style)
    worst = diag_suite.assert_equals_the_restatement(hmm, p0, n, samples=cases.edge_samples(n),
                                                     with_xi=[s for s in (0, 63, 64) if s < n])
    assert hmm.diagnostics_info() > 0
    print(f"DEVIATION diagnostics against the restatement H={H} n={n} {style}: worst absolute differences "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    whole = hmm.diagnostics()
    assert sorted(whole) == sorted(diag_suite.NAMES)
    diag_suite.assert_same_bits(hmm.diagnostics(), whole)
    for k, rows in diag_suite.flat(whole).items():
        assert_all_different(rows, k)
    for s in range(n):
        diag_suite.assert_same_bits(hmm.diagnostics(sample=s), {k: [a[s] for a in v] for k, v in whole.items()})
    hmm.close()


# ---- log-likelihoods -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", SMALL_AND_ONE_PAST)
def test_loglik(H, n, style):
    """hmm.loglik and hmm.loglik_tables with the five candidates of loglik_cases.  (a) / (c) against
    loglik_restate.per_chromosome - the oracle's forward pass - for the EDGE_SAMPLES only, at test_loglik_gpu.RTOL; for
    EVERY sample test_base_reduction's bound against the device's own scaler row, n_c 2^-53 sum |scaler_i|.  (b) for every
    sample, both calls."""
    names = ("base",) + loglik_cases.CANDIDATES
    hmm, p0 = launch(H, n, style)
    nc = len(p0.chroms)
    got = hmm.loglik()
    assert got.shape == (n, nc) and got.dtype == np.float64 and hmm.loglik_info()[0] > 0
    tabs = [[loglik_cases.candidate(H, style, name)[ci] for name in names] for ci in range(nc)]
    under = np.stack([hmm.loglik_tables(ci, tabs[ci]) for ci in range(nc)], axis=-1)           # [candidate, sample, chromosome]
    assert under.shape == (len(names), n, nc) and not np.isnan(under).any()
    np.testing.assert_allclose(under[0], got, rtol=loglik_suite.RTOL, atol=0)                    # the base as a candidate
    worst = 0.0
    for s in cases.edge_samples(n):
        for k, name in enumerate(names):
            want = loglik_restate.per_chromosome(H, style, s, name)
            np.testing.assert_allclose(under[k, s], want, rtol=loglik_suite.RTOL, atol=0, err_msg=f"{name} sample {s}")
            worst = max(worst, loglik_suite.relative(under[k, s], want))
        want = loglik_restate.per_chromosome(H, style, s)
        np.testing.assert_allclose(got[s], want, rtol=loglik_suite.RTOL, atol=0, err_msg=f"sample {s}")
        worst = max(worst, loglik_suite.relative(got[s], want))
    print(f"DEVIATION loglik and loglik_tables against the restatement H={H} n={n} {style}: worst relative difference "
          f"{worst:.2e} (rtol {loglik_suite.RTOL:g})")
    for s in range(n):
        for ci, c in enumerate(p0.chroms):
            scaler = hmm.get(ci, sample=s, want=("scaler",))["scaler"]
            bound = len(scaler) * 2.0 ** -53 * np.abs(scaler).sum()
            assert abs(got[s, ci] - -scaler.sum()) <= bound, (s, c, got[s, ci], -scaler.sum(), bound)
    # (b)
    assert same_bytes(hmm.loglik(), got)
    assert_all_different(got, "loglik")
    assert_all_different(under.transpose(1, 0, 2), "loglik_tables")
    for ci in range(nc):
        assert same_bytes(hmm.loglik_tables(ci, tabs[ci]), under[:, :, ci]), f"loglik_tables, chromosome {ci}: two calls"
    for s in range(n):
        one = hmm.loglik(sample=s)
        assert one.shape == (1, nc) and same_bytes(one[0], got[s]), f"loglik: sample {s} alone"
        for ci in range(nc):
            one = hmm.loglik_tables(ci, tabs[ci], sample=s)
            assert one.shape == (len(names), 1) and same_bytes(one[:, 0], under[:, s, ci]), \
                f"loglik_tables: sample {s} alone, chromosome {ci}"
    assert same_bytes(hmm.loglik(), got)
    hmm.close()


# ---- match -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,n", MATCH_ROWS)
def test_match_sums(H, n):
    """(a) match_cases.restate - one numpy product on hmm.grid()'s dosages - for EVERY sample through
    test_match_gpu.assert_sums (rtol match_cases.rtol(points, H) = 4 K 2^-53, atol 0), 65 random panel entries, both
    grids.  (b) for every sample.  No sample is left out of either."""
    hmm, p0 = launch(H, n, "do")
    rng = np.random.default_rng(100 * H + n)
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        points, offsets = match_cases.handle_points(p0.chroms, grid)
        hmm.set_grid(grid.positions, grid.points)
        panel = match_cases.random_panel(rng, M_PANEL, sum(points), H)
        hmm.set_panel(panel)
        first, info = hmm.match(), hmm.match_info()
        assert info["n_panel"] == M_PANEL and first["cross"].shape == (n, len(p0.chroms), M_PANEL)
        assert first["sample_norm"].shape == (n, len(p0.chroms))
        want = match_cases.restate(hmm.grid()["dosage"], panel, points, offsets)
        match_suite.assert_sums(first, info, want, points, H, f"grid {name}")
        worst, bound = max((float(np.max(np.abs(first["cross"][:, c] - want[0][:, c]) / np.maximum(want[0][:, c], 1e-300))),
                            match_cases.rtol(m, H)) for c, m in enumerate(points) if m)
        print(f"DEVIATION cross against numpy, H={H} n={n} M={M_PANEL} grid {name}: {worst:.3g} (bound {bound:.3g} on "
              f"that chromosome)")
        again = hmm.match()
        assert same_bytes(again["cross"], first["cross"]) and same_bytes(again["sample_norm"], first["sample_norm"])
        assert_all_different(first["cross"], f"cross, grid {name}")
        assert_all_different(first["sample_norm"], f"sample_norm, grid {name}")
        for s in range(n):
            one = hmm.match(sample=s)
            assert same_bytes(one["cross"], first["cross"][s]), f"cross, grid {name}: sample {s} alone"
            assert same_bytes(one["sample_norm"], first["sample_norm"][s]), f"sample_norm, grid {name}: sample {s} alone"
        whole = hmm.match()                                              # grid_dosage holds one sample now: made again
        assert same_bytes(whole["cross"], first["cross"])
    hmm.close()


@pytest.mark.parametrize("H,n", MATCH_ROWS)
def test_match_exact_values_are_exact(H, n):
    """As test_match_gpu.test_exact_values_are_exact: one-hot posteriors give dosages in {0, 1/2, 1}, and against a panel of
    such values the three sums of every sample equal the restatement with ==; the last entry is disjoint from sample 0."""
    cases.case(H, n)
    hmm, p0, state = match_suite.run_one_hot(H, n)
    pairs = match_cases.states(H)
    rng = np.random.default_rng(7 * H + n)
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        points, offsets = match_cases.handle_points(p0.chroms, grid)
        hmm.set_grid(grid.positions, grid.points)
        panel = match_cases.one_hot_panel(rng, M_PANEL, sum(points), H)
        d = np.zeros((sum(points), H))
        for ci, (m, o) in enumerate(zip(points, offsets)):
            free = [f for f in range(H) if f not in pairs[state(0, ci)]]
            d[o:o + m, free[0]] = 1.0
        panel[-1] = d
        hmm.set_panel(panel)
        got, info = hmm.match(), hmm.match_info()
        dosage = hmm.grid()["dosage"]
        assert np.isin(dosage, (0.0, 0.5, 1.0)).all(), "the dosages of this case are not exact"
        cross, snorm, pnorm = match_cases.restate(dosage, panel, points, offsets)
        np.testing.assert_array_equal(got["cross"], cross)
        np.testing.assert_array_equal(got["sample_norm"], snorm)
        np.testing.assert_array_equal(info["panel_norm"], pnorm)
        assert (snorm[:, [c for c, m in enumerate(points) if m]] > 0).all()
        assert (got["cross"][0, :, -1] == 0.0).all() and (pnorm[-1] == np.asarray(points, dtype=float)).all()
    hmm.close()


@pytest.mark.parametrize("H", (8, 3))
def test_match_rows_do_not_depend_on_the_launch(H):
    """As test_match_gpu.test_a_samples_numbers_do_not_depend_on_its_launch_or_on_the_panels_size: one-hot posteriors - the
    same dosages in every run - against a panel of random doubles whose sums depend on the order (asserted, as there).
    The samples 58 .. 64 at positions 0 .. 6 of a run of 7 and the samples 32 .. 47 in a run of 16 have, bit for bit, the
    rows they had in the run of 65: the block, the wavefront and the row within it play no part."""
    n = 65
    cases.case(H, n)
    grid = grid_cases.grids()["b"]
    big, p0, _ = match_suite.run_one_hot(H, n)
    points, offsets = match_cases.handle_points(p0.chroms, grid)
    panel = match_cases.random_panel(np.random.default_rng(11), M_PANEL, sum(points), H)
    big.set_grid(grid.positions, grid.points)
    big.set_panel(panel)
    want = big.match()
    big.close()
    on_x = np.stack(panel)[:, offsets[4]:offsets[4] + points[4]].reshape(M_PANEL, -1)
    assert any(np.cumsum(x)[-1] != np.cumsum(x[::-1])[-1] for x in on_x), "the sums of this case do not depend on the order"
    assert len(np.unique(want["cross"][58:, 4, :])) > 7 * M_PANEL // 2
    for first, count in ((58, 7), (32, 16)):
        small, _, _ = match_suite.run_one_hot(H, count, first=first)
        small.set_grid(grid.positions, grid.points)
        small.set_panel(panel)
        got = small.match()
        small.close()
        np.testing.assert_array_equal(got["cross"], want["cross"][first:first + count], err_msg=f"samples {first} ..")
        np.testing.assert_array_equal(got["sample_norm"], want["sample_norm"][first:first + count], err_msg=f"samples {first} ..")


# ---- SNP dosages -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", SMALL_AND_ONE_PAST)
def test_snp_dosages(H, n, style):
    """Every SNP set of impute_cases.  (a) test_impute_gpu.restated - the rule on hmm.get's gamma - for the EDGE_SAMPLES
    only, within test_impute_gpu.reassociation_atol(H).  (c) impute_cases.composed for the EDGE_SAMPLES only, at
    test_impute_against_the_composed_oracle's rtol 1e-8 and atol 4 S 2^-53.  (b) for every sample."""
    hmm, p0 = launch(H, n, style)
    S = hmm.S
    edges = cases.edge_samples(n)
    worst = worst_oracle = 0.0
    for name, snps in impute_cases.snp_sets().items():
        masks = impute_cases.masks_for(name, H)
        hmm.set_snps(snps.positions, snps.points, masks)
        M = sum(len(x) for x in snps.points.values())
        whole = hmm.impute()
        assert whole.shape == (n, M) and hmm.impute_info()["n_snps"] == M
        assert same_bytes(hmm.impute(), whole), f"set {name}: two calls"
        assert_all_different(whole, f"set {name}")
        for s in range(n):
            assert same_bytes(hmm.impute(sample=s), whole[s]), f"set {name}: sample {s} alone"
        assert same_bytes(hmm.impute(), whole), f"set {name}: after single samples the launch is made again"
        for s in edges:
            want = impute_suite.restated(hmm, p0, snps, masks, s)
            worst = max(worst, float(np.abs(whole[s] - want).max()))
            np.testing.assert_allclose(whole[s], want, rtol=0, atol=impute_suite.reassociation_atol(H),
                                       err_msg=f"set {name} sample {s}")
            composed = impute_cases.handle_order(p0.chroms, snps, impute_cases.composed(
                grid_cases.sample_problem(H, style, s), snps, masks, grid_cases.oracle_arrays(H, style, s)[0],
                sorted_knots=name in impute_cases.NEEDS_SORTED_KNOTS))
            worst_oracle = max(worst_oracle, float(np.abs(whole[s] - composed).max()))
            np.testing.assert_allclose(whole[s], composed, rtol=1e-8, atol=2 * 2 * S * 2.0 ** -53,
                                       err_msg=f"set {name} sample {s} against the composed oracle")
    print(f"DEVIATION SNP dosages H={H} n={n} {style}: against the restatement {worst:.3g} (bound "
          f"{impute_suite.reassociation_atol(H):.3g}), against the composed oracle {worst_oracle:.3g} (rtol 1e-8, atol "
          f"{4 * S * 2.0 ** -53:.3g})")
    hmm.close()


@pytest.mark.parametrize("H,n", SMALL_AND_ONE_PAST)
def test_a_samples_snp_row_does_not_depend_on_the_chunk(H, n):
    """The chunk rule of test_impute_gpu.test_a_samples_row_does_not_depend_on_the_batch_or_the_chunk for chunks of 7 and of
    all 260 SNPs: every sample's row in the launch, and the EDGE_SAMPLES asked for alone in chunks of 7."""
    hmm, p0 = launch(H, n, "do")
    snps, masks = impute_cases.snp_sets()["n257"], impute_cases.masks_for("n257", H)
    hmm.set_snps(snps.positions, snps.points, masks)
    M = hmm.impute_info()["n_snps"]
    assert M == 260
    whole = hmm.impute(chunk=M)
    np.testing.assert_array_equal(hmm.impute(chunk=7), whole, err_msg="chunk 7")
    for s in cases.edge_samples(n):
        np.testing.assert_array_equal(hmm.impute(sample=s, chunk=7), whole[s], err_msg=f"sample {s} alone, chunk 7")
    np.testing.assert_array_equal(hmm.impute(), whole)
    hmm.close()


# ---- the scan's hand-over --------------------------------------------------------------------------------------------------

def test_scan_append_from_a_launch_of_65():
    """GenomeScan.append_from of the 65-sample handle leaves what append of hmm.grid()['dosage'] copied to the host leaves:
    the same LODs, bit for bit.  One phenotype, grid "a"."""
    from gbrs_amd.scan import GenomeScan
    H, n = 8, 65
    hmm, p0 = launch(H, n, "do")
    grid = grid_cases.grids()["a"]
    hmm.set_grid(grid.positions, grid.points)
    y = np.random.default_rng(65).normal(size=n)
    by_device = GenomeScan(H, hmm.grid_points)
    by_device.append_from(hmm)
    dosage = hmm.grid()["dosage"]
    by_host = GenomeScan(H, hmm.grid_points)
    by_host.append(dosage)
    assert by_device.n == by_host.n == n
    results = []
    for scan in (by_device, by_host):
        scan.prepare()
        results.append(scan.run(y))
        scan.close()
    assert np.isfinite(results[0]["lod"]).all() and (results[0]["lod"] > 0).any()
    for key in results[0]:
        assert same_bytes(results[0][key], results[1][key]), key
    hmm.close()


# ---- the raw calls write no row too many -----------------------------------------------------------------------------------

def test_raw_calls_stay_inside_the_rows_of_the_launch():
    """gbrs_hmm_match, gbrs_hmm_diagnostics and gbrs_hmm_loglik of the 65-sample launch into host buffers one sample's rows
    longer than needed, filled with -7 beforehand: the extra row is intact and the first 65 equal the wrapper's result."""
    from gbrs_amd import _lib
    lib = _lib.load()
    H, n, fill = 8, 65, -7
    hmm, p0 = launch(H, n, "do")
    nc, G = len(p0.chroms), sum(grid_cases.LENS)
    grid = grid_cases.grids()["a"]
    points, _ = match_cases.handle_points(p0.chroms, grid)
    hmm.set_grid(grid.positions, grid.points)
    hmm.set_panel(match_cases.random_panel(np.random.default_rng(3), M_PANEL, sum(points), H))

    cross, norm = np.full((n + 1, nc, M_PANEL), float(fill)), np.full((n + 1, nc), float(fill))
    assert lib.gbrs_hmm_match(hmm._h, -1, _lib.ptr(cross), _lib.ptr(norm)) == _lib.GBRS_OK
    want = hmm.match()
    assert (cross[n] == fill).all() and (norm[n] == fill).all()
    assert same_bytes(cross[:n], want["cross"]) and same_bytes(norm[:n], want["sample_norm"])

    out = {k: np.full((n + 1, G), fill, dtype=np.int32 if k == "maxmarg" else np.float64) for k in diag_suite.NAMES}
    assert lib.gbrs_hmm_diagnostics(hmm._h, -1, *[_lib.ptr(out[k]) for k in diag_suite.NAMES]) == _lib.GBRS_OK
    want = hmm.diagnostics()
    first = np.concatenate(([0], np.cumsum(grid_cases.LENS)))
    for k in diag_suite.NAMES:
        assert (out[k][n] == fill).all(), k
        assert (out[k][:n] != fill).all(), k
        for ci in range(nc):
            cut = 1 if k in ("xo", "pswitch") else 0
            assert same_bytes(out[k][:n, first[ci]:first[ci + 1] - cut], want[k][ci]), (k, ci)
            if cut:
                assert (out[k][:n, first[ci + 1] - 1] == 0.0).all(), (k, ci)        # the slot of the chromosome's last gene

    loglik = np.full((n + 1, nc), float(fill))
    assert lib.gbrs_hmm_loglik(hmm._h, -1, _lib.ptr(loglik)) == _lib.GBRS_OK
    assert (loglik[n] == fill).all() and same_bytes(loglik[:n], hmm.loglik())
    hmm.close()


# ---- the command -----------------------------------------------------------------------------------------------------------

def test_sample_file_with_the_default_batch_size(tmp_path, tables):  # noqa: F811
    """`reconstruct --sample-file` with two samples more than the default batch size and NO --batch-size, with --grid-file,
    --diagnostics and --sim-geno 2: the command must have made one full launch and one of two samples.  Both are rebuilt
    here with run_samples, and the files of the first, the two middle and the last sample of the full launch and of the
    two behind it are checked with test_diagnostics_gpu.assert_diagnostics_files and
    test_sim_geno_gpu.assert_sim_geno_files, the dosage table against hmm.grid (the `%.6f` text: half a unit of the sixth
    decimal, the 0.5e-6 + 1e-8 of test_grid_gpu.test_reconstruct_many_in_partial_batches).  The default is read from the
    parser; it must be the sample count of a row of cohort_cases whose route is the one the other tests here cover."""
    from gbrs_amd import cli
    H, style = diag_suite.H_FILES, diag_suite.STYLE_FILES
    assert (H, style) == (paths_suite.H_FILES, paths_suite.STYLE_FILES)
    (tmp_path / "samples.txt").write_text("# cohort\n")
    args = ["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "-t", tables["tprob"], "-x", tables["avecs"], "-g",
            tables["gpos"], "--grid-file", tables["grid"], "--diagnostics", "--sim-geno", "2"]
    batch = cli.build_parser().parse_args(args).batch_size
    full = cases.case(H, batch)
    assert (full.sweep, full.delta, full.bp) == ("mfma", "lanes", "lanes") and cases.case(H, batch + 1)[2:] == full[2:]
    n = batch + 2
    checked = (0, batch // 2 - 1, batch // 2, batch - 1, batch, batch + 1)
    with open(tmp_path / "samples.txt", "a") as fh:
        for s in range(n):
            fh.write(f"{diag_suite.sample_tpm(tmp_path, s)}\t{tmp_path / f'many{s}'}\n")
    assert cli.main(args) == 0
    grid = grid_cases.grids()["b"]
    for lo in range(0, n, batch):                    # the launches the command must have made
        members = list(range(lo, min(lo + batch, n)))
        hmm, p0 = run_samples(H, style, members)
        hmm.set_grid(grid.positions, grid.points)
        for slot, s in enumerate(members):
            if s not in checked:
                continue
            stem = str(tmp_path / f"many{s}")
            diag_suite.assert_diagnostics_files(stem, hmm, slot, s, 2.0)
            paths_suite.assert_sim_geno_files(stem, hmm, slot, s, 0, 2)
            header, numbers = grid_cases.read_tsv(f"{stem}.interpolated.genoprobs.tsv")
            assert header == "# " + "\t".join(p0.hap_names) + "\n"
            want = match_cases.to_grid_order(hmm.grid(sample=slot)["dosage"], p0.chroms, grid)
            np.testing.assert_allclose(numbers, want, rtol=0, atol=0.5e-6 + 1e-8, err_msg=f"sample {s}")
        hmm.close()
    assert all(os.path.exists(tmp_path / f"many{s}.diagnostics.npz") for s in range(n))
