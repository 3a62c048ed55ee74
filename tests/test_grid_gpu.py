"""The grid pass of the HIP HMM (gbrs_hmm_set_grid / gbrs_hmm_grid) and the commands over it: `gbrs reconstruct
--grid-file`, `--sample-file`, the worker's `grid_file` (needs an MI355X).  Shapes, grids and the composed oracle:
tests/grid_cases.py.

Two kinds of comparison.  Against the device's own posteriors the grid probabilities are bit-equal to
oracle.postproc_oracle.interpolate of them: the kernel takes scipy's operations in scipy's order and the library is built
without FMA contraction (the claim tests/test_postproc_edges_gpu.py makes for gbrs_interpolate).  The dosages are length-S
sums of non-negative products: within 2 S 2^-53 of any other order.  Against the oracle end to end the posteriors carry
their own 1e-8 (tests/test_hmm_gpu.py); an interpolated value is a convex combination of two of them, which keeps that
relative error, plus four roundings of values in [0, 1]."""
import os
import sys

import numpy as np
import pytest

import grid_cases
import small_ops_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

# founders x samples: 1, 3 and 25 samples at 8 founders take the blocked scan, the small batch and the two-samples-per-wave
# chains of the HMM
TABLE = [(H, n) for H in (1, 3, 8, 16) for n in (1, 3)] + [(8, 25)]
STYLES = ("benign", "do")


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_")):
            monkeypatch.delenv(k, raising=False)


def run_samples(H, style, samples):
    """A handle on the table's problem with the given samples run."""
    from gbrs_amd.hmm import DiplotypeHMM
    p0 = grid_cases.problem(H, style)
    hmm = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    av, ha = grid_cases.specificity(p0)
    rows = [grid_cases.expression_rows(grid_cases.sample_problem(H, style, s)) for s in samples]
    hmm.set_expression([np.stack([r[ci] for r in rows]) for ci in range(len(p0.chroms))], av, ha, 1.5, 0.12)
    hmm.run()
    return hmm, p0


def dosage_rows(hmm, p0, dosage, chrom):
    ci = p0.chroms.index(chrom)
    return dosage[..., hmm.grid_offsets[ci]:hmm.grid_offsets[ci] + hmm.grid_points[ci], :]


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_grid_pass_on_the_devices_own_posteriors(H, n, style):
    """Every (sample, chromosome): gamma_grid equals the oracle's interpolation of hmm.get's gamma bit for bit (a wrong
    sample stride, gene offset or knot shows as another sample's or another gene's numbers), the dosage is within
    2 S 2^-53 of the oracle's product, the dosage asked for alone is the dosage asked for with gamma_grid, and one sample
    asked for alone is that sample of the whole run."""
    from oracle import postproc_oracle
    hmm, p0 = run_samples(H, style, range(n))
    S = hmm.S
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        hmm.set_grid(grid.positions, grid.points)
        both = hmm.grid(want=("dosage", "gamma_grid"))
        alone = hmm.grid(want=("dosage",))
        M = sum(len(x) for x in grid.points.values())
        assert hmm.grid_info()[0] == M and both["dosage"].shape == (n, M, H) and set(alone) == {"dosage"}
        np.testing.assert_array_equal(alone["dosage"], both["dosage"])
        worst = 0.0
        for s in range(n):
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
        print(f"DEVIATION dosage against the oracle's product, H={H} n={n} {style} grid {name}: {worst:.3g} "
              f"(bound {cases.dosage_rtol(H):.3g})")
        for s in range(n):
            for c in grid.points:
                ci = p0.chroms.index(c)
                dw = postproc_oracle.dosage(both["gamma_grid"][s][ci].T, H)
                np.testing.assert_allclose(dosage_rows(hmm, p0, both["dosage"][s], c), dw, rtol=cases.dosage_rtol(H), atol=0,
                                           err_msg=f"dosage, grid {name} sample {s} chromosome {c}")
        s = n - 1
        one = hmm.grid(sample=s, want=("dosage", "gamma_grid"))
        np.testing.assert_array_equal(one["dosage"], both["dosage"][s])
        for a, b in zip(one["gamma_grid"], both["gamma_grid"][s]):
            assert (a is None and b is None) or np.array_equal(a, b)
    hmm.close()


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_grid_pass_against_the_oracle_end_to_end(H, n, style):
    """grid_cases.expected (reconstruct_arrays + interpolate + dosage on the CPU) for every sample: rtol 1e-8 is the
    posterior's own tolerance, atol 4 x 2^-53 the four roundings of an interpolated value, 2 S 2^-53 the dosage sum's.
    The samples of the 25-sample run are held to the same bound (the route of a 25-sample launch cannot be forced on a
    launch of one)."""
    hmm, p0 = run_samples(H, style, range(n))
    S = hmm.S
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        hmm.set_grid(grid.positions, grid.points)
        got = hmm.grid(want=("dosage", "gamma_grid"))
        for s in range(n):
            on_grid, dosage = grid_cases.expected_for(H, style, s, name)
            row = 0
            for c in grid.points:                                   # the oracle's dosage rows are in grid order
                ci = p0.chroms.index(c)
                at = f"grid {name} sample {s} chromosome {c}"
                np.testing.assert_allclose(got["gamma_grid"][s][ci], on_grid[c], rtol=1e-8, atol=4 * 2.0 ** -53, err_msg=at)
                m = len(grid.points[c])
                np.testing.assert_allclose(dosage_rows(hmm, p0, got["dosage"][s], c), dosage[row:row + m], rtol=1e-8,
                                           atol=2 * S * 2.0 ** -53, err_msg=at)
                row += m
    hmm.close()


@pytest.mark.parametrize("H,n", [(8, 1), (8, 3), (3, 3), (16, 1)])
def test_unsorted_knots_equal_interpolate_arrays(H, n):
    """Two genes out of order and a gene beyond the last grid point + 1: the grid pass sorts the knots as
    postproc.interpolate_arrays does, and equals it on the device's own posteriors bit for bit."""
    from gbrs_amd.postproc import interpolate_arrays
    hmm, p0 = run_samples(H, "benign", range(n))
    grid = grid_cases.grids()["unsorted"]
    hmm.set_grid(grid.positions, grid.points)
    got = hmm.grid(want=("gamma_grid",))["gamma_grid"]
    for s in range(n):
        for c in grid.points:
            ci = p0.chroms.index(c)
            gamma = hmm.get(ci, sample=s, want=("gamma",))["gamma"]
            np.testing.assert_array_equal(got[s][ci], interpolate_arrays(grid.positions[c], gamma, grid.points[c]),
                                          err_msg=f"sample {s} chromosome {c}")
    hmm.close()


@pytest.mark.parametrize("H,n", [(1, 1), (3, 3), (8, 1), (8, 3), (8, 25), (16, 3)])
def test_dosage_of_one_hot_posteriors_is_exact(H, n):
    """Emissions that are -inf off one state (another one per sample and chromosome): every posterior row is one-hot, so is
    every interpolated row (slope 0), and the dosage is 0.5 for each founder of that state, 1.0 for a homozygote.  Exact."""
    from gbrs_amd.hmm import DiplotypeHMM
    p0 = grid_cases.problem(H, "benign")
    S = H * (H + 1) // 2
    hmm = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    state = lambda s, ci: (5 * s + 3 * ci + 1) % S
    eprob = []
    for ci, c in enumerate(p0.chroms):
        e = np.full((n, len(p0.gene_ids[c]), S), -np.inf)
        for s in range(n):
            e[s, :, state(s, ci)] = 0.0
        eprob.append(e)
    hmm.set_eprob(eprob)
    hmm.run()
    _, one_hot_dosage = cases.dosage_one_hot(H)
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        hmm.set_grid(grid.positions, grid.points)
        got = hmm.grid(want=("dosage", "gamma_grid"))
        for s in range(n):
            for c in grid.points:
                ci = p0.chroms.index(c)
                gamma = hmm.get(ci, sample=s, want=("gamma",))["gamma"]
                assert (gamma == np.eye(S)[:, [state(s, ci)]]).all(), "the posteriors of this case are not one-hot"
                m = len(grid.points[c])
                np.testing.assert_array_equal(got["gamma_grid"][s][ci], np.repeat(np.eye(S)[:, [state(s, ci)]], m, axis=1))
                np.testing.assert_array_equal(dosage_rows(hmm, p0, got["dosage"][s], c),
                                              np.repeat(one_hot_dosage[[state(s, ci)]], m, axis=0))
    hmm.close()


def test_raw_call_errors_leave_the_outputs_untouched():
    """No run: GBRS_ERR_STATE.  No grid, a sample out of range, a grid chromosome without genes (at set time), gene
    positions that are not the handle's: GBRS_ERR_INVALID.  A grid point outside the knots: interp1d's text."""
    import ctypes as C
    from gbrs_amd import _lib
    lib = _lib.load()
    hmm, p0 = run_samples(3, "benign", range(2))
    grid = grid_cases.grids()["a"]
    M = sum(len(x) for x in grid.points.values())
    dosage, flat = np.full((2, M, 3), -1.0), np.full((2, 6 * M), -1.0)

    def call(sample):
        return lib.gbrs_hmm_grid(hmm._h, sample, _lib.ptr(dosage), _lib.ptr(flat))

    def untouched():
        return (dosage == -1.0).all() and (flat == -1.0).all()

    assert call(-1) == _lib.GBRS_ERR_INVALID and b"no grid" in lib.gbrs_last_error() and untouched()
    assert hmm.grid_info()[0] == 0
    with pytest.raises(_lib.GbrsHipError):
        hmm.grid()
    # set time
    where = [np.ascontiguousarray(grid.positions[c]) for c in p0.chroms]
    points = [np.ascontiguousarray(grid.points.get(c, np.zeros(0))) for c in p0.chroms]
    n_pos = np.array([len(x) for x in where], dtype=np.int32)
    n_grid = np.array([len(x) for x in points], dtype=np.int32)

    def set_grid(n_pos, where, n_grid, points):
        return lib.gbrs_hmm_set_grid(hmm._h, _lib.ptr(n_pos), _lib.ptr_table(where), _lib.ptr(n_grid), _lib.ptr_table(points))

    no_genes = n_pos.copy()
    no_genes[1] = 0
    assert set_grid(no_genes, where, n_grid, points) == _lib.GBRS_ERR_INVALID and b"out of bounds" in lib.gbrs_last_error()
    fewer = n_pos.copy()
    fewer[3] -= 1
    assert set_grid(fewer, where, n_grid, points) == _lib.GBRS_ERR_INVALID
    below = [x.copy() for x in points]
    below[2][0] = -0.5
    assert set_grid(n_pos, where, n_grid, below) == _lib.GBRS_ERR_INVALID and b"below the interpolation range" in lib.gbrs_last_error()
    assert call(-1) == _lib.GBRS_ERR_INVALID and untouched()               # a failed set leaves the handle without a grid
    with pytest.raises(ValueError, match="below the interpolation range"):
        hmm.set_grid(grid.positions, dict(grid.points, **{"3": below[2]}))
    with pytest.raises(IndexError):
        hmm.set_grid(dict(grid.positions, **{"2": np.zeros(0)}), grid.points)
    assert set_grid(n_pos, where, n_grid, points) == _lib.GBRS_OK
    for sample in (2, -2, 25):
        assert call(sample) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error() and untouched()
    assert call(1) == _lib.GBRS_OK and (dosage[0] != -1.0).all() and (dosage[1] == -1.0).all()
    assert lib.gbrs_hmm_grid(hmm._h, -1, None, None) == _lib.GBRS_OK
    # a failed set keeps the grid the handle had
    assert set_grid(n_pos, where, n_grid, below) == _lib.GBRS_ERR_INVALID
    again = np.full((1, M, 3), -2.0)
    assert lib.gbrs_hmm_grid(hmm._h, 1, _lib.ptr(again), None) == _lib.GBRS_OK
    np.testing.assert_array_equal(again[0], dosage[0])
    # new samples on the handle, no run yet
    rows = grid_cases.expression_rows(grid_cases.sample_problem(3, "benign", 2))
    hmm.set_expression(rows, expr_threshold=1.5, sigma=0.12)
    dosage[:] = -1.0
    flat[:] = -1.0
    assert call(-1) == _lib.GBRS_ERR_STATE and untouched()
    assert lib.gbrs_hmm_grid(None, -1, _lib.ptr(dosage), None) == _lib.GBRS_ERR_INVALID
    hmm.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES = 8, "benign"


@pytest.fixture
def tables(tmp_path, monkeypatch):
    """$GBRS_DATA with the table's 8-founder problem, a grid file of grid "b" (its chromosome order is not the genome's)."""
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    return paths


def sample_tpm(tmp_path, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, sample))


def chain(tpm, paths, stem):
    """`gbrs reconstruct` -> `gbrs interpolate` -> `gbrs export -s <the header's haplotypes>` on the same inputs."""
    from gbrs_amd import hmm as H, postproc
    H.reconstruct(tpm, paths["tprob"], paths["avecs"], paths["gpos"], 1.5, 0.12, stem)
    postproc.interpolate(f"{stem}.genoprobs.npz", paths["grid"], paths["gpos"], f"{stem}.interp.npz")
    postproc.export(f"{stem}.interp.npz", grid_cases.problem(H_FILES, STYLE_FILES).hap_names, paths["grid"], f"{stem}.export.tsv")


def assert_grid_files_equal_the_chain(stem, chain_stem, npz=True):
    header, numbers = grid_cases.read_tsv(f"{stem}.interpolated.genoprobs.tsv")
    ref_header, ref_numbers = grid_cases.read_tsv(f"{chain_stem}.export.tsv")
    assert header == ref_header
    assert numbers.shape == ref_numbers.shape
    np.testing.assert_allclose(numbers, ref_numbers, rtol=0, atol=1.01e-6)      # %.6f text: one unit of the sixth decimal
    if npz:
        got, ref = np.load(f"{stem}.interpolated.genoprobs.npz"), np.load(f"{chain_stem}.interp.npz")
        assert got.files == ref.files                                            # members and order
        for c in ref.files:
            np.testing.assert_array_equal(got[c], ref[c])     # the same posteriors through the same operations
    else:
        assert not os.path.exists(f"{stem}.interpolated.genoprobs.npz")


def test_reconstruct_with_a_grid_file_equals_the_chain(tmp_path, tables):
    from gbrs_amd import cli, hmm as H
    tpm = sample_tpm(tmp_path, 0)
    chain(tpm, tables, str(tmp_path / "chain"))
    times = {}
    H.reconstruct(tpm, tables["tprob"], tables["avecs"], tables["gpos"], 1.5, 0.12, str(tmp_path / "one"),
                  grid_file=tables["grid"], stage_times=times)
    assert "grid" in times
    assert_grid_files_equal_the_chain(str(tmp_path / "one"), str(tmp_path / "chain"), npz=False)
    assert cli.main(["reconstruct", "-e", tpm, "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"],
                     "--grid-file", tables["grid"], "--grid-genoprobs", "-o", str(tmp_path / "two")]) == 0
    assert_grid_files_equal_the_chain(str(tmp_path / "two"), str(tmp_path / "chain"))
    for suffix in ("genotypes.tsv", "genoprobs.npz", "genotypes.npz"):
        assert os.path.getsize(tmp_path / f"two.{suffix}") > 0
    assert open(tmp_path / "two.genotypes.tsv").read() == open(tmp_path / "chain.genotypes.tsv").read()


def test_grid_chromosome_missing_from_the_tables(tmp_path, tables, caplog):
    """A grid chromosome without a transition table has no posteriors: `export` ends with a KeyError in the chain, so no
    .tsv here either; the error is logged, the command returns 0, the .npz (asked for) and the three ordinary files are
    there."""
    from gbrs_amd import cli
    grid = grid_cases.grids()["b"]
    points = dict(grid.points)
    points["Z"] = np.array([1.0, 2.0])
    grid_file = grid_cases.write_grid_file(tmp_path / "grid_z.txt", points)
    tpm = sample_tpm(tmp_path, 0)
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["reconstruct", "-e", tpm, "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"],
                         "--grid-file", grid_file, "--grid-genoprobs", "-o", str(tmp_path / "out")]) == 0
    assert any("Z" in r.getMessage() for r in caplog.records if r.levelname == "ERROR")
    assert not os.path.exists(tmp_path / "out.interpolated.genoprobs.tsv")
    assert np.load(tmp_path / "out.interpolated.genoprobs.npz").files == [c for c in grid.points]
    for suffix in ("genotypes.tsv", "genoprobs.npz", "genotypes.npz"):
        assert os.path.getsize(tmp_path / f"out.{suffix}") > 0


def read_calls(path):
    with open(path) as fh:
        assert fh.readline() == "#Gene_ID\tDiplotype\n"
        return dict(line.rstrip("\n").split("\t") for line in fh)


def test_reconstruct_many_in_partial_batches(tmp_path, tables, caplog):
    """25 samples in launches of 7 (the last one of 4) through `--sample-file`, one entry of which cannot be read: the
    other 25 get their files, the calls equal the oracle's, the posteriors are within 1e-8 of it, the dosage text is the
    oracle's dosage to one unit of the sixth decimal, and the samples at the batch boundaries equal the chain's files."""
    from gbrs_amd import cli
    from gbrs_amd.synth import diplotype_names
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    names = diplotype_names(p0.hap_names)
    cohort = grid_cases.cohort(H_FILES, STYLE_FILES, 25)
    lines = ["# genes.tpm\toutbase", ""]
    for k, sample in enumerate(cohort):
        lines.append(f"{sample_tpm(tmp_path, sample)}\t{tmp_path / f'many{k}'}")
        if k == 9:
            lines.append(f"{tmp_path / 'missing.genes.tpm'}\t{tmp_path / 'missing'}")
    (tmp_path / "samples.txt").write_text("\n".join(lines) + "\n")
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "--batch-size", "7", "-t", tables["tprob"],
                         "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--grid-genoprobs"]) == 0
    errors = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(errors) == 1 and "missing.genes.tpm" in errors[0]
    assert not any(f.startswith("missing.") for f in os.listdir(tmp_path) if f != "missing.genes.tpm")
    grid = grid_cases.grids()["b"]
    for k, sample in enumerate(cohort):
        stem = str(tmp_path / f"many{k}")
        res, _ = grid_cases.oracle_arrays(H_FILES, STYLE_FILES, sample)
        want = {g: names[s] for c in p0.chroms for g, s in zip(p0.gene_ids[c], res[c]["calls"]) if s >= 0}
        assert read_calls(f"{stem}.genotypes.tsv") == want, f"sample {k}"
        gam = np.load(f"{stem}.genoprobs.npz")
        for c in p0.chroms:
            np.testing.assert_allclose(gam[c], res[c]["gamma"], rtol=1e-8, atol=1e-300, err_msg=f"sample {k} chromosome {c}")
        on_grid, dosage = grid_cases.expected_for(H_FILES, STYLE_FILES, sample, "b")
        header, numbers = grid_cases.read_tsv(f"{stem}.interpolated.genoprobs.tsv")
        assert header == "# " + "\t".join(p0.hap_names) + "\n"
        np.testing.assert_allclose(numbers, dosage, rtol=0, atol=0.5e-6 + 1e-8, err_msg=f"sample {k}")
        z = np.load(f"{stem}.interpolated.genoprobs.npz")
        assert z.files == list(grid.points)
        for c in z.files:
            np.testing.assert_allclose(z[c], on_grid[c], rtol=1e-8, atol=4 * 2.0 ** -53, err_msg=f"sample {k} chromosome {c}")
    for k in (0, 6, 7, 24):
        chain(str(tmp_path / f"s{cohort[k]}.genes.tpm"), tables, str(tmp_path / f"chain{k}"))
        np.testing.assert_allclose(grid_cases.read_tsv(str(tmp_path / f"many{k}.interpolated.genoprobs.tsv"))[1],
                                   grid_cases.read_tsv(str(tmp_path / f"chain{k}.export.tsv"))[1], rtol=0, atol=1.01e-6)
        assert read_calls(tmp_path / f"many{k}.genotypes.tsv") == read_calls(tmp_path / f"chain{k}.genotypes.tsv")


def test_the_command_and_a_cohort_write_the_same_files_with_every_option_on(tmp_path, tables):
    """`--grid-file --grid-genoprobs --sim-geno 3 --diagnostics --loglik --match-panel --snp-file` together: the
    single-sample command on sample 0 and a `--sample-file` cohort whose first line is that sample (three samples in
    launches of two) write byte-identical files for every suffix the sample gets; the cohort's first sample draws on stream
    0, so `sim_geno.npz` is among them.  `snp_dosage.npz` is compared array by array: np.savez stamps every member of the
    archive with the time of writing."""
    import impute_cases
    import match_cases
    from gbrs_amd import cli
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid = grid_cases.grids()["b"]
    rng = np.random.default_rng(grid_cases.SEED + 7)
    panel = match_cases.write_panel(tmp_path, [f"entry{k}" for k in range(5)],
                                    match_cases.random_panel(rng, 5, sum(len(x) for x in grid.points.values()), H_FILES),
                                    p0.hap_names)
    snps = impute_cases.snp_sets()["b"]                             # the positions of grid "b": the same gene positions
    snp_file = impute_cases.write_snp_file(tmp_path / "snps.tsv", H_FILES, snps.points, impute_cases.masks_for("b", H_FILES),
                                           extra=[("MT", 1.0, "10000000")])
    tpms = [sample_tpm(tmp_path, s) for s in range(3)]
    (tmp_path / "samples.txt").write_text("".join(f"{tpms[s]}\t{tmp_path / f'many{s}'}\n" for s in range(3)))
    options = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"],
               "--grid-genoprobs", "--sim-geno", "3", "--diagnostics", "--loglik", "--match-panel", panel, "--snp-file", snp_file]
    assert cli.main(["reconstruct", "-e", tpms[0], "-o", str(tmp_path / "one")] + options) == 0
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "--batch-size", "2"] + options) == 0
    suffixes = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz", "interpolated.genoprobs.tsv", "interpolated.genoprobs.npz",
                "sim_geno.npz", "sim_geno.crossovers.tsv", "diagnostics.npz", "diagnostics.tsv", "loglik.tsv", "match.tsv",
                "snp_dosage.npz")
    for stem in ("one", "many0", "many1", "many2"):
        assert sorted(f.name for f in tmp_path.glob(f"{stem}.*")) == sorted(f"{stem}.{s}" for s in suffixes)
    for suffix in suffixes:
        one, many = tmp_path / f"one.{suffix}", tmp_path / f"many0.{suffix}"
        if suffix == "snp_dosage.npz":
            a, b = np.load(one), np.load(many)
            assert a.files == b.files
            for k in a.files:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        else:
            assert one.read_bytes() == many.read_bytes(), suffix
    assert np.load(tmp_path / "one.sim_geno.npz")["stream"] == 0


def test_reconstruct_many_header_mismatch(tmp_path, tables):
    from gbrs_amd.hmm import reconstruct_many
    first = sample_tpm(tmp_path, 0)
    other = grid_cases.write_genes_tpm(tmp_path / "other.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, 1),
                                       hap_names=list("ABCDEFGZ"))
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(RuntimeError, match="haplotypes"):
        reconstruct_many([first, other], [str(tmp_path / "m0"), str(tmp_path / "m1")], tables["tprob"], tables["avecs"],
                         tables["gpos"], grid_file=tables["grid"])
    assert sorted(os.listdir(tmp_path)) == before


def test_worker_job_with_a_grid_file(tmp_path, monkeypatch):
    """A worker job with `grid_file` leaves the .tsv; a second job on the same tables and grid runs on the same context,
    and the grid goes to the device once."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_bench
    from test_worker_gpu import _write_sample
    from gbrs_amd import cli, postproc
    from gbrs_amd.worker import SampleWorker
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    samples = [_write_sample(tmp_path, seed, rows=20_000, loci=400) for seed in (7, 8)]
    aln, grp, lens = samples[0]
    assert cli.main(["quantify", "-i", aln, "-g", grp, "-L", lens, "-o", str(tmp_path / "seed")]) == 0
    rec, _ = e2e_bench.write_reconstruct_inputs(str(tmp_path), str(tmp_path / "seed.multiway.genes.tpm"))
    gpos = np.load(rec["gpos"])
    rng = np.random.default_rng(3)
    points = {c: np.sort(rng.uniform(0.0, float(gpos[c]["f1"][-1]) + 500.0, size=9)) for c in reversed(gpos.files) if len(gpos[c])}
    grid_file = grid_cases.write_grid_file(tmp_path / "grid.txt", points)
    worker = SampleWorker(0)
    contexts = []
    for k, (aln, grp, lens) in enumerate(samples):
        job = dict(alignment_file=aln, group_file=grp, length_file=lens, outbase=str(tmp_path / f"wrk{k}"), diploid=False,
                   tprob_file=rec["tprob"], avec_file=rec["avecs"], gpos_file=rec["gpos"], grid_file=grid_file)
        out = worker.process(job)
        assert "grid" in out["reconstruct"]
        contexts.append(worker._ctx)
    assert contexts[0] is contexts[1] and contexts[0].grid_uploads == 1
    for k in range(2):
        stem = str(tmp_path / f"wrk{k}")
        postproc.interpolate(f"{stem}.genoprobs.npz", grid_file, rec["gpos"], f"{stem}.interp.npz")
        postproc.export(f"{stem}.interp.npz", list("ABCDEFGH"), grid_file, f"{stem}.export.tsv")
        header, numbers = grid_cases.read_tsv(f"{stem}.interpolated.genoprobs.tsv")
        ref_header, ref_numbers = grid_cases.read_tsv(f"{stem}.export.tsv")
        assert header == ref_header
        np.testing.assert_allclose(numbers, ref_numbers, rtol=0, atol=1.01e-6)
    assert not np.array_equal(grid_cases.read_tsv(str(tmp_path / "wrk0.interpolated.genoprobs.tsv"))[1],
                              grid_cases.read_tsv(str(tmp_path / "wrk1.interpolated.genoprobs.tsv"))[1])
    worker.close()
