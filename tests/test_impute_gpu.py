"""The imputation pass of the HIP HMM (gbrs_hmm_set_snps / gbrs_hmm_impute) and `gbrs reconstruct --snp-file`,
`--snp-matrix` over it (needs an MI355X).  The rule restated in numpy, the SNP sets and the composed oracle:
tests/impute_cases.py; shapes and problems: tests/grid_cases.py.

Three comparisons.  Against the restatement on the device's own posteriors the kernel takes the same operations in the
same order and the library is built without FMA contraction.  Against the device's own grid route (36 states interpolated
first, founders reduced second) and against the composed CPU oracle the two orders differ by reassociation, and the
oracle's posteriors carry their own 1e-8."""
import os

import numpy as np
import pytest

import grid_cases
import impute_cases

pytestmark = pytest.mark.gpu

FOUNDERS = (1, 2, 3, 8, 16)
CASES = [(H, "benign") for H in FOUNDERS] + [(8, "do")]


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


def restated(hmm, p0, snps, masks, sample):
    return impute_cases.impute(p0.chroms, snps, masks,
                               lambda c: hmm.get(p0.chroms.index(c), sample=sample, want=("gamma",))["gamma"], hmm.H)


def reassociation_atol(H):
    """8 (S + H + 8) 2^-53: both orders round at most 2 S + H + 6 times on terms <= 1, doubled by the final factor."""
    return 8 * (H * (H + 1) // 2 + H + 8) * 2.0 ** -53


@pytest.mark.parametrize("H,style", CASES)
def test_impute_equals_the_restatement_on_the_devices_posteriors(H, style):
    """Every SNP set, one sample: the rule restated on hmm.get's gamma, bit for bit - the kernel takes the restatement's
    operations in its order and nothing is contracted, so the H + 4 roundings of values <= 2 that would bound two
    orders apart do not come into it (a wrong gene row, knot, pattern bit or chromosome offset shows as another gene's or
    founder's numbers)."""
    hmm, p0 = run_samples(H, style, [0])
    for name, snps in impute_cases.snp_sets().items():
        masks = impute_cases.masks_for(name, H)
        hmm.set_snps(snps.positions, snps.points, masks)
        M = sum(len(x) for x in snps.points.values())
        assert hmm.snp_points == [len(snps.points.get(c, ())) for c in p0.chroms]
        assert hmm.snp_offsets == [int(o) for o in np.concatenate(([0], np.cumsum(hmm.snp_points)[:-1]))]
        info = hmm.impute_info()
        assert info["n_snps"] == M and info["device_bytes"] >= 16 * M
        got = hmm.impute(sample=0)
        assert got.shape == (M,) and hmm.impute().shape == (1, M)
        want = restated(hmm, p0, snps, masks, 0)
        worst = float(np.abs(got - want).max())
        print(f"DEVIATION impute against the restatement, H={H} {style} set {name}: {worst:.3g} "
              f"(the bound of H + 4 roundings of values <= 2: {(H + 4) * 2.0 ** -52:.3g})")
        np.testing.assert_array_equal(got, want, err_msg=f"set {name}")         # the build gives the same bits (§26)
        zero = np.concatenate([masks[c] for c in p0.chroms if c in snps.points]) == 0
        assert (got[zero] == 0.0).all()
        assert hmm.impute_info()["last_ms"] > 0.0
    hmm.close()


@pytest.mark.parametrize("H,style", CASES)
def test_impute_equals_the_grid_route_on_the_same_handle(H, style):
    """set_grid with the SNP positions, grid()['dosage'], the pattern folded in numpy: the route that existed before the
    pass, which interpolates the states first."""
    hmm, p0 = run_samples(H, style, [0])
    for name, snps in impute_cases.snp_sets().items():
        masks = impute_cases.masks_for(name, H)
        hmm.set_snps(snps.positions, snps.points, masks)
        hmm.set_grid(snps.positions, snps.points)
        dosage = hmm.grid(sample=0)["dosage"]
        bits = np.vstack([impute_cases.bits_of(masks[c], H) for c in p0.chroms if c in snps.points])
        want = 2.0 * (dosage * bits).sum(-1)
        got = hmm.impute(sample=0)
        print(f"DEVIATION impute against the grid route, H={H} {style} set {name}: {np.abs(got - want).max():.3g} "
              f"(bound {reassociation_atol(H):.3g})")
        np.testing.assert_allclose(got, want, rtol=0, atol=reassociation_atol(H), err_msg=f"set {name}")
    hmm.close()


@pytest.mark.parametrize("H,style", CASES)
def test_impute_against_the_composed_oracle(H, style):
    """reconstruct_arrays + interpolate + dosage on the CPU, folded with the patterns: rtol 1e-8 is the posterior's own
    tolerance and atol 2 S 2^-53 the dosage sum's in tests/test_grid_gpu.py, the latter doubled by the factor in `out`;
    a pattern only drops non-negative terms."""
    hmm, p0 = run_samples(H, style, [0])
    S = hmm.S
    p = grid_cases.sample_problem(H, style, 0)
    res = grid_cases.oracle_arrays(H, style, 0)[0]
    for name, snps in impute_cases.snp_sets().items():
        masks = impute_cases.masks_for(name, H)
        hmm.set_snps(snps.positions, snps.points, masks)
        want = impute_cases.handle_order(p0.chroms, snps, impute_cases.composed(
            p, snps, masks, res, sorted_knots=name in impute_cases.NEEDS_SORTED_KNOTS))
        np.testing.assert_allclose(hmm.impute(sample=0), want, rtol=1e-8, atol=2 * 2 * S * 2.0 ** -53, err_msg=f"set {name}")
    hmm.close()


@pytest.mark.parametrize("n", (1, 3, 25))
def test_a_samples_row_does_not_depend_on_the_batch_or_the_chunk(n):
    """1, 3 and 25 samples at 8 founders, 260 SNPs over two chromosomes (a workgroup and one lane on the first): the row
    of a sample is the same bits asked for alone and in the batch, and for chunks of 1, 7, 256 and all SNPs."""
    H = 8
    hmm, p0 = run_samples(H, "benign", range(n))
    snps = impute_cases.snp_sets()["n257"]
    masks = impute_cases.masks_for("n257", H)
    hmm.set_snps(snps.positions, snps.points, masks)
    M = hmm.impute_info()["n_snps"]
    assert M == 260
    whole = hmm.impute(chunk=M)
    assert whole.shape == (n, M)
    for chunk in (1, 7, 256):
        np.testing.assert_array_equal(hmm.impute(chunk=chunk), whole, err_msg=f"chunk {chunk}")
    for k in sorted({0, n // 2, n - 1}):
        np.testing.assert_array_equal(hmm.impute(sample=k), whole[k], err_msg=f"sample {k} alone")
        np.testing.assert_array_equal(hmm.impute(sample=k, chunk=7), whole[k], err_msg=f"sample {k} alone, chunk 7")
        np.testing.assert_array_equal(whole[k], restated(hmm, p0, snps, masks, k), err_msg=f"sample {k}")
    np.testing.assert_array_equal(hmm.impute(), whole)           # after single samples the batch is made again
    hmm.close()


def test_abi_edges():
    """impute before a run: GBRS_ERR_STATE.  Without SNPs, a range outside 0 .. M, a sample out of range, a pattern bit at
    or above H: GBRS_ERR_INVALID, outputs untouched, the handle keeps its SNPs.  count = 0 is accepted.  A SNP beyond the
    knots: the grid's text.  set_grid and set_panel leave impute() as it was; all zeros drops the SNPs."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.hmm import DiplotypeHMM
    lib = _lib.load()
    H = 3
    p0 = grid_cases.problem(H, "benign")
    snps = impute_cases.snp_sets()["a"]
    masks = impute_cases.masks_for("a", H)
    M = sum(len(x) for x in snps.points.values())
    out = np.full((2, M), -1.0)

    def call(hmm, sample, first, count):
        return lib.gbrs_hmm_impute(hmm._h, sample, C.c_int64(first), C.c_int64(count), _lib.ptr(out))

    def untouched():
        return (out == -1.0).all()

    fresh = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    fresh.set_snps(snps.positions, snps.points, masks)
    assert call(fresh, -1, 0, M) == _lib.GBRS_ERR_STATE and untouched()
    assert fresh.impute_info()["last_ms"] == 0.0
    fresh.close()

    hmm, p0 = run_samples(H, "benign", range(2))
    assert hmm.impute_info()["n_snps"] == 0 and hmm.impute_info()["last_ms"] == 0.0
    assert call(hmm, -1, 0, M) == _lib.GBRS_ERR_INVALID and b"no SNPs" in lib.gbrs_last_error() and untouched()
    with pytest.raises(_lib.GbrsHipError):
        hmm.impute()
    hmm.set_snps(snps.positions, snps.points, masks)
    for first, count in ((-1, 1), (0, M + 1), (M, 1), (M + 1, 0), (0, -1), (1, M)):
        assert call(hmm, -1, first, count) == _lib.GBRS_ERR_INVALID and untouched(), (first, count)
    for sample in (2, -2, 25):
        assert call(hmm, sample, 0, M) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error() and untouched()
    assert call(hmm, -1, 0, 0) == _lib.GBRS_OK and call(hmm, -1, M, 0) == _lib.GBRS_OK and untouched()
    assert lib.gbrs_hmm_impute(hmm._h, -1, C.c_int64(3), C.c_int64(0), None) == _lib.GBRS_OK
    assert lib.gbrs_hmm_impute(None, -1, C.c_int64(0), C.c_int64(M), _lib.ptr(out)) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_hmm_impute_info(hmm._h, None, None, None) == _lib.GBRS_OK
    before = hmm.impute()
    # a sub-range is those columns
    assert call(hmm, 1, 5, 9) == _lib.GBRS_OK
    np.testing.assert_array_equal(out.ravel()[:9], before[1, 5:14])
    assert (out.ravel()[9:] == -1.0).all()

    # a pattern bit at or above H: refused, names chromosome and index, the SNPs stay
    bad = {c: m.copy() for c, m in masks.items()}
    bad["3"][7] |= np.uint32(1 << H)
    with pytest.raises(_lib.GbrsHipError, match="chromosome 2, SNP 7"):
        hmm.set_snps(snps.positions, snps.points, bad)
    assert lib.gbrs_last_error() and hmm.impute_info()["n_snps"] == M
    np.testing.assert_array_equal(hmm.impute(), before)
    # a SNP beyond the knots: the grid's text, the SNPs stay
    below = dict(snps.points, **{"3": np.concatenate(([-0.5], snps.points["3"][1:]))})
    with pytest.raises(ValueError, match="below the interpolation range"):
        hmm.set_snps(snps.positions, below, masks)
    above = dict(snps.points, **{"4": np.concatenate((snps.points["4"][:-1] + 1000.0, snps.points["4"][-1:]))})
    with pytest.raises(ValueError, match="above the interpolation range"):
        hmm.set_snps(snps.positions, above, masks)
    with pytest.raises(IndexError):
        hmm.set_snps(dict(snps.positions, **{"2": np.zeros(0)}), snps.points, masks)
    np.testing.assert_array_equal(hmm.impute(), before)

    # the grid and the panel are independent of the SNPs
    grid = grid_cases.grids()["b"]
    hmm.set_grid(grid.positions, grid.points)
    np.testing.assert_array_equal(hmm.impute(), before)
    G = sum(len(x) for x in grid.points.values())
    hmm.set_panel([np.full((G, H), 1.0 / H)])
    hmm.match()
    np.testing.assert_array_equal(hmm.impute(), before)
    dosage = hmm.grid()["dosage"]
    hmm.set_snps(snps.positions, snps.points, masks)             # and the SNPs leave the grid and the panel alone
    np.testing.assert_array_equal(hmm.grid()["dosage"], dosage)
    assert hmm.match_info()["n_panel"] == 1 and hmm.grid_info()[0] == G

    # all zeros drops the SNPs
    hmm.set_snps(snps.positions, {}, {})
    assert hmm.impute_info()["n_snps"] == 0 and hmm.snp_points == [0] * len(p0.chroms)
    out[:] = -1.0
    assert call(hmm, -1, 0, 0) == _lib.GBRS_ERR_INVALID and b"no SNPs" in lib.gbrs_last_error() and untouched()
    hmm.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES, SET_FILES = 8, "benign", "b"
RECONSTRUCTION = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz")


@pytest.fixture
def tables(tmp_path, monkeypatch):
    """$GBRS_DATA with the table's 8-founder problem and a SNP file of set "b" - its chromosome order is not the
    genome's - with two SNPs on MT, which has no transition table, at the end."""
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    snps = impute_cases.snp_sets()[SET_FILES]
    paths = grid_cases.write_tables(tmp_path, p0, snps.positions)
    paths["snps"] = impute_cases.write_snp_file(tmp_path / "snps.tsv", H_FILES, snps.points,
                                                impute_cases.masks_for(SET_FILES, H_FILES),
                                                extra=[("MT", 1.0, "10000000"), ("MT", 2.0, "11111111")])
    return paths


def sample_tpm(tmp_path, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, sample))


def direct(samples):
    """impute() of the samples on a handle of the test's own, in the SNP file's order with nan for the two MT lines."""
    hmm, p0 = run_samples(H_FILES, STYLE_FILES, samples)
    snps = impute_cases.snp_sets()[SET_FILES]
    hmm.set_snps(snps.positions, snps.points, impute_cases.masks_for(SET_FILES, H_FILES))
    got = hmm.impute()                                            # handle order
    hmm.close()
    first, col = {}, 0
    for c in p0.chroms:
        if c in snps.points:
            first[c] = col
            col += len(snps.points[c])
    in_file_order = np.concatenate([got[:, first[c]:first[c] + len(x)] for c, x in snps.points.items()], axis=1)
    return np.concatenate((in_file_order, np.full((len(got), 2), np.nan)), axis=1)


def test_reconstruct_with_a_snp_file(tmp_path, tables, caplog):
    from gbrs_amd import cli
    tpm = sample_tpm(tmp_path, 0)
    common = ["reconstruct", "-e", tpm, "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"]]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["--snp-file", tables["snps"], "-o", str(tmp_path / "with")]) == 0
    assert sorted(f.name for f in tmp_path.glob("plain.*")) == sorted(f"plain.{s}" for s in RECONSTRUCTION)
    assert sorted(f.name for f in tmp_path.glob("with.*")) == sorted(f"with.{s}" for s in RECONSTRUCTION + ("snp_dosage.npz",))
    for suffix in RECONSTRUCTION:
        assert (tmp_path / f"with.{suffix}").read_bytes() == (tmp_path / f"plain.{suffix}").read_bytes(), suffix
    z = np.load(tmp_path / "with.snp_dosage.npz")
    want = direct([0])[0]
    assert z["dosage"].dtype == np.float64 and z["dosage"].shape == want.shape
    np.testing.assert_array_equal(z["dosage"], want)               # nan at the same two places
    assert np.isnan(z["dosage"][-2:]).all() and not np.isnan(z["dosage"][:-2]).any()
    assert z["snp_id"].tolist() == [f"snp{k}" for k in range(len(want))]
    assert any("2 SNPs" in r.getMessage() for r in caplog.records)


def test_reconstruct_many_with_a_snp_matrix(tmp_path, tables):
    from gbrs_amd import cli
    samples = (0, 1, 2)
    with open(tmp_path / "cohort.tsv", "w") as fh:
        for s in samples:
            fh.write(f"{sample_tpm(tmp_path, s)}\t{tmp_path / f'out{s}'}\n")
        fh.write(f"{tmp_path / 'missing.genes.tpm'}\t{tmp_path / 'out9'}\n")          # a sample that fails
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "cohort.tsv"), "-t", tables["tprob"], "-x", tables["avecs"],
                     "-g", tables["gpos"], "--snp-file", tables["snps"], "--snp-matrix", str(tmp_path / "all.npz")]) == 0
    z = np.load(tmp_path / "all.npz")
    want = direct(samples)
    assert z["outbases"].tolist() == [str(tmp_path / f"out{s}") for s in samples]    # the failed sample is left out
    np.testing.assert_array_equal(z["dosage"], want)
    for k, s in enumerate(samples):
        one = np.load(tmp_path / f"out{s}.snp_dosage.npz")
        np.testing.assert_array_equal(one["dosage"], z["dosage"][k])
        assert one["snp_id"].tolist() == z["snp_id"].tolist()
    assert not (tmp_path / "out9.snp_dosage.npz").exists()
    snps = impute_cases.snp_sets()[SET_FILES]
    assert z["chrom"].tolist() == [c for c, x in snps.points.items() for _ in x] + ["MT", "MT"]
    np.testing.assert_array_equal(z["cM"], np.concatenate(list(snps.points.values()) + [[1.0, 2.0]]))
    assert z["bp"].shape == z["cM"].shape and z["pattern"].tolist()[-1] == "11111111"
    masks = impute_cases.masks_for(SET_FILES, H_FILES)
    assert z["pattern"].tolist()[0] == impute_cases.pattern_text(masks[next(iter(snps.points))][0], H_FILES)


def test_without_a_snp_file_nothing_changes(tmp_path, tables):
    """The files of a cohort run are the parent's, and a handle that never saw SNPs reports none and no pass."""
    from gbrs_amd import hmm as HM
    tpm = sample_tpm(tmp_path, 0)
    ctx = HM.ReconstructContext(tables["tprob"], tables["avecs"], tables["gpos"])
    HM.reconstruct_many([tpm], [str(tmp_path / "solo")], tables["tprob"], context=ctx)
    assert sorted(f.name for f in tmp_path.glob("solo.*")) == sorted(f"solo.{s}" for s in RECONSTRUCTION)
    info = ctx.hmm.impute_info()
    assert info["n_snps"] == 0 and info["last_ms"] == 0.0 and ctx.snp_uploads == 0
    HM.reconstruct_many([tpm, tpm], [str(tmp_path / "x0"), str(tmp_path / "x1")], tables["tprob"], context=ctx, batch_size=1,
                        snp_file=tables["snps"])
    assert ctx.snp_uploads == 1                                    # once per handle, not per launch
    for suffix in RECONSTRUCTION:
        assert (tmp_path / f"x1.{suffix}").read_bytes() == (tmp_path / f"solo.{suffix}").read_bytes(), suffix
    ctx.close()
