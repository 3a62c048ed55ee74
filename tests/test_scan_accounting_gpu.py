"""The scan's memory account (peak_device_bytes of every pass; needs an MI355X): a pass reports what the
handle holds - the SNPs, the kinship products, the mixed model and the interaction model included, whichever pass made them -
plus the buffers the call allocated for itself.  One tiny handle: 8 founders, 3 chromosomes of 4 grid points, 24 samples, an
intercept and one 0/1 covariate, 3 phenotypes, 4 SNPs, that covariate interacting."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, POINTS, N, P = 8, [4, 4, 4], 24, 3
PASSES = ("permute", "run_snps", "mediate", "effects", "run_lmm", "run_snps_lmm", "effects_lmm")


def problem():
    rng = np.random.default_rng(27)
    dosage = rng.dirichlet(np.ones(H), size=(N, sum(POINTS)))
    covariates = np.column_stack([np.ones(N), np.arange(N) % 2])
    pheno = rng.normal(size=(N, P))
    return dosage, covariates, pheno


def test_problem_is_regular():
    """What the handle checks, on the host: every leave-one-chromosome-out kinship has full rank (8 points x 7 free founders
    + 1 = 57 independent columns for 24 samples), and the interaction model's 14 columns leave degrees of freedom."""
    dosage, covariates, _ = problem()
    for c in range(len(POINTS)):
        keep = np.ones(sum(POINTS), dtype=bool)
        keep[4 * c:4 * c + 4] = False
        a = dosage[:, keep, :].reshape(N, -1)
        assert np.linalg.matrix_rank(a) == N
        lam = np.linalg.eigvalsh(a @ a.T)
        assert lam.min() > 1e-6 * lam.max()             # the handle refuses at 1e-10
    assert N > covariates.shape[1] + (H - 1) * 2


def open_scan():
    from gbrs_amd.scan import GenomeScan
    dosage, covariates, pheno = problem()
    scan = GenomeScan(H, POINTS)
    scan.append(dosage)
    scan.prepare(covariates)
    return scan, covariates, pheno


def set_snps(scan):
    grid = [np.arange(4.0)] * 3
    scan.set_snps(grid, [np.array([0.5, 2.25]), np.array([1.5]), np.array([3.0])],
                  [np.array([0x0F, 0x33], dtype=np.uint32), np.array([0x55], dtype=np.uint32), np.array([0x81], dtype=np.uint32)])


def run_pass(scan, name, pheno, **more):
    """One pass on the handle; its peak_device_bytes."""
    if name == "permute":
        scan.permute(pheno, 2, seed=1)
        return scan.perm_info()["peak_device_bytes"]
    if name == "run_snps":
        scan.run_snps(pheno)
        return scan.snp_info()["peak_device_bytes"]
    if name == "mediate":
        scan.mediate(pheno[:, 0], [5], pheno[:, 1:])
        return scan.mediate_info()["peak_device_bytes"]
    if name == "effects":
        scan.effects(pheno, [0, 2], [5, 9])
        return scan.effects_info()["peak_device_bytes"]
    if name == "run_lmm":
        scan.run_lmm(pheno, **more)
        return scan.lmm_info()["peak_device_bytes"]
    if name == "run_snps_lmm":
        scan.run_snps_lmm(pheno)
        return scan.lmm_snp_info()["peak_device_bytes"]
    scan.effects_lmm(pheno, [0, 2], [5, 9])
    return scan.lmm_effects_info()["peak_device_bytes"]


def test_a_pass_counts_the_snps_whoever_set_them():
    scan, _, pheno = open_scan()
    before = run_pass(scan, "permute", pheno)
    set_snps(scan)
    after = run_pass(scan, "permute", pheno)
    held = scan.snp_info()["device_bytes"]
    scan.close()
    assert held > 0 and after - before == held


def test_a_pass_counts_the_interaction_model():
    scan, covariates, pheno = open_scan()
    set_snps(scan)
    before = run_pass(scan, "run_snps", pheno)
    scan.prepare_int(covariates, [1])
    after = run_pass(scan, "run_snps", pheno)
    held = scan.int_info()["device_bytes"]
    scan.close()
    assert held > 0 and after - before == held


def test_every_pass_counts_everything_resident_and_nothing_twice():
    scan, covariates, pheno = open_scan()
    set_snps(scan)
    scan.prepare_lmm(covariates)
    scan.prepare_int(covariates, [1])
    resident = (scan.info()["device_bytes"] + scan.snp_info()["device_bytes"] + scan.lmm_info()["device_bytes"] +
                scan.int_info()["device_bytes"])
    peaks = {name: run_pass(scan, name, pheno) for name in PASSES}
    again = {name: run_pass(scan, name, pheno) for name in PASSES}
    with_support = run_pass(scan, "run_lmm", pheno, lod_drop=1.5)
    timed = {"run_lmm": scan.lmm_info(), "effects_lmm": scan.lmm_effects_info(), "run_snps_lmm": scan.lmm_snp_info()}
    scan.close()
    for name in PASSES:
        assert peaks[name] > resident, name                      # the call's own buffers on top of all the handle holds
        assert again[name] == peaks[name], name                  # a call's tally starts at nothing
    # the two interval tables of a chunk, int64 [min(P, 512)][n_chrom], and nothing else
    assert with_support - peaks["run_lmm"] == 2 * min(P, 512) * len(POINTS) * 8
    # the timed regions as gbrs_hip.h words them: each null fit is a part of its pass
    assert timed["run_lmm"]["run_ms"] >= timed["run_lmm"]["null_ms"] > 0
    assert timed["effects_lmm"]["pass_ms"] >= timed["effects_lmm"]["null_ms"] > 0
    assert timed["run_snps_lmm"]["pass_ms"] >= timed["run_snps_lmm"]["null_ms"] > 0
