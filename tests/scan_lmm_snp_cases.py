"""SNP sets, phenotypes and the two host computations of the SNP association under the mixed model (gbrs_scan_lmm_snps,
GenomeScan.run_snps_lmm): plain numpy, no GPU.  The cohorts, covariates and kinships are those of
tests/scan_lmm_cases.py, the SNP sets those of tests/scan_snp_cases.py on the same (H, n, cz, P, points).

snp_lmm_rule restates the rule itself - the SNP dosage rotated by its chromosome's eigenvectors, the null fit's weighted
columns g, o, c_k, the three sums, G = raw - S, the threshold, ess = b^2 / G - with numpy's sums.  snp_lmm_gls knows
nothing of the rotation or of the difference form: the dense V = h K + (1 - h) I, its Cholesky factor, np.linalg.lstsq
with rcond=1e-10 on the whitened [Z] and [Z | x].  Neither is the code under test; the worst difference between them, both
at the restatement's heritabilities, is the figure from which a case's tolerances are taken (scan_cases' scheme)."""
import functools

import numpy as np

import scan_cases as base
import scan_lmm_cases as lmm
import scan_snp_cases as snp

PIVOT = base.PIVOT                         # the used rule's threshold: G > PIVOT raw
UNDECIDED = (1e-12, 1e-8)                  # no ratio G / raw of a case may lie here: it could flip `used` by rounding
DEVICE_FACTOR = base.DEVICE_FACTOR
CPU_HEADROOM = base.CPU_HEADROOM
CASES, LARGE_CASES = lmm.CASES, lmm.LARGE_CASES
ALL_CASES = CASES + LARGE_CASES
EXTRA = 4                                  # phenotype columns added to a case: 3 x the dosage of a main-set SNP plus noise
case_id = lmm.case_id

# Worst |snp_lmm_rule - snp_lmm_gls| / max(1, |lod|) over the main SNP set of every case, both at the rule's
# heritabilities, measured on the CPU (test_scan_lmm_snp_cpu.py prints it): the measured numbers themselves, not bounds.
MEASURED_LMM_SNP = {
    'H8-n33-c2-P63-M22-loco': 2.69e-14, 'H8-n70-c2-P65-M28-loco': 3.33e-14, 'H4-n31-c1-P1-M38-loco': 5.28e-15,
    'H2-n32-c1-P5-M92-loco': 1.55e-14, 'H9-n65-c4-P7-M31-loco': 1.84e-14, 'H17-n64-c2-P3-M22-loco': 1.15e-14,
    'H8-n130-c3-P9-M63-loco': 1.87e-14, 'H8-n70-c16-P4-M28-loco': 3.16e-14, 'H8-n40-c2-P4-M17-loco': 3.49e-14,
    'H8-n10-c2-P2-M22-loco': 2.71e-14, 'H8-n33-c2-P4-M22-overall': 2.79e-14, 'H8-n33-c2-P4-M22-given': 2.38e-14,
    'H8-n70-c2-P24-M28-scaled': 2.04e-14, 'H8-n257-c2-P2-M75-loco': 2.48e-14, 'H17-n400-c2-P2-M60-loco': 3.86e-14,
}
# Over the 15 main sets `used` equals lstsq's rank for every (phenotype, SNP) pair; the smallest kept ratio G / raw and
# the largest skipped |G / raw| over all of them (expected() asserts that none lies in UNDECIDED):
SMALLEST_KEPT = 3.55e-3
LARGEST_SKIPPED = 6.57e-16
# The largest LODs of the main sets run from 4.1 (n = 10) to 47.8 (n = 400); eleven of the fifteen cases have one above 6.


def measured_floor(case):
    return MEASURED_LMM_SNP[case_id(case)]


def cpu_bound(case):
    return CPU_HEADROOM * measured_floor(case)


def device_tol(case):
    return DEVICE_FACTOR * measured_floor(case)


def snp_case(case):
    """The case as scan_snp_cases takes it: (H, n, c, P, points)."""
    return case[:5]


def snp_set(case, which='main', count=None):
    if which == 'main':
        return snp.main_set(snp_case(case))
    if which == 'descending':
        return snp.descending_set(snp_case(case))
    return snp.sized_set(snp_case(case), count)


@functools.lru_cache(maxsize=None)
def main_dosages(case):
    grid, pos, masks, _ = snp_set(case)
    X = snp.snp_dosage_rule(lmm.build(case)[0], case[4], grid, pos, masks)
    X.setflags(write=False)
    return X, [len(x) for x in pos]


def dosages(case, chosen=None):
    """X [n, M_snp] of a SNP set (default: the main set) by §29's rule, and the SNPs per chromosome."""
    if chosen is None:
        return main_dosages(case)
    grid, pos, masks, _ = chosen
    return snp.snp_dosage_rule(lmm.build(case)[0], case[4], grid, pos, masks), [len(x) for x in pos]


@functools.lru_cache(maxsize=None)
def phenotypes(case):
    """Y [n, P + EXTRA]: the case's phenotypes and EXTRA columns that carry 3 x the dosage of a main-set SNP (random
    patterns at random positions, spread over the chromosomes) plus unit noise, so that some LODs are well above 6."""
    Y = lmm.build(case)[2]
    X, _ = dosages(case)
    labels = snp_set(case)[3]
    rng = np.random.default_rng(81000 + 100 * case[0] + case[1])
    pool = [j for j, label in enumerate(labels) if label.endswith((':random', ':on', ':middle'))]
    picks = [pool[(k * len(pool)) // EXTRA] for k in range(EXTRA)]
    extra = np.column_stack([3.0 * X[:, j] + rng.normal(size=len(X)) for j in picks])
    out = np.hstack([Y, extra])
    out.setflags(write=False)
    return out


def snp_lmm_rule(X, counts, Z, Y, eigs, eig_of_chrom, hsq=None):
    """The rule.  X [n, M_snp] in handle order, counts the SNPs per chromosome, eigs [(U, lambda)], eig_of_chrom[c] the
    pair of chromosome c; hsq [P, n_eig] or None (the fixed search).  Returns lod [P, M_snp], used [P, M_snp], ratio G / raw
    [P, M_snp] (NaN where raw is 0) and hsq [P, n_eig]."""
    n, M = X.shape
    Y = lmm.centred(Y)
    P, cz = Y.shape[1], Z.shape[1]
    off = np.concatenate(([0], np.cumsum(counts)))
    out = {'lod': np.zeros((P, M)), 'used': np.zeros((P, M), dtype=bool), 'ratio': np.full((P, M), np.nan),
           'hsq': np.zeros((P, len(eigs)))}
    for e, (U, lam) in enumerate(eigs):
        cols = np.concatenate([np.arange(off[c], off[c + 1]) for c in range(len(counts)) if eig_of_chrom[c] == e] +
                              [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        Zs, Ys, Xs = U.T @ Z, U.T @ Y, U.T @ X[:, cols]
        for p in range(P):
            ys = Ys[:, p]
            flat = lmm.reml(0.0, ys, Zs, lam)[1] <= 0.0
            h = 0.0 if flat else lmm.search(ys, Zs, lam)[0] if hsq is None else float(hsq[p, e])
            out['hsq'][p, e] = h
            sw = np.sqrt(1.0 / (h * lam + (1.0 - h)))
            Q = lmm.gram_schmidt(sw[:, None] * Zs)
            yh = sw * ys
            yt = yh - Q @ (Q.T @ yh)
            rss0 = 0.0 if flat else yt @ yt
            g, o, C = sw * yt, sw * sw, sw[:, None] * Q
            b, raw, qtx = Xs.T @ g, (Xs * Xs).T @ o, Xs.T @ C
            S = np.zeros(len(cols))
            for k in range(cz):
                S = S + qtx[:, k] * qtx[:, k]
            G = raw - S
            used = (G > 0.0) & (G > PIVOT * raw)
            ess = b * b / np.where(used, G, 1.0)
            out['lod'][p, cols] = np.where(used, base.lod_of(n, rss0, rss0 - ess), 0.0)
            out['used'][p, cols] = used
            out['ratio'][p, cols] = np.where(raw > 0.0, G / np.where(raw > 0.0, raw, 1.0), np.nan)
    return out


def snp_lmm_gls(X, counts, Z, Y, kinships, kin_of_chrom, hsq):
    """(lod [P, M_snp], rank of x beside Z [P, M_snp]) by generalised least squares on the dense covariance, at the
    heritabilities given ([P, kinships])."""
    n, M = X.shape
    Y = lmm.centred(Y)
    P, cz = Y.shape[1], Z.shape[1]
    off = np.concatenate(([0], np.cumsum(counts)))
    lod, rank = np.zeros((P, M)), np.zeros((P, M), dtype=np.int32)
    for e, K in enumerate(kinships):
        cols = [j for c in range(len(counts)) if kin_of_chrom[c] == e for j in range(off[c], off[c + 1])]
        for p in range(P):
            h = float(hsq[p, e])
            C = np.linalg.cholesky(h * K + (1.0 - h) * np.eye(n))
            white = np.linalg.solve(C, np.hstack([Z, Y[:, p:p + 1], X[:, cols]]))
            Zw, yw, Xw = white[:, :cz], white[:, cz], white[:, cz + 1:]
            r0 = yw - Zw @ np.linalg.lstsq(Zw, yw, rcond=1e-10)[0]
            rss0 = 0.0 if (Y[:, p] == 0.0).all() else r0 @ r0
            for k, j in enumerate(cols):
                A = np.hstack([Zw, Xw[:, k:k + 1]])
                coef, _, rk, _ = np.linalg.lstsq(A, yw, rcond=1e-10)
                r1 = yw - A @ coef
                rank[p, j] = rk - cz
                lod[p, j] = base.lod_of(n, rss0, r1 @ r1) if rk > cz else 0.0
    return lod, rank


def snp_lmm_peaks(lod, used, counts):
    """(peak_lod, peak_index, n_used) [P, n_chrom]: the first of the largest over the used SNPs of a chromosome, NaN and
    -1 where it has none; `used` is [P, M_snp]."""
    off = np.concatenate(([0], np.cumsum(counts)))
    P = len(lod)
    peak, index = np.full((P, len(counts)), np.nan), np.full((P, len(counts)), -1, dtype=np.int64)
    count = np.zeros((P, len(counts)), dtype=np.int64)
    for ci, (a, b) in enumerate(zip(off[:-1], off[1:])):
        for p in range(P):
            on = a + np.flatnonzero(used[p, a:b])
            count[p, ci] = len(on)
            if len(on):
                index[p, ci] = on[lod[p, on].argmax()]
                peak[p, ci] = lod[p, index[p, ci]]
    return peak, index, count


def check_ratios(rule, rank):
    """`used` equals lstsq's rank for every pair and no ratio lies in UNDECIDED.  Returns (smallest kept, largest skipped
    |ratio|; NaN where there is none)."""
    assert np.array_equal(rule['used'], rank == 1)
    ratio = rule['ratio']
    with np.errstate(invalid='ignore'):
        assert not ((np.abs(ratio) > UNDECIDED[0]) & (np.abs(ratio) < UNDECIDED[1])).any()
    kept, skipped = ratio[rule['used']], np.abs(ratio[~rule['used'] & np.isfinite(ratio)])
    return (float(kept.min()) if len(kept) else np.nan), (float(skipped.max()) if len(skipped) else np.nan)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(X, counts, the rule's dict at its own heritabilities, the GLS route's lod and rank at the same) of a case's main
    set, computed once; asserts check_ratios."""
    D, Z, _, kinships, kin_of_chrom, _ = lmm.build(case)
    X, counts = dosages(case)
    Y = phenotypes(case)
    rule = snp_lmm_rule(X, counts, Z, Y, lmm.decompositions(case), kin_of_chrom)
    gls, rank = snp_lmm_gls(X, counts, Z, Y, kinships, kin_of_chrom, rule['hsq'])
    check_ratios(rule, rank)
    for a in [gls, rank] + list(rule.values()):
        a.setflags(write=False)
    return X, counts, rule, gls, rank


def per_decomposition(case, by_chrom):
    kin_of_chrom = lmm.build(case)[4]
    return by_chrom[:, [list(kin_of_chrom).index(e) for e in range(max(kin_of_chrom) + 1)]]


def flat_snps(case):
    """The SNPs of the main set with the all-zeros or the all-ones pattern whose dosage is the same in every sample."""
    X, labels = dosages(case)[0], snp_set(case)[3]
    return [j for j, label in enumerate(labels) if label.endswith((':zeros', ':ones')) and np.ptp(X[:, j]) < 1e-12]


def complement_pairs(case):
    """(a, b): a pattern and its complement at one position whose dosages add up to the same number in every sample."""
    X, labels = dosages(case)[0], snp_set(case)[3]
    pairs = [(labels.index(f'{ci}:pattern'), labels.index(f'{ci}:complement')) for ci, k in enumerate(case[4]) if k >= 5]
    return [(a, b) for a, b in pairs if np.ptp(X[:, a] + X[:, b]) < 1e-12]


deviation = base.deviation
