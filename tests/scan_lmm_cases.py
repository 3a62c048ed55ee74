"""Cohorts, phenotypes and the two host computations of the mixed-model genome scan (gbrs_scan_kinship, gbrs_scan_lmm_*,
GenomeScan.prepare_lmm / run_lmm): plain numpy, no GPU.

lmm_rule restates the rule itself - the kinship's eigenvectors rotate the cohort, the REML search of the heritability on
its fixed steps, the weighted projection on the covariates' Gram-Schmidt basis, §27's Gram matrix, skip rule and solve -
and nothing else.  lmm_gls knows nothing of the rule and never rotates: the dense V = h K + (1 - h) I, its Cholesky
factor, np.linalg.lstsq with rcond=1e-10 on the whitened [Z] and [Z | X_m].  Neither is the code under test; the worst
difference between them, both at the restatement's heritabilities, is the floor from which the device tolerance is
taken (scan_cases' scheme)."""
import functools

import numpy as np

import scan_cases as base

GRID_STEPS = 20                            # f is first looked at on k / 20, k = 0 .. 20
GOLDEN_STEPS = 48                          # then exactly this many golden-section steps
INVPHI = (np.sqrt(5.0) - 1.0) / 2.0
LAMBDA_FLOOR = 1e-10                       # every eigenvalue must exceed this share of the largest
CASE_LAMBDA = 1e-6                         # what the case builder asks of its own kinships
ENDPOINT_MARGIN = 1e-9                     # a boundary optimum is compared with == only when f says so by more than this

# (H, n, cz, P, points per chromosome, kinship mode).  The first seven are the issue's shapes with P 63, 65 and 1 among
# them; then cz = 16, a chromosome of one point, n = cz + H (one residual degree of freedom), the overall kinship, a
# kinship the caller brings, and the caller's own LOCO matrices at 1,024 times the usual scale: the LODs are the same,
# f's slope at the ends of [0, 1] is 1,024 times as steep, and so the boundary optima of this case are decided by a
# margin far above rounding (ENDPOINT_MARGIN).  Every case has a point where founder 0 is exactly zero and (H >= 3) one where founders 0 and
# 1 are exactly equal, on its last chromosome.
CASES = [
    (8, 33, 2, 63, (6, 7, 9), 'loco'),
    (8, 70, 2, 65, (12, 7, 9), 'loco'),
    (4, 31, 1, 1, (12, 17, 9), 'loco'),
    (2, 32, 1, 5, (40, 7, 45), 'loco'),
    (9, 65, 4, 7, (10, 12, 9), 'loco'),
    (17, 64, 2, 3, (6, 7, 9), 'loco'),
    (8, 130, 3, 9, (20, 22, 21), 'loco'),
    (8, 70, 16, 4, (12, 7, 9), 'loco'),
    (8, 40, 2, 4, (1, 7, 9), 'loco'),
    (8, 10, 2, 2, (6, 7, 9), 'loco'),
    (8, 33, 2, 4, (6, 7, 9), 'overall'),
    (8, 33, 2, 4, (6, 7, 9), 'given'),
    (8, 70, 2, 24, (12, 7, 9), 'scaled'),
]
# Past the first K chunk of every kernel (n = 257: nine chunks of 32 samples, a second lap of the 256-thread loops) and,
# at H = 17 with 400 samples, past the size up to which lmm_point_kernel keeps a point's columns in LDS.  Apart from CASES
# so that what is measured over CASES stays as it is.
LARGE_CASES = [
    (8, 257, 2, 2, (25, 25, 25), 'loco'),
    (17, 400, 2, 2, (20, 20, 20), 'loco'),
]

# Worst |lmm_rule - lmm_gls| / max(1, |lod|) per case, both at lmm_rule's heritabilities, measured on the CPU
# (test_scan_lmm_cpu.py prints them).  These are the measured numbers themselves, not bounds on them.
MEASURED_LMM = {
    'H8-n33-c2-P63-M22-loco': 1.24e-14, 'H8-n70-c2-P65-M28-loco': 2.26e-14, 'H4-n31-c1-P1-M38-loco': 3.76e-15,
    'H2-n32-c1-P5-M92-loco': 1.18e-14, 'H9-n65-c4-P7-M31-loco': 1.2e-14, 'H17-n64-c2-P3-M22-loco': 3.39e-15,
    'H8-n130-c3-P9-M63-loco': 1.53e-14, 'H8-n70-c16-P4-M28-loco': 9.66e-15, 'H8-n40-c2-P4-M17-loco': 5.77e-15,
    'H8-n10-c2-P2-M22-loco': 5.77e-12,       # n = cz + H: one residual degree of freedom, LODs up to 27 from 10 samples
    'H8-n33-c2-P4-M22-overall': 5.7e-15, 'H8-n33-c2-P4-M22-given': 6.86e-15, 'H8-n70-c2-P24-M28-scaled': 1.59e-14,
    'H8-n257-c2-P2-M75-loco': 2.45e-14, 'H17-n400-c2-P2-M60-loco': 1.92e-14,
}
# Ten times the largest change of lmm_rule's fitted heritability over CASES when y*, Z* and lambda are each multiplied by
# 1 + r 2^-50 with r uniform in [-1, 1] (measure_hsq below): the minimum of f is flat, so a rounding of f moves the last
# golden-section steps.  The largest change measured is 2.46e-7.
MEASURED_HSQ = 2.46e-6
# LODs under `scale` and 4 `scale`: the eigenvalues are four times as large, each run fits its own heritability, and the
# two searches stop at slightly different places of the same flat minimum; the LODs feel that to first order.  The worst
# |difference| / max(1, |lod|) measured over CASES.
MEASURED_SCALE = 1.09e-7


def case_id(case):
    H, n, cz, P, points, mode = case
    return f'H{H}-n{n}-c{cz}-P{P}-M{sum(points)}-{mode}'


def measured_floor(case):
    return MEASURED_LMM[case_id(case)]


def cpu_bound(case):
    return base.CPU_HEADROOM * measured_floor(case)


def device_tol(case):
    return base.DEVICE_FACTOR * measured_floor(case)


def kinship(D, points, leave_out=None, scale=2.0):
    """scale * (sum over the chromosomes c' != leave_out of A_c' A_c'', added in chromosome order) / (their grid points)."""
    n = len(D)
    off = np.concatenate(([0], np.cumsum(points)))
    acc, count = np.zeros((n, n)), 0
    for c, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if c == leave_out or a == b:
            continue
        A = D[:, a:b, :].reshape(n, -1)
        acc = acc + A @ A.T
        count += b - a
    return scale * acc / count


def kinship_longdouble(D, points, leave_out=None, scale=2.0):
    """The same sums accumulated in np.longdouble, rounded once at the end."""
    n = len(D)
    off = np.concatenate(([0], np.cumsum(points)))
    acc, count = np.zeros((n, n), dtype=np.longdouble), 0
    for c, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if c == leave_out or a == b:
            continue
        A = D[:, a:b, :].reshape(n, -1).astype(np.longdouble)
        acc = acc + np.stack([(A[k] * A).sum(axis=1) for k in range(n)])
        count += b - a
    return (np.longdouble(scale) * acc / count).astype(np.float64)


@functools.lru_cache(maxsize=None)
def build(case):
    """(D [n, M, H], Z [n, cz], Y [n, P], kinships, kin_of_chrom, special points) of a case.  kinships: the distinct
    matrices (one per chromosome for 'loco', one otherwise), kin_of_chrom[c] the matrix chromosome c is scanned with.
    Phenotype p is sqrt(g) u + sqrt(1 - g) e with u drawn from the overall kinship, g = (0, 0.3, 0.6, 0.9)[p % 4], and
    every third one has a founder's dosage at some grid point added."""
    H, n, cz, P, points, mode = case
    rng = np.random.default_rng(100 * H + n)
    M = sum(points)
    D = rng.dirichlet(np.ones(H), size=(n, M))
    first = M - points[-1]
    special = {'zero': first + 1}
    D[:, special['zero'], 0] = 0.0
    D[:, special['zero']] /= D[:, special['zero']].sum(axis=1, keepdims=True)
    if H >= 3:
        special['equal'] = first + 2
        D[:, special['equal'], 1] = D[:, special['equal'], 0]
    Z = np.ones((n, cz))
    Z[:, 1:] = rng.normal(size=(n, cz - 1))
    if cz >= 2:
        Z[:, 1] = rng.integers(0, 2, size=n)
        Z[0, 1], Z[1, 1] = 0.0, 1.0
    overall = kinship(D, points)
    if mode == 'loco':
        kinships = [kinship(D, points, leave_out=c) for c in range(len(points))]
        kin_of_chrom = list(range(len(points)))
    elif mode == 'scaled':
        kinships = [1024.0 * kinship(D, points, leave_out=c) for c in range(len(points))]
        kin_of_chrom = list(range(len(points)))
    elif mode == 'overall':
        kinships, kin_of_chrom = [overall], [0] * len(points)
    else:                                   # the caller's own: the overall one shrunk towards the identity
        kinships, kin_of_chrom = [0.9 * overall + 0.1 * np.eye(n)], [0] * len(points)
    root = np.linalg.cholesky(overall / np.mean(np.diag(overall)))
    Y = np.empty((n, P))
    for p in range(P):
        g = (0.0, 0.3, 0.6, 0.9)[p % 4]
        Y[:, p] = np.sqrt(g) * (root @ rng.normal(size=n)) + np.sqrt(1.0 - g) * rng.normal(size=n)
        if p % 3 == 0:
            Y[:, p] += 3.0 * D[:, rng.integers(0, M), rng.integers(0, H)]
    for a in [D, Z, Y] + kinships:
        a.setflags(write=False)
    return D, Z, Y, kinships, kin_of_chrom, special


def decompose(K):
    """(U, lambda) of a kinship by numpy's eigh, refused as gbrs_amd.scan refuses it."""
    lam, U = np.linalg.eigh(K)
    assert np.isfinite(lam).all() and lam.min() > LAMBDA_FLOOR * lam.max()
    return np.ascontiguousarray(U), lam


def centred(Y):
    """What run_lmm uploads: every column minus its mean, a constant column as zeros."""
    y = np.array(Y, dtype=np.float64)
    if y.ndim == 1:
        y = y[:, None]
    constant = (y == y[0]).all(axis=0)
    y = y - y.mean(axis=0)
    y[:, constant] = 0.0
    return y


def reml(h, ys, Zs, lam):
    """(f(h), rss) of one phenotype in one rotation; f is +inf where rss <= 0."""
    n, cz = Zs.shape
    v = h * lam + (1.0 - h)
    om = 1.0 / v
    A = Zs.T @ (om[:, None] * Zs)
    b = Zs.T @ (om * ys)
    L = np.linalg.cholesky(A)
    t = np.linalg.solve(L, b)
    rss = (om * ys) @ ys - t @ t
    if rss <= 0.0:
        return np.inf, rss
    return (n - cz) * np.log(rss) + np.log(v).sum() + 2.0 * np.log(np.diag(L)).sum(), rss


def search(ys, Zs, lam):
    """(hsq, margin) by the fixed search: the grid, the bracket, 48 golden-section steps, the endpoint rule.  margin: at
    a boundary optimum f(midpoint) - f(endpoint), NaN at an interior one."""
    f = lambda h: reml(h, ys, Zs, lam)[0]
    grid = [f(k / GRID_STEPS) for k in range(GRID_STEPS + 1)]
    best = int(np.argmin(grid))                       # the lowest k on ties
    a, b = max(best - 1, 0) / GRID_STEPS, min(best + 1, GRID_STEPS) / GRID_STEPS
    c, d = b - INVPHI * (b - a), a + INVPHI * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(GOLDEN_STEPS):
        if fc <= fd:                                  # on equal f the left point stays
            b, d, fd = d, c, fc
            c = b - INVPHI * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + INVPHI * (b - a)
            fd = f(d)
    h = 0.5 * (a + b)
    fh, margin = f(h), np.nan
    if a == 0.0 and grid[0] <= fh:
        h, margin, fh = 0.0, fh - grid[0], grid[0]
    if b == 1.0 and grid[GRID_STEPS] <= fh:
        h, margin = 1.0, fh - grid[GRID_STEPS]
    return h, margin


def gram_schmidt(Zh):
    """Modified Gram-Schmidt in column order, each column swept twice over the ones before it, then normalised."""
    Q = np.array(Zh, dtype=np.float64)
    for j in range(Q.shape[1]):
        for _ in range(2):
            for k in range(j):
                Q[:, j] -= (Q[:, k] @ Q[:, j]) * Q[:, k]
        Q[:, j] /= np.sqrt(Q[:, j] @ Q[:, j])
    return Q


def lmm_rule(D, Z, Y, points, eigs, eig_of_chrom, hsq=None, perturb=None):
    """The rule.  eigs: [(U, lambda)], eig_of_chrom[c] the pair of chromosome c.  Returns a dict: lod [P, M], hsq, sigma2,
    margin [P, n_eig], rank_min, rank_max [P], ratios [P, M, H - 1] (the weighted pivot ratios).  hsq [P, n_eig]: the
    search is skipped.  perturb (what, rng): y*, Z* or lambda multiplied by 1 + r 2^-50 (measure_hsq)."""
    n, M, H = D.shape
    Y = centred(Y)
    P, cz = Y.shape[1], Z.shape[1]
    off = np.concatenate(([0], np.cumsum(points)))
    out = {'lod': np.zeros((P, M)), 'hsq': np.zeros((P, len(eigs))), 'sigma2': np.zeros((P, len(eigs))),
           'margin': np.full((P, len(eigs)), np.nan), 'ratios': np.full((P, M, H - 1), np.nan),
           'rank_min': np.full(P, H, dtype=np.int32), 'rank_max': np.zeros(P, dtype=np.int32)}
    for e, (U, lam) in enumerate(eigs):
        Zs, Ys = U.T @ Z, U.T @ Y
        if perturb is not None:
            what, rng = perturb
            jitter = lambda a: a * (1.0 + rng.uniform(-1.0, 1.0, size=a.shape) * 2.0 ** -50)
            Zs, Ys, lam = (jitter(Zs) if what == 'Z' else Zs, jitter(Ys) if what == 'y' else Ys,
                           jitter(lam) if what == 'lambda' else lam)
        chroms = [c for c in range(len(points)) if eig_of_chrom[c] == e]
        R = {m: U.T @ D[:, m, :H - 1] for c in chroms for m in range(off[c], off[c + 1])}
        for p in range(P):
            ys = Ys[:, p]
            flat = reml(0.0, ys, Zs, lam)[1] <= 0.0          # the constant column: hsq 0, rss0 0 and so LODs 0.0
            if flat:
                h = 0.0
            elif hsq is None:
                h, out['margin'][p, e] = search(ys, Zs, lam)
            else:
                h = float(hsq[p, e])
            out['hsq'][p, e] = h
            out['sigma2'][p, e] = 0.0 if flat else reml(h, ys, Zs, lam)[1] / (n - cz)
            if perturb is not None:
                continue
            sw = np.sqrt(1.0 / (h * lam + (1.0 - h)))
            Q = gram_schmidt(sw[:, None] * Zs)
            yh = sw * ys
            yt = yh - Q @ (Q.T @ yh)
            rss0 = 0.0 if flat else yt @ yt
            for m, Rm in R.items():
                X = sw[:, None] * Rm
                Xt = X - Q @ (Q.T @ X)
                L, keep, out['ratios'][p, m] = base.factor(Xt.T @ Xt, (X * X).sum(axis=0))
                b = Xt.T @ yt
                z = np.zeros(H - 1)
                for j in np.flatnonzero(keep):
                    z[j] = (b[j] - L[j, :j] @ z[:j]) / L[j, j]
                out['lod'][p, m] = base.lod_of(n, rss0, rss0 - z @ z)
                out['rank_min'][p] = min(out['rank_min'][p], keep.sum())
                out['rank_max'][p] = max(out['rank_max'][p], keep.sum())
    return out


def lmm_gls(D, Z, Y, points, kinships, kin_of_chrom, hsq):
    """lod [P, M] by generalised least squares on the dense covariance, at the heritabilities given ([P, kinships])."""
    n, M, H = D.shape
    Y = centred(Y)
    P, cz = Y.shape[1], Z.shape[1]
    off = np.concatenate(([0], np.cumsum(points)))
    lod = np.zeros((P, M))
    for e, K in enumerate(kinships):
        points_e = [m for c in range(len(points)) if kin_of_chrom[c] == e for m in range(off[c], off[c + 1])]
        X = D[:, points_e, :H - 1].reshape(n, -1)
        for p in range(P):
            if (Y[:, p] == 0.0).all():
                continue
            h = float(hsq[p, e])
            C = np.linalg.cholesky(h * K + (1.0 - h) * np.eye(n))
            white = np.linalg.solve(C, np.hstack([Z, Y[:, p:p + 1], X]))
            Zw, yw, Xw = white[:, :cz], white[:, cz], white[:, cz + 1:]
            r0 = yw - Zw @ np.linalg.lstsq(Zw, yw, rcond=1e-10)[0]
            rss0 = r0 @ r0
            for k, m in enumerate(points_e):
                A = np.hstack([Zw, Xw[:, k * (H - 1):(k + 1) * (H - 1)]])
                r1 = yw - A @ np.linalg.lstsq(A, yw, rcond=1e-10)[0]
                lod[p, m] = base.lod_of(n, rss0, r1 @ r1)
    return lod


@functools.lru_cache(maxsize=None)
def decompositions(case):
    return [decompose(K) for K in build(case)[3]]


@functools.lru_cache(maxsize=None)
def expected(case):
    """(lmm_rule's dict, lmm_gls' lod at the rule's heritabilities) of a case, computed once."""
    D, Z, Y, kinships, kin_of_chrom, _ = build(case)
    points = case[4]
    rule = lmm_rule(D, Z, Y, points, decompositions(case), kin_of_chrom)
    gls = lmm_gls(D, Z, Y, points, kinships, kin_of_chrom, rule['hsq'])
    for a in list(rule.values()) + [gls]:
        a.setflags(write=False)
    return rule, gls


def hsq_by_chrom(hsq, kin_of_chrom):
    return np.asarray(hsq)[:, list(kin_of_chrom)]


def decided(rule):
    """Mask [P, n_eig] of the pairs whose device heritability is judged: all interior ones, and the boundary ones whose
    endpoint wins by more than ENDPOINT_MARGIN."""
    boundary = (rule['hsq'] == 0.0) | (rule['hsq'] == 1.0)
    with np.errstate(invalid='ignore'):
        return ~boundary | (rule['margin'] > ENDPOINT_MARGIN) | np.isnan(rule['margin'])


def measure_hsq(cases=None, seed=7):
    """The largest change of lmm_rule's heritability under the three perturbations, over the cases."""
    worst = 0.0
    for case in (CASES if cases is None else cases):
        D, Z, Y, _, kin_of_chrom, _ = build(case)
        want = expected(case)[0]['hsq']
        for k, what in enumerate(('y', 'Z', 'lambda')):
            got = lmm_rule(D, Z, Y, case[4], decompositions(case), kin_of_chrom,
                           perturb=(what, np.random.default_rng(seed + k)))['hsq']
            worst = max(worst, float(np.abs(got - want).max()))
    return worst


deviation = base.deviation
