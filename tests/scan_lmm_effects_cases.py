"""Targets and the two host computations of the founder effects under the mixed model (gbrs_scan_lmm_effects,
GenomeScan.effects_lmm): plain numpy, no GPU.  The cohorts are those of tests/scan_lmm_cases.py, unchanged,
so its special grid points come along.

effects_lmm_rule restates the rule on scan_lmm_cases' pieces - the rotation, the weights, gram_schmidt, the Gram matrix,
scan_cases.factor, R = L_S^-1 G[S, :], its closing column, C = R R', the effects, sigma2, se, the LOD - and nothing else.
effects_lmm_gls knows nothing of rotation, W or the Gram route: the dense V = h K + (1 - h) I, its Cholesky factor,
[Z | y | D_m] whitened with all H founder columns, residuals on the whitened Z by np.linalg.lstsq(rcond=1e-10), the last
column replaced by minus the sum of the others, an SVD whose singular values above SVD_KEEP |D_m|_2 (D_m whitened: the
share does not depend on the kinship's scale) make the pseudo-inverse.  Neither is the code under test; the worst
difference between them, both at the rule's heritabilities, is the floor from which the device tolerance is taken."""
import functools

import numpy as np

import scan_cases as base
import scan_effects_cases as plain
import scan_lmm_cases as lmm

SVD_KEEP = plain.SVD_KEEP
SVD_UNDECIDED = plain.SVD_UNDECIDED
KEYS = plain.KEYS                          # ('effect', 'se', 'lod', 'sigma2')
DEVICE_FACTOR = base.DEVICE_FACTOR
CPU_HEADROOM = base.CPU_HEADROOM
CASES = lmm.CASES + lmm.LARGE_CASES
CHUNK = (8, 10, 2, 2, (6, 7, 9), 'loco')   # the smallest cohort: its target list is filled up to 513, one past the chunk
CHUNK_T = 513
DRAWN = 5
case_id = lmm.case_id

# Worst deviation (see scan_effects_cases.deviation) between effects_lmm_rule and effects_lmm_gls over a case's own targets,
# per output, both at the restatement's heritabilities, measured on the CPU (test_scan_lmm_effects_cpu.py prints it).
# These are the measured numbers themselves, not bounds on them.  §27's scheme: over the cases with more than one residual
# degree of freedom the worst per output is MEASURED_FLOOR, and a case whose own figure is above it - n = cz + H leaves
# one degree, and sigma2, se and the LOD lose the digits that rss0 - |a|^2 loses - carries its own instead.  The LOD and
# the se of the `exact` target are in neither: its rss1 is rounding by construction.
MEASURED_LMM_EFFECTS = {                   # (effect, se, lod, sigma2)
    'H8-n33-c2-P63-M22-loco': (7.76e-15, 4.96e-15, 6.79e-15, 2.52e-15),
    'H8-n70-c2-P65-M28-loco': (1.18e-14, 4.55e-15, 9.81e-15, 3.68e-15),
    'H4-n31-c1-P1-M38-loco': (6.42e-15, 1.98e-15, 3.57e-15, 1.02e-15),
    'H2-n32-c1-P5-M92-loco': (1.78e-15, 3.33e-16, 6.77e-15, 1.57e-15),
    'H9-n65-c4-P7-M31-loco': (7.27e-15, 3.05e-15, 6.25e-15, 1.2e-15),
    'H17-n64-c2-P3-M22-loco': (6.31e-15, 2.69e-15, 2.13e-15, 1.01e-15),
    'H8-n130-c3-P9-M63-loco': (6.02e-15, 1.78e-15, 6.11e-15, 9.13e-16),
    'H8-n70-c16-P4-M28-loco': (1.98e-14, 3.95e-15, 8.47e-15, 2.01e-15),
    'H8-n40-c2-P4-M17-loco': (3.56e-15, 1.81e-15, 3.8e-15, 9.38e-16),
    'H8-n10-c2-P2-M22-loco': (2.74e-13, 3.35e-12, 5.76e-12, 1.49e-12),      # n = cz + H: one residual degree of freedom
    'H8-n33-c2-P4-M22-overall': (6.31e-15, 2.21e-15, 4.17e-15, 1.36e-15),
    'H8-n33-c2-P4-M22-given': (6.42e-15, 2.42e-15, 3.91e-15, 2.09e-15),
    'H8-n70-c2-P24-M28-scaled': (1.06e-14, 2.44e-15, 1.04e-14, 8.56e-16),
    'H8-n257-c2-P2-M75-loco': (8.22e-15, 1.22e-15, 2.45e-14, 8.25e-16),
    'H17-n400-c2-P2-M60-loco': (1.14e-14, 2.89e-15, 1.65e-14, 6.2e-16),
}
MEASURED_FLOOR = {'effect': 1.98e-14, 'se': 4.96e-15, 'lod': 2.45e-14, 'sigma2': 3.68e-15}


def measured_floor(case, key):
    return max(MEASURED_FLOOR[key], MEASURED_LMM_EFFECTS[case_id(case)][KEYS.index(key)])


def cpu_bound(case, key):
    return CPU_HEADROOM * measured_floor(case, key)


def device_tol(case, key):
    return DEVICE_FACTOR * measured_floor(case, key)


def chrom_of(points, m):
    return int(np.searchsorted(np.cumsum(points), m, side='right'))


@functools.lru_cache(maxsize=None)
def build(case):
    """(pheno [n, P + 1], columns [T], points [T], planted) of a case, on scan_lmm_cases.build's cohort.  pheno holds the
    cohort's P phenotypes and the `exact` column, 3 x founder 0's dosage at HOME + 1.5 x the last covariate: it lies in the
    span of covariates + founders at HOME, so its rss1 there is rounding under any weights.  HOME is the first point of the
    last chromosome (an ordinary point: `zero` and `equal` follow it).  planted[name] is the index of
      zero, equal     targets at the cohort's special points (`equal` only with H >= 3), phenotype 0
      exact           the exact column at HOME
      alone           phenotype P - 1 at point 0, the target the bit equalities single out
    then the first and the last point of every chromosome, every (phenotype, chromosome) peak of scan_lmm_cases' restatement,
    DRAWN drawn (phenotype, point) pairs, and for CHUNK drawn pairs up to CHUNK_T targets."""
    H, n, cz, P, points, mode = case
    D, Z, Y, _, _, special = lmm.build(case)
    M = sum(points)
    home = M - points[-1]
    pheno = np.empty((n, P + 1))
    pheno[:, :P] = Y
    pheno[:, P] = 3.0 * D[:, home, 0] + 1.5 * Z[:, cz - 1]
    rng = np.random.default_rng(34 + 1000 * H + 10 * n + cz)
    pairs = [(0, special['zero'])]
    planted = {'zero': 0}
    if 'equal' in special:
        planted['equal'] = len(pairs)
        pairs.append((0, special['equal']))
    planted['exact'] = len(pairs)
    pairs.append((P, home))
    planted['alone'] = len(pairs)
    pairs.append((P - 1, 0))
    off = np.concatenate(([0], np.cumsum(points)))
    for c in range(len(points)):
        pairs.append((c % P, int(off[c])))
        pairs.append(((c + 1) % P, int(off[c + 1]) - 1))
    lod = lmm.expected(case)[0]['lod']
    for p in range(P):
        for c in range(len(points)):
            pairs.append((p, int(off[c]) + int(np.argmax(lod[p, off[c]:off[c + 1]]))))
    more = DRAWN + (max(0, CHUNK_T - len(pairs) - DRAWN) if case == CHUNK else 0)
    pairs += [(int(rng.integers(0, P)), int(rng.integers(0, M))) for _ in range(more)]
    columns = np.array([p for p, _ in pairs], dtype=np.int64)
    at = np.array([m for _, m in pairs], dtype=np.int64)
    for a in (pheno, columns, at):
        a.setflags(write=False)
    return pheno, columns, at, planted


def rule_hsq(case):
    """[P + 1, n_eig]: scan_lmm_cases' fitted heritabilities and, for the exact column, the same search's."""
    D, Z, _, _, _, _ = lmm.build(case)
    pheno = build(case)[0]
    eigs = lmm.decompositions(case)
    y = lmm.centred(pheno[:, -1:])[:, 0]
    last = [lmm.search(U.T @ y, U.T @ Z, lam)[0] for U, lam in eigs]
    return np.vstack([lmm.expected(case)[0]['hsq'], last])


def effects_lmm_rule(D, Z, pheno, points, eigs, eig_of_chrom, columns, at, hsq):
    """effect [T, H], se [T, H], lod [T], sigma2 [T], rank [T] by the rule, at the heritabilities hsq [P, n_eig]."""
    n, M, H = D.shape
    Y = lmm.centred(pheno)
    cz, T = Z.shape[1], len(columns)
    effect, se, lod, sigma2, rank = np.zeros((T, H)), np.zeros((T, H)), np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
    fits, rows = {}, {}
    for t in range(T):
        p, m = int(columns[t]), int(at[t])
        e = int(eig_of_chrom[chrom_of(points, m)])
        U, lam = eigs[e]
        if (p, e) not in fits:
            Zs, ys = U.T @ Z, U.T @ Y[:, p]
            flat = lmm.reml(0.0, ys, Zs, lam)[1] <= 0.0
            h = 0.0 if flat else float(hsq[p, e])
            sw = np.sqrt(1.0 / (h * lam + (1.0 - h)))
            Q = lmm.gram_schmidt(sw[:, None] * Zs)
            yh = sw * ys
            yt = yh - Q @ (Q.T @ yh)
            fits[p, e] = (sw, Q, yt, 0.0 if flat else np.float64(yt @ yt))
        sw, Q, yt, rss0 = fits[p, e]
        if (p, e, m) not in rows:
            X = sw[:, None] * (U.T @ D[:, m, :H - 1])
            Xt = X - Q @ (Q.T @ X)
            G = Xt.T @ Xt
            L, keep, _ = base.factor(G, (X * X).sum(axis=0))
            S = np.flatnonzero(keep)
            R = np.zeros((len(S), H))
            for k, i in enumerate(S):
                R[k, :H - 1] = (G[i] - L[i, S[:k]] @ R[:k, :H - 1]) / L[i, i]
            tail = np.zeros(len(S))
            for j in range(H - 1):
                tail = tail + R[:, j]
            R[:, H - 1] = -tail
            rows[p, e, m] = (Xt, L, S, R, np.linalg.cholesky(R @ R.T) if len(S) else np.zeros((0, 0)))
        Xt, L, S, R, Lc = rows[p, e, m]
        b = Xt.T @ yt
        a = np.zeros(len(S))
        for k, i in enumerate(S):
            a[k] = (b[i] - L[i, S[:k]] @ a[:k]) / L[i, i]
        ess = np.float64((a * a).sum())
        r = len(S)
        rss1 = max(rss0 - ess, 0.0)
        sigma2[t] = rss1 / (n - cz - r)
        lod[t] = base.lod_of(n, rss0, rss0 - ess)
        rank[t] = r
        if r:
            solve = lambda v: np.linalg.solve(Lc.T, np.linalg.solve(Lc, v))
            effect[t] = R.T @ solve(a)
            V = solve(R)
            se[t] = np.sqrt(sigma2[t]) * np.sqrt((V * V).sum(axis=0))
    return effect, se, lod, sigma2, rank


def effects_lmm_gls(D, Z, pheno, points, kinships, kin_of_chrom, columns, at, hsq):
    """effect, se, lod, sigma2, rank as effects_lmm_rule gives them, and the singular values of every target's whitened
    design as shares of its whitened |D_m|_2 [T, H], by generalised least squares on the dense covariance."""
    n, M, H = D.shape
    Y = lmm.centred(pheno)
    cz, T = Z.shape[1], len(columns)
    effect, se, lod, sigma2, rank = np.zeros((T, H)), np.zeros((T, H)), np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
    shares = np.zeros((T, H))
    roots = {}
    for t in range(T):
        p, m = int(columns[t]), int(at[t])
        e = int(kin_of_chrom[chrom_of(points, m)])
        flat = bool((Y[:, p] == 0.0).all())
        h = 0.0 if flat else float(hsq[p, e])
        if (e, h) not in roots:
            roots[e, h] = np.linalg.cholesky(h * kinships[e] + (1.0 - h) * np.eye(n))
        white = np.linalg.solve(roots[e, h], np.hstack([Z, Y[:, p:p + 1], D[:, m, :]]))
        Zw, A = white[:, :cz], white[:, cz:]
        res = A - Zw @ np.linalg.lstsq(Zw, A, rcond=1e-10)[0]
        yt, X = res[:, 0], res[:, 1:].copy()
        X[:, H - 1] = -X[:, :H - 1].sum(axis=1)
        Us, s, Vt = np.linalg.svd(X, full_matrices=False)
        scale = np.linalg.norm(white[:, cz + 1:], 2)
        shares[t, :len(s)] = s / scale
        on = s > SVD_KEEP * scale
        pinv = (Vt[on].T / s[on]) @ Us[:, on].T
        effect[t] = pinv @ yt
        rank[t] = on.sum()
        r1 = yt - X @ effect[t]
        rss0, rss1 = np.float64(yt @ yt), np.float64(r1 @ r1)
        sigma2[t] = rss1 / (n - cz - rank[t])
        se[t] = np.sqrt(sigma2[t] * (pinv * pinv).sum(axis=1))
        lod[t] = base.lod_of(n, rss0, rss1)
    return effect, se, lod, sigma2, rank, shares


def both_routes(case, hsq):
    """({key: array} by the rule, {key: array} by GLS, the singular value shares) of a case's targets at the heritabilities
    hsq [P + 1, n_eig]: the distinct (column, point) pairs go through the two routes, the targets take their pair's rows."""
    D, Z, _, kinships, kin_of_chrom, _ = lmm.build(case)
    pheno, columns, at, _ = build(case)
    pairs, where = np.unique(np.stack([columns, at], axis=1), axis=0, return_inverse=True)
    where = where.reshape(-1)
    rule = effects_lmm_rule(D, Z, pheno, case[4], lmm.decompositions(case), kin_of_chrom, pairs[:, 0], pairs[:, 1], hsq)
    gls = effects_lmm_gls(D, Z, pheno, case[4], kinships, kin_of_chrom, pairs[:, 0], pairs[:, 1], hsq)
    names = KEYS + ('rank',)
    out = ({k: a[where] for k, a in zip(names, rule)}, {k: a[where] for k, a in zip(names, gls[:5])}, gls[5][where])
    for a in list(out[0].values()) + list(out[1].values()) + [out[2]]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(case):
    """both_routes at the restatement's own heritabilities, computed once."""
    return both_routes(case, rule_hsq(case))


deviation = plain.deviation
EXACT_SHARE = plain.EXACT_SHARE
exact_lod_bound = plain.exact_lod_bound


def whitened_size(case):
    """An upper bound of the `exact` column's rss0 on the whitened scale under any heritability: |y|^2 of the centred column
    over the smallest eigenvalue V = h K + (1 - h) I can have, min(1, the kinships' smallest eigenvalue).  The target's
    sigma2 = rss1 / (n - cz - r) must stay below EXACT_SHARE of it, as §31's stays below that share of |y|^2."""
    y = lmm.centred(build(case)[0][:, -1:])
    floor = min([1.0] + [float(lam.min()) for _, lam in lmm.decompositions(case)])
    return float((y * y).sum()) / floor


def judged(case, key):
    """The targets whose `key` is compared: all, but for the LOD and se not the `exact` target, whose rss1 is rounding."""
    _, columns, _, planted = build(case)
    on = np.ones(len(columns), dtype=bool)
    if key in ('lod', 'se'):
        on[planted['exact']] = False
    return on


def measure(cases=None):
    """{case id: (effect, se, lod, sigma2)}: what MEASURED_LMM_EFFECTS holds."""
    out = {}
    for case in (CASES if cases is None else cases):
        rule, gls, _ = expected(case)
        out[case_id(case)] = tuple(deviation(rule[k][judged(case, k)], gls[k][judged(case, k)]) for k in KEYS)
    return out
