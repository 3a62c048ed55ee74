"""Targets and the host computations of the founder effects and the LOD support intervals (gbrs_scan_effects,
gbrs_scan_run_support, GenomeScan.effects, GenomeScan.run(lod_drop=...)): plain numpy, no GPU.  The cohorts
are those of tests/scan_cases.py, so its special grid points come along.

effects_rule restates the rule - the projections, W_m by scan_cases.factor, R, C = R R', its Cholesky factor, the effects,
sigma2, se, the LOD - and nothing else.  effects_svd knows nothing of W: residuals of [y | D_m] on Z by np.linalg.lstsq, the
last founder's column replaced by minus the sum of the others, an SVD whose singular values above 1e-5 |D_m|_2 make the
pseudo-inverse.  Neither is the code under test; the worst difference between them is the floor from which the device
tolerance is taken.  support_rule restates the interval rule on LOD rows; it needs no tolerance."""
import functools

import numpy as np

import scan_cases as base

SVD_KEEP = 1e-5                            # effects_svd keeps the singular values above this share of |D_m|_2
SVD_UNDECIDED = (1e-9, 1e-3)               # no singular value of a fixture may lie in this band: the rank is then beyond doubt
KEYS = ('effect', 'se', 'lod', 'sigma2')

# Worst deviation (see `deviation`) between effects_rule and effects_svd over a case's own targets, per output, measured on
# the CPU (test_scan_effects_cpu.py prints it).  These are the measured numbers themselves, not bounds on them.  Over the
# cases with more than one residual degree of freedom the worst per output is MEASURED_FLOOR; the cases with n = c + H leave
# one degree - rss1 is what is left of rss0 after |a|^2 took nearly all of it, and sigma2, se and the LOD lose those digits in
# either route - so an output of theirs whose own figure is above MEASURED_FLOOR carries it instead, as
# scan_cases.MEASURED_SATURATED does.  The LOD of the `exact` target is in neither: its rss1 is rounding by construction.
MEASURED_EFFECTS = {                       # (effect, se, lod, sigma2)
    'H2-n3-c1-T1': (2.01e-16, 1.11e-16, 0, 0),
    'H2-n33-c1-T9': (2.96e-16, 2.36e-16, 1.59e-15, 4.16e-16),
    'H3-n32-c2-T9': (9.48e-16, 6.66e-16, 8.05e-16, 1.67e-16),
    'H8-n70-c4-T65': (3e-15, 1.74e-15, 6.55e-15, 7.84e-16),
    'H8-n9-c1-T513': (8.79e-13, 4.23e-11, 5.96e-11, 1.48e-12),
    'H9-n33-c1-T9': (1.55e-15, 1.1e-15, 1.24e-15, 1.11e-16),
    'H10-n70-c4-T9': (1.97e-15, 1.19e-15, 2.5e-15, 2.12e-16),
    'H17-n31-c2-T9': (2.13e-15, 2.96e-15, 1.66e-15, 1.22e-15),
    'H10-n12-c2-T9': (7.29e-15, 5.38e-15, 3.62e-15, 3.61e-15),
    'H8-n257-c2-T9': (2.55e-15, 5.55e-16, 1.23e-14, 3.19e-16),
    'H8-n72-c64-T9': (1.47e-14, 3.75e-12, 2.87e-12, 1.75e-14),
}
MEASURED_FLOOR = {'effect': 3e-15, 'se': 2.96e-15, 'lod': 1.23e-14, 'sigma2': 1.22e-15}
DEVICE_FACTOR = base.DEVICE_FACTOR         # the device adds the samples in another, fixed order
CPU_HEADROOM = base.CPU_HEADROOM           # between the two host routes, for another LAPACK build's rounding

# (H, n, c, T).  Between them: H 2, 3, 8, 9, 10, 17 (both row paddings, their edges, the founder limit), n = c + H (the
# minimum: one residual degree; at H 2, 8 and 10), 31, 32, 33, 70 (both sides of the K chunk) and 257 (past one wavefront
# stride of 256), c 1, 2, 4 and once 64, T 1, 9, 65 and 513 (one past the target chunk).  H = 17 stands at n = 31: at
# n = c + H its design has a singular value of 9e-4 |D_m|_2, inside SVD_UNDECIDED.
CASES = [
    (2, 3, 1, 1),
    (2, 33, 1, 9),
    (3, 32, 2, 9),
    (8, 70, 4, 65),
    (8, 9, 1, 513),
    (9, 33, 1, 9),
    (10, 70, 4, 9),
    (17, 31, 2, 9),
    (10, 12, 2, 9),
    (8, 257, 2, 9),
    (8, 72, 64, 9),
]
TILE = (8, 70, 4, 65)                      # the case the bit equalities are asserted on
CHUNK = (8, 9, 1, 513)                     # the case that crosses the 512-target chunk boundary
COLUMNS = 16                               # phenotype columns of the cohort's case; the planted ones follow them
HOME = 2                                   # an ordinary point of the second chromosome


def case_id(case):
    H, n, c, T = case
    return f'H{H}-n{n}-c{c}-T{T}'


def measured_floor(case, key):
    return max(MEASURED_FLOOR[key], MEASURED_EFFECTS[case_id(case)][KEYS.index(key)])


def cpu_bound(case, key):
    return CPU_HEADROOM * measured_floor(case, key)


def device_tol(case, key):
    return DEVICE_FACTOR * measured_floor(case, key)


def run_tol(case):
    """What the pass's LOD may differ by from run()'s at the same (column, point): the scan's own device tolerance for the
    cohort.  scan_cases keeps the figure of a cohort with one residual degree of freedom per case, and the cohorts here
    (COLUMNS phenotypes) are not in its table, so for those the same figure measured on this cohort's own LODs - the
    rule against the independent route - stands in; everywhere else the scan's is the larger."""
    return max(base.device_tol(cohort_case(case)), device_tol(case, 'lod'))


def cohort_case(case):
    H, n, c, T = case
    return (H, n, c, COLUMNS, base.POINTS)


@functools.lru_cache(maxsize=None)
def build(case):
    """(D, Z, pheno [n, P], columns [T], points [T], planted) of a case.  pheno holds the cohort's COLUMNS phenotypes, then a
    constant column (2.5 in every sample) and the `exact` column, 3 x founder 0's dosage at HOME + 1.5 x the last covariate:
    it lies in the span of covariates + founders at HOME, so its rss1 there is rounding.  Target 0 is phenotype 0 at HOME.
    With T >= 9, planted[name] is the index of
      zero, equal, last, twin   targets at the cohort's special points (`equal` needs H >= 3: the `zero` point again without)
      shared                    another phenotype at HOME: two targets on one point
      twice                     target 0 again, column and point
      constant                  the constant column at an ordinary point
      exact                     the exact column at HOME
    and the targets from 9 on are phenotype t % COLUMNS at a random point."""
    H, n, c, T = case
    D, Z, Y, special = base.build(cohort_case(case))
    rng = np.random.default_rng(31 + 1000 * H + 10 * n + c + 100000 * T)
    pheno = np.empty((n, COLUMNS + 2))
    pheno[:, :COLUMNS] = Y
    pheno[:, COLUMNS] = 2.5
    pheno[:, COLUMNS + 1] = 3.0 * D[:, HOME, 0] + 1.5 * Z[:, c - 1]
    columns = np.arange(T, dtype=np.int64) % COLUMNS
    points = rng.integers(0, D.shape[1], size=T).astype(np.int64)
    points[0] = HOME
    planted = {}
    if T >= 9:
        planted = dict(zero=1, equal=2, last=3, twin=4, shared=5, twice=6, constant=7, exact=8)
        points[1], points[2], points[3] = special['zero'], special.get('equal', special['zero']), special['last']
        points[4], columns[4] = special['twin'], 0
        points[5], columns[5] = HOME, 4
        points[6], columns[6] = points[0], columns[0]
        points[7], columns[7] = 5, COLUMNS
        points[8], columns[8] = HOME, COLUMNS + 1
    for a in (pheno, columns, points):
        a.setflags(write=False)
    return D, Z, pheno, columns, points, planted


def zeroed(y):
    """The Python layer's step: a column whose values are all equal goes to the device as zeros."""
    y = np.array(y, dtype=np.float64)
    y[:, (y == y[0]).all(axis=0)] = 0.0
    return y


def effects_rule(D, Z, pheno, columns, points):
    """effect [T, H], se [T, H], lod [T], sigma2 [T], rank [T] by the rule."""
    n, M, H = D.shape
    c = Z.shape[1]
    Qz = np.linalg.qr(Z)[0]
    project = lambda v: v - Qz @ (Qz.T @ v)
    y0 = zeroed(pheno)
    T = len(columns)
    effect, se, lod, sigma2, rank = np.zeros((T, H)), np.zeros((T, H)), np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
    rows = {}
    for t in range(T):
        m = int(points[t])
        if m not in rows:
            X = D[:, m, :H - 1]
            Xt = np.stack([project(X[:, j]) for j in range(H - 1)], axis=1)
            L, keep, _ = base.factor(Xt.T @ Xt, (X * X).sum(axis=0))
            W = np.zeros((H - 1, n))
            for j in np.flatnonzero(keep):
                W[j] = (Xt[:, j] - L[j, :j] @ W[:j]) / L[j, j]
            last = np.zeros(n)
            for j in range(H - 1):
                last = last + Xt[:, j]
            full = np.column_stack([Xt, -last])
            S = np.flatnonzero(keep)
            R = np.array([[W[i] @ full[:, h] for h in range(H - 1)] for i in S]).reshape(len(S), H - 1)
            tail = np.zeros(len(S))
            for j in range(H - 1):
                tail = tail + R[:, j]
            R = np.column_stack([R, -tail])
            rows[m] = (W[S], R, np.linalg.cholesky(R @ R.T) if len(S) else np.zeros((0, 0)))
        WS, R, Lc = rows[m]
        r = len(WS)
        yt = project(y0[:, int(columns[t])])
        rss0 = np.float64(yt @ yt)
        a = WS @ yt
        ess = np.float64((a * a).sum())
        rss1 = max(rss0 - ess, 0.0)
        sigma2[t] = rss1 / (n - c - r)
        lod[t] = base.lod_of(n, rss0, rss0 - ess)
        rank[t] = r
        if r:
            solve = lambda b: np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
            effect[t] = R.T @ solve(a)
            U = solve(R)
            se[t] = np.sqrt(sigma2[t]) * np.sqrt((U * U).sum(axis=0))
    return effect, se, lod, sigma2, rank


def effects_svd(D, Z, pheno, columns, points):
    """effect, se, lod, sigma2, rank as effects_rule gives them, and the singular values of every target's design as shares of
    |D_m|_2 [T, H], by np.linalg.lstsq and an SVD."""
    n, M, H = D.shape
    c = Z.shape[1]
    y0 = zeroed(pheno)
    T = len(columns)
    effect, se, lod, sigma2, rank = np.zeros((T, H)), np.zeros((T, H)), np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
    shares = np.zeros((T, H))
    for t in range(T):
        Dm = D[:, int(points[t]), :]
        A = np.column_stack([y0[:, int(columns[t])], Dm])
        res = A - Z @ np.linalg.lstsq(Z, A, rcond=None)[0]
        yt, X = res[:, 0], res[:, 1:].copy()
        X[:, H - 1] = -X[:, :H - 1].sum(axis=1)
        U, s, Vt = np.linalg.svd(X, full_matrices=False)
        scale = np.linalg.norm(Dm, 2)
        shares[t, :len(s)] = s / scale
        on = s > SVD_KEEP * scale
        pinv = (Vt[on].T / s[on]) @ U[:, on].T
        effect[t] = pinv @ yt
        rank[t] = on.sum()
        r1 = yt - X @ effect[t]
        rss0, rss1 = np.float64(yt @ yt), np.float64(r1 @ r1)
        sigma2[t] = rss1 / (n - c - rank[t])
        se[t] = np.sqrt(sigma2[t] * (pinv * pinv).sum(axis=1))
        lod[t] = base.lod_of(n, rss0, rss1)
    return effect, se, lod, sigma2, rank, shares


@functools.lru_cache(maxsize=None)
def expected(case):
    """({key: array} by the rule, {key: array} by the SVD, the singular value shares) of a case, computed once: the distinct
    (column, point) pairs go through the two routes and the targets take their pair's rows."""
    D, Z, pheno, columns, points, _ = build(case)
    pairs, where = np.unique(np.stack([columns, points], axis=1), axis=0, return_inverse=True)
    where = where.reshape(-1)
    rule = effects_rule(D, Z, pheno, pairs[:, 0], pairs[:, 1])
    svd = effects_svd(D, Z, pheno, pairs[:, 0], pairs[:, 1])
    names = KEYS + ('rank',)
    out = ({k: a[where] for k, a in zip(names, rule)}, {k: a[where] for k, a in zip(names, svd[:5])}, svd[5][where])
    for a in list(out[0].values()) + list(out[1].values()) + [out[2]]:
        a.setflags(write=False)
    return out


def deviation(got, want):
    """Worst over the targets of |got - want| / max(1, max_h |want|); infinities must coincide."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any()
    fin = np.isfinite(want)
    size = np.maximum(1.0, np.max(np.where(fin, np.abs(want), 0.0).reshape(len(want), -1), axis=1, initial=0.0))
    diff = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0).reshape(len(want), -1)
    return float(np.max(diff.max(axis=1, initial=0.0) / size, initial=0.0))


def judged(case, key):
    """The targets whose `key` is compared: all, but for the LOD and se not the `exact` target, whose rss1 is rounding: its
    LOD is +inf or what the rounding left, and its se the square root of that."""
    T = case[3]
    on = np.ones(T, dtype=bool)
    if key in ('lod', 'se') and T >= 9:
        on[8] = False
    return on


EXACT_SHARE = 1e-10                        # what rounding may leave of the `exact` target's rss0, with room to spare


def exact_lod_bound(n):
    """The LOD an `exact` target must reach if it is finite.  Its rss1 = rss0 - |a|^2 is the rounding of two sums of n
    products and of projections on c columns, a few (n + c) eps of rss0 - under 1e-13 rss0 for every fixture - so it stays
    below EXACT_SHARE rss0 and the LOD above (n / 2) x 10."""
    return 5.0 * n


# ---- support intervals -------------------------------------------------------------------------------------------------------

def support_rule(lod, points, drop):
    """(peak_index, support_lo, support_hi) [P, n_chrom] of LOD rows [P, M] by the rule: the peak is the first of the largest
    of a chromosome; lo the largest index below it with lod <= peak - drop, the first point without one; hi the smallest
    index above it, the last point without one; -1 for a chromosome without points."""
    lod = np.atleast_2d(np.asarray(lod, dtype=np.float64))
    off = np.concatenate(([0], np.cumsum(points))).astype(np.int64)
    P, nc = len(lod), len(points)
    peak, lo, hi = (np.full((P, nc), -1, dtype=np.int64) for _ in range(3))
    for p in range(P):
        for c in range(nc):
            first, end = int(off[c]), int(off[c + 1])
            if end == first:
                continue
            k = first + int(np.argmax(lod[p, first:end]))
            bound = lod[p, k] - drop
            lo[p, c], hi[p, c] = first, end - 1
            for i in range(k - 1, first - 1, -1):
                if lod[p, i] <= bound:
                    lo[p, c] = i
                    break
            for i in range(k + 1, end):
                if lod[p, i] <= bound:
                    hi[p, c] = i
                    break
            peak[p, c] = k
    return peak, lo, hi


PLATEAU_POINTS = (75,)
PLATEAU_DROP = 1.5


@functools.lru_cache(maxsize=None)
def plateau(side):
    """(D [40, 75, 4], Z, Y [40, 1]) whose LOD profile stays within the drop for 72 points next to the peak.  The phenotype
    follows founder 0 of the dosages A, which one end point of the chromosome holds (side 'lo': the last point, so the
    interval's lower end is far away; 'hi': the first).  The 72 points next to it hold A with its founders 2 and 3 merged:
    their model is a subspace of the peak's, so their LOD - the same at all of them - is lower, and by little, since the
    phenotype does not tell founders 2 and 3 apart.  The two points at the other end are unrelated.  With PLATEAU_DROP the
    LOD has fallen only there: the interval ends 73 points from the peak - more than one 64-point step of the walk - and one
    point short of the chromosome's end, which a walk that gave up would report."""
    rng = np.random.default_rng(3175)
    n, M, H = 40, 75, 4
    A = rng.dirichlet(np.ones(H), size=n)
    merged = A.copy()
    merged[:, 2] = merged[:, 3] = 0.5 * (A[:, 2] + A[:, 3])
    D = np.empty((n, M, H))
    D[:, :2] = rng.dirichlet(np.ones(H), size=(n, 2))
    D[:, 2:M - 1] = merged[:, None, :]
    D[:, M - 1] = A
    Y = (6.0 * A[:, 0] + 0.25 * rng.normal(size=n))[:, None]
    if side == 'hi':
        D = np.ascontiguousarray(D[:, ::-1])
    Z = np.ones((n, 1))
    for a in (D, Z, Y):
        a.setflags(write=False)
    return D, Z, Y


PLATEAU_WANT = {'lo': (74, 1, 74), 'hi': (0, 0, 73)}      # (peak, support_lo, support_hi) of either side
