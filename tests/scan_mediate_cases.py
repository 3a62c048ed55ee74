"""Targets, mediators and the host computations of the mediation pass (gbrs_scan_mediate, GenomeScan.mediate; DESIGN.md
§30): plain numpy, no GPU.  The cohorts are those of tests/scan_cases.py, so its special grid points come along.

mediate_rule restates the rule - the projections, W_m by scan_cases.factor, the six numbers of a pair, the three guards,
the LOD - and nothing else.  mediate_lstsq knows nothing of the rule: per pair np.linalg.lstsq on [Z | z_q] and on
[Z | z_q | X_m] with rcond=1e-10; it sees the guards as lost rank and as a residual down at rounding.  Neither is the
code under test; the worst difference between them is the floor from which the device tolerance is taken."""
import functools

import numpy as np

import scan_cases as base

PIVOT = base.PIVOT                         # the three guards' threshold: the scan's own
UNDECIDED = base.UNDECIDED                 # a guard ratio in this band could flip `used` by rounding

# Worst |mediate_rule - mediate_lstsq| / max(1, |lod|) over lod0 and every used lod_med of a case, measured on the CPU
# (test_scan_mediate_cpu.py prints it).  These are the measured numbers themselves, not bounds on them.  The cases with
# n = c + H + 1 leave one residual degree of freedom once the mediator is in: rss1' is what is left of rss1 after e_yz^2 / e_zz
# took nearly all of it, and both routes lose those digits, so their figures are larger, as scan_cases.MEASURED_SATURATED's.
MEASURED_MEDIATE = {'H2-n4-c1-T1-Q1-K5': 6.77e-15, 'H3-n32-c2-T8-Q63-K1': 1.08e-13, 'H8-n70-c4-T65-Q130-K5': 1.29e-14,
                    'H8-n10-c1-T9-Q64-K0': 4.68e-11, 'H9-n33-c1-T9-Q65-K5': 4.78e-14, 'H10-n31-c2-T8-Q64-K1': 5.42e-14,
                    'H17-n22-c4-T9-Q63-K5': 1.71e-10, 'H8-n257-c2-T9-Q65-K5': 2.7e-13}
DEVICE_FACTOR = base.DEVICE_FACTOR         # the device adds the samples in another, fixed order
CPU_HEADROOM = base.CPU_HEADROOM           # between the two host routes, for another LAPACK build's rounding

# (H, n, c, T, Q, K).  Between them: H 2, 3, 8, 9, 10, 17 (both row paddings, their edges, the founder limit),
# n = c + H + 1 (the minimum), 31, 32, 33, 70 (both sides of the K chunk) and 257, c 1, 2, 4, T 1, 8, 9, 65 (one tile of
# targets at HP = 8, one past it, many), Q 1, 63, 64, 65, 130 (around the mediator tile), K 0, 1, 5 and, at Q = 1, a K
# above n_used.
CASES = [
    (2, 4, 1, 1, 1, 5),
    (3, 32, 2, 8, 63, 1),
    (8, 70, 4, 65, 130, 5),
    (8, 10, 1, 9, 64, 0),
    (9, 33, 1, 9, 65, 5),
    (10, 31, 2, 8, 64, 1),
    (17, 22, 4, 9, 63, 5),
    (8, 257, 2, 9, 65, 5),
]
TILE = (8, 70, 4, 65, 130, 5)              # the case the bit equalities are asserted on


def case_id(case):
    H, n, c, T, Q, K = case
    return f'H{H}-n{n}-c{c}-T{T}-Q{Q}-K{K}'


def measured_floor(case):
    return MEASURED_MEDIATE[case_id(case)]


def cpu_bound(case):
    return CPU_HEADROOM * measured_floor(case)


def device_tol(case):
    return DEVICE_FACTOR * measured_floor(case)


def cohort_case(case):
    H, n, c, T, Q, K = case
    return (H, n, c, max(T, Q, 16), base.POINTS)


HOME = 2                                   # the grid point of the planted target: an ordinary point of the second chromosome


@functools.lru_cache(maxsize=None)
def build(case):
    """(D, Z, targets [n, T], points [T], mediators [n, Q], planted) of a case.  The ordinary targets and mediators are
    phenotype columns of the cohort's case, so target column k is also mediator k where both exist: the pair is unused
    by the third guard.  Planted, as far as T and Q have room (planted[name] is the index, absent without room):
      targets    0        2 x the true mediator + noise, at HOME
                 1, 2, 3  at the cohort's `zero`, `equal` (H >= 3) and `last` points, whose W has skipped columns
                 4        another phenotype at HOME: two targets on one point
                 5        target 0 again, column and point: the same target twice
      mediators  true     founder 0's dosage at HOME + noise: what target 0 follows (index min(3, Q - 1))
                 constant 2.5 in every sample: in the intercept's span
                 span     1.5 x the last covariate + a combination of the founders at HOME: unusable at HOME alone
                 same     target 0 itself
                 twin     a copy of the true mediator (the last index): a tie in the selection"""
    H, n, c, T, Q, K = case
    D, Z, Y, special = base.build(cohort_case(case))
    rng = np.random.default_rng(7 + 1000 * H + 10 * n + c + 100000 * T + Q)
    med = np.array(Y[:, :Q])
    planted = {'true': min(3, Q - 1)}
    med[:, planted['true']] = 4.0 * D[:, HOME, 0] + 0.3 * rng.normal(size=n)
    tgt = np.empty((n, T))
    pts = np.empty(T, dtype=np.int64)
    for t in range(T):
        tgt[:, t] = Y[:, t % Y.shape[1]]
        pts[t] = rng.integers(0, D.shape[1])
    tgt[:, 0] = 2.0 * med[:, planted['true']] + 0.2 * rng.normal(size=n)
    pts[0] = HOME
    if T >= 8:
        pts[1], pts[2], pts[3] = special['zero'], special.get('equal', special['zero']), special['last']
        pts[4] = HOME
        tgt[:, 5], pts[5] = tgt[:, 0], pts[0]
    if Q >= 63:
        planted.update(constant=5, span=6, same=7, twin=Q - 1)
        med[:, 5] = 2.5
        med[:, 6] = 1.5 * Z[:, c - 1] + D[:, HOME, :H - 1] @ rng.uniform(0.5, 2.0, size=H - 1)
        med[:, 7] = tgt[:, 0]
        med[:, Q - 1] = med[:, planted['true']]
    for a in (tgt, pts, med):
        a.setflags(write=False)
    return D, Z, tgt, pts, med, planted


def zeroed(y):
    """The Python layer's step: a column whose values are all equal goes to the device as zeros."""
    y = np.array(y, dtype=np.float64)
    y[:, (y == y[0]).all(axis=0)] = 0.0
    return y


def mediate_rule(D, Z, target, point, mediator):
    """lod0 [T], lod_med [T, Q] (NaN where unused), used [T, Q], ratios [T, Q, 2]: e_zz / s_zz and rss0' / s_yy (NaN where
    the denominator is 0) by the rule."""
    n, M, H = D.shape
    Qz = np.linalg.qr(Z)[0]
    # column by column, so that equal columns give equal bits wherever they stand (a matrix product need not)
    project = lambda V: np.stack([v - Qz @ (Qz.T @ v) for v in zeroed(V).T], axis=1)
    Yt, Zt = project(target), project(mediator)
    syy, szz = (Yt * Yt).sum(axis=0), (Zt * Zt).sum(axis=0)
    T, Qn = Yt.shape[1], Zt.shape[1]
    lod0, lod, used, ratios = np.empty(T), np.full((T, Qn), np.nan), np.zeros((T, Qn), dtype=bool), np.full((T, Qn, 2), np.nan)
    rows = {}
    for t in range(T):
        m = int(point[t])
        if m not in rows:
            X = D[:, m, :H - 1]
            Xt = X - Qz @ (Qz.T @ X)
            L, keep, _ = base.factor(Xt.T @ Xt, (X * X).sum(axis=0))
            W = np.zeros((H - 1, n))
            for j in np.flatnonzero(keep):
                W[j] = (Xt[:, j] - L[j, :j] @ W[:j]) / L[j, j]
            rows[m] = (W, np.stack([W @ Zt[:, q] for q in range(Qn)], axis=1))
        W, B = rows[m]
        a = W @ Yt[:, t]
        rss1 = syy[t] - (a * a).sum()
        lod0[t] = base.lod_of(n, syy[t], rss1)
        syz = np.array([Yt[:, t] @ Zt[:, q] for q in range(Qn)])
        ezz = szz - (B * B).sum(axis=0)
        eyz = syz - np.array([a @ B[:, q] for q in range(Qn)])
        with np.errstate(divide='ignore', invalid='ignore'):
            rss0p = syy[t] - syz * syz / szz
            rss1p = rss1 - eyz * eyz / ezz
            ratios[t, :, 0] = np.where(szz > 0, ezz / szz, np.nan)
            ratios[t, :, 1] = np.where((szz > 0) & (syy[t] > 0), rss0p / syy[t], np.nan)
        ok = (szz != 0.0) & ~(ezz <= PIVOT * szz)
        ok &= ~(np.where(ok, rss0p, 0.0) <= PIVOT * syy[t])
        used[t] = ok
        lod[t, ok] = base.lod_of(n, rss0p[ok], rss1p[ok])
    return lod0, lod, used, ratios


def mediate_lstsq(D, Z, target, point, mediator):
    """lod0 [T], lod_med [T, Q] (NaN where unused), used [T, Q] by np.linalg.lstsq, two fits per pair.  A pair is unused
    when the mediator adds no rank to Z, when it adds none to [Z | X_m], or when the target's residual given [Z | z_q] is
    within 1e-10 of nothing."""
    n, M, H = D.shape
    c = Z.shape[1]
    T, Qn = target.shape[1], mediator.shape[1]
    lod0, lod, used = np.empty(T), np.full((T, Qn), np.nan), np.zeros((T, Qn), dtype=bool)

    def fit(A, y):
        b, _, rank, _ = np.linalg.lstsq(A, y, rcond=1e-10)
        r = y - A @ b
        return float(r @ r), rank

    for t in range(T):
        y, X = target[:, t], D[:, int(point[t]), :H - 1]
        rss_z, _ = fit(Z, y)
        rss_zx, rank_zx = fit(np.hstack([Z, X]), y)
        lod0[t] = base.lod_of(n, rss_z, rss_zx)
        for q in range(Qn):
            z = mediator[:, q:q + 1]
            rss0p, rank0 = fit(np.hstack([Z, z]), y)
            rss1p, rank1 = fit(np.hstack([Z, z, X]), y)
            if rank0 == c + 1 and rank1 == rank_zx + 1 and rss0p > PIVOT * rss_z:
                used[t, q] = True
                lod[t, q] = base.lod_of(n, rss0p, rss1p)
    return lod0, lod, used


def select(lod, used, K):
    """(n_used [T], mean [T], sd [T], best_index [T, K], best_lod [T, K]) over the used mediators of every target: numpy's
    mean and standard deviation with n_used - 1 below, NaN below 2; the K lowest by (value, index), -1 / NaN beyond."""
    T = len(lod)
    count = used.sum(axis=1).astype(np.int64)
    mean, sd = np.full(T, np.nan), np.full(T, np.nan)
    index, best = np.full((T, K), -1, dtype=np.int64), np.full((T, K), np.nan)
    for t in range(T):
        on = np.flatnonzero(used[t])
        if len(on) >= 2:
            mean[t], sd[t] = lod[t, on].mean(), lod[t, on].std(ddof=1)
        order = on[np.lexsort((on, lod[t, on]))][:K]
        index[t, :len(order)] = order
        best[t, :len(order)] = lod[t, order]
    return count, mean, sd, index, best


@functools.lru_cache(maxsize=None)
def expected(case):
    """(rule's lod0, lod_med, used, ratios, lstsq's lod0, lod_med, used) of a case, computed once."""
    D, Z, tgt, pts, med, _ = build(case)
    out = mediate_rule(D, Z, tgt, pts, med) + mediate_lstsq(D, Z, tgt, pts, med)
    for a in out:
        a.setflags(write=False)
    return out


def deviation(got, want):
    """Worst |got - want| / max(1, |want|); NaNs and infinities must coincide."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return base.deviation(np.nan_to_num(got, nan=0.0, posinf=np.inf, neginf=-np.inf),
                          np.nan_to_num(want, nan=0.0, posinf=np.inf, neginf=-np.inf))


def undecided(ratios):
    """The guard ratios that lie in UNDECIDED."""
    with np.errstate(invalid='ignore'):
        return (ratios > UNDECIDED[0]) & (ratios < UNDECIDED[1])
