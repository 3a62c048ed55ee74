"""Cohorts and the two host computations of the scan with interactive covariates (gbrs_scan_int_*, GenomeScan.prepare_int /
run_int): plain numpy, no GPU.  The cohorts are built by tests/scan_cases.py, so its special grid points come
along; the interactive covariates are zint = Z[:, 1:1+k], whose first column is the 0/1 covariate.

int_rule restates the rule - the columns in their order, raw, the projection, the Gram matrix, scan_cases.factor, the
triangular solve, the three LODs - and nothing else.  int_lstsq knows nothing of it: np.linalg.lstsq with rcond=1e-10 on
[Z | X | X*z] for lod_full and on [Z | X] for lod_add, lod_int from those two residual sums, the ranks lstsq's minus c.
Neither is the code under test; the worst difference between them is the floor from which the device tolerance is taken."""
import functools

import numpy as np

import scan_cases as base

KEYS = ('lod_full', 'lod_add', 'lod_int')
POINTS = base.POINTS

# (H, n, c, k, P, points per chromosome).  Between them: every HPI (16: H <= 5 with k = 1 and H 2 .. 9 where 8 + k Hx <= 16;
# 32; 64), the 16, 32 and 64 rows exactly full (H9 k1, H17 k1, H17 k3), both Hp, one residual degree of freedom (H2-n5,
# H4-n9, H8-n17, H17-n69), both sides of the K chunk, n past 256, P on both sides of a 64-column tile.
CASES = [
    (2, 5, 2, 1, 1, POINTS),
    (2, 33, 2, 1, 64, POINTS),
    (4, 9, 2, 1, 64, POINTS),
    (8, 33, 2, 1, 65, POINTS),
    (8, 17, 2, 1, 1, POINTS),
    (8, 70, 4, 2, 130, (1, 65, 9)),
    (8, 32, 3, 2, 64, POINTS),
    (9, 31, 2, 1, 63, POINTS),
    (9, 40, 3, 2, 1, POINTS),
    (10, 33, 2, 1, 64, POINTS),
    (13, 64, 3, 2, 65, POINTS),
    (17, 70, 2, 1, 65, POINTS),
    (17, 120, 4, 3, 1, POINTS),
    (17, 69, 4, 3, 1, POINTS),
    (8, 257, 2, 1, 65, POINTS),
    (16, 80, 4, 3, 63, POINTS),
    (8, 72, 5, 3, 9, POINTS),
]
PLAIN = [(8, 70, 4, 2, 130, (1, 65, 9)), (17, 70, 2, 1, 65, POINTS)]      # lod_add against GenomeScan.run() with ==
SMALL = (2, 33, 2, 1, 64, POINTS)                                        # the case of the chunk boundary and the appends

# Worst deviation (scan_cases.deviation) between int_rule and int_lstsq per output (lod_full, lod_add, lod_int), measured on
# the CPU (test_scan_int_cpu.py prints it).  These are the measured numbers themselves, not bounds on them.  Over the cases
# with more than one residual degree of freedom the worst per output is MEASURED_FLOOR; the four cases with
# n = c + Hx (1 + k) + 1 leave one degree - rss_full is what is left of rss0 after ess_full took nearly all of it, and
# lod_full and lod_int lose those digits in either route - so an output of theirs whose own figure is above MEASURED_FLOOR
# carries it instead, as scan_cases.MEASURED_SATURATED does.  H8-n257 stands apart from the floor as scan_cases.LARGE_CASES do
# (the absolute rounding of (n / 2) log10 grows with n) and carries its own figures in the same way.
MEASURED_INT = {                           # (lod_full, lod_add, lod_int)
    'H2-n5-c2-k1-P1-M17': (2.51e-15, 2.24e-15, 4.58e-15),
    'H2-n33-c2-k1-P64-M17': (6.19e-15, 6.26e-15, 6.26e-15),
    'H4-n9-c2-k1-P64-M17': (6.05e-15, 6.05e-15, 3.91e-15),
    'H8-n33-c2-k1-P65-M17': (1.19e-14, 5.55e-15, 1.82e-14),
    'H8-n17-c2-k1-P1-M17': (4.78e-13, 6.32e-15, 6.54e-13),
    'H8-n70-c4-k2-P130-M75': (1.35e-14, 1.91e-14, 1.49e-14),
    'H8-n32-c3-k2-P64-M17': (3.84e-14, 5.95e-15, 4.39e-14),
    'H9-n31-c2-k1-P63-M17': (5.68e-14, 5e-15, 7.36e-14),
    'H9-n40-c3-k2-P1-M17': (4.24e-15, 1.89e-15, 5.27e-15),
    'H10-n33-c2-k1-P64-M17': (1.02e-14, 6.75e-15, 2.05e-14),
    'H13-n64-c3-k2-P65-M17': (1.53e-14, 1.15e-14, 1.73e-14),
    'H17-n70-c2-k1-P65-M17': (1.07e-14, 9.19e-15, 1.29e-14),
    'H17-n120-c4-k3-P1-M17': (4.73e-15, 2.85e-15, 5.44e-15),
    'H17-n69-c4-k3-P1-M17': (1.25e-10, 3.92e-15, 1.28e-10),
    'H8-n257-c2-k1-P65-M17': (5.41e-14, 9.83e-14, 1.46e-13),
    'H16-n80-c4-k3-P63-M17': (2.93e-14, 1.14e-14, 3.24e-14),
    'H8-n72-c5-k3-P9-M17': (6.22e-15, 1.31e-14, 7.05e-15),
}
MEASURED_FLOOR = {'lod_full': 5.68e-14, 'lod_add': 1.91e-14, 'lod_int': 7.36e-14}
DEVICE_FACTOR = base.DEVICE_FACTOR         # the device adds the samples in another, fixed order
CPU_HEADROOM = base.CPU_HEADROOM           # between the two host routes, for another LAPACK build's rounding


def case_id(case):
    H, n, c, k, P, points = case
    return f'H{H}-n{n}-c{c}-k{k}-P{P}-M{sum(points)}'


def one_degree(case):
    H, n, c, k, P, points = case
    return n == c + (H - 1) * (1 + k) + 1


def measured_floor(case, key):
    return max(MEASURED_FLOOR[key], MEASURED_INT[case_id(case)][KEYS.index(key)])


def cpu_bound(case, key):
    return CPU_HEADROOM * measured_floor(case, key)


def device_tol(case, key):
    return DEVICE_FACTOR * measured_floor(case, key)


def hpi_of(case):
    H, k = case[0], case[3]
    rows = (8 if H <= 9 else 16) + k * (H - 1)
    return 16 if rows <= 16 else 32 if rows <= 32 else 64


@functools.lru_cache(maxsize=None)
def build(case):
    """(D [n, M, H], Z [n, c], Y [n, P], zint [n, k], special points) of a case: scan_cases.build's cohort of (H, n, c, P,
    points) and the covariates after the intercept as the interactive ones."""
    H, n, c, k, P, points = case
    D, Z, Y, special = base.build((H, n, c, P, points))
    zint = np.ascontiguousarray(Z[:, 1:1 + k])
    zint.setflags(write=False)
    return D, Z, Y, zint, special


def columns(D, zint, m):
    """The design columns of grid point m in the rule's order: additive, then per interactive covariate the products."""
    X = D[:, m, :D.shape[2] - 1]
    return np.hstack([X] + [X * zint[:, q:q + 1] for q in range(zint.shape[1])])


def lod_int_of(n, rss0, rss_add, rss_full):
    with np.errstate(divide='ignore', invalid='ignore'):
        lod = 0.5 * n * np.log10(rss_add / rss_full)
    lod = np.where(rss_full <= 0.0, np.inf, lod)
    return np.where((rss0 == 0.0) | (rss_add <= 0.0), 0.0, lod)


def int_rule(D, Z, Y, zint):
    """({lod_full, lod_add, lod_int} [P, M], rank_full [M], rank_add [M], pivot ratios [M, Hx (1 + k)]) by the rule."""
    n, M, H = D.shape
    Hx, NC = H - 1, (H - 1) * (1 + zint.shape[1])
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    rss0 = (Yt * Yt).sum(axis=0)
    out = {key: np.empty((Y.shape[1], M)) for key in KEYS}
    rank_full, rank_add, ratios = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32), np.empty((M, NC))
    for m in range(M):
        X = columns(D, zint, m)
        Xt = X - Q @ (Q.T @ X)
        L, keep, ratios[m] = base.factor(Xt.T @ Xt, (X * X).sum(axis=0))
        W = np.zeros((NC, n))
        for j in np.flatnonzero(keep):
            W[j] = (Xt[:, j] - L[j, :j] @ W[:j]) / L[j, j]
        a = (W @ Yt) ** 2
        ess_add = a[:Hx].sum(axis=0)
        ess_full = ess_add + a[Hx:].sum(axis=0)
        out['lod_full'][:, m] = base.lod_of(n, rss0, rss0 - ess_full)
        out['lod_add'][:, m] = base.lod_of(n, rss0, rss0 - ess_add)
        out['lod_int'][:, m] = lod_int_of(n, rss0, rss0 - ess_add, rss0 - ess_full)
        rank_full[m], rank_add[m] = keep.sum(), keep[:Hx].sum()
    return out, rank_full, rank_add, ratios


def int_lstsq(D, Z, Y, zint):
    """({lod_full, lod_add, lod_int} [P, M], rank_full [M], rank_add [M]) by np.linalg.lstsq."""
    n, M, H = D.shape
    c = Z.shape[1]
    rss = lambda A: ((Y - A @ np.linalg.lstsq(A, Y, rcond=1e-10)[0]) ** 2).sum(axis=0)
    rss0 = rss(Z)
    out = {key: np.empty((Y.shape[1], M)) for key in KEYS}
    rank_full, rank_add = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32)
    for m in range(M):
        X = columns(D, zint, m)
        A_add, A_full = np.hstack([Z, X[:, :H - 1]]), np.hstack([Z, X])
        rss_add, rss_full = rss(A_add), rss(A_full)
        out['lod_full'][:, m] = base.lod_of(n, rss0, rss_full)
        out['lod_add'][:, m] = base.lod_of(n, rss0, rss_add)
        out['lod_int'][:, m] = lod_int_of(n, rss0, rss_add, rss_full)
        rank_full[m] = np.linalg.lstsq(A_full, Y[:, :1], rcond=1e-10)[2] - c
        rank_add[m] = np.linalg.lstsq(A_add, Y[:, :1], rcond=1e-10)[2] - c
    return out, rank_full, rank_add


@functools.lru_cache(maxsize=None)
def expected(case):
    """(int_rule's four, int_lstsq's three) of a case, computed once."""
    D, Z, Y, zint, _ = build(case)
    rule, lstsq = int_rule(D, Z, Y, zint), int_lstsq(D, Z, Y, zint)
    for a in list(rule[0].values()) + list(rule[1:]) + list(lstsq[0].values()) + list(lstsq[1:]):
        a.setflags(write=False)
    return rule, lstsq


def deviation(got, want):
    """scan_cases.deviation, except that lod_int of the lstsq route may be slightly negative where the interaction explains
    nothing (two residual sums from two solves): what is compared is the value itself."""
    return base.deviation(np.asarray(got), np.asarray(want))
