"""Cohorts, phenotypes and the two host computations of the genome scan (gbrs_scan_*, gbrs_amd/scan.py):
plain numpy, no GPU.

scan_rule restates the rule itself - projection on the covariates' basis, the Gram matrix, the Cholesky factorisation
with the skip rule, the triangular solve - and nothing else.  scan_lstsq knows nothing of the rule: np.linalg.lstsq on
[Z | X_m] with rcond=1e-10, and on Z alone for rss0.  Neither is the code under test; the worst difference between
them over every case below is the floor from which the device tolerance is taken."""
import functools

import numpy as np

PIVOT = 1e-10                              # the skip rule's threshold
UNDECIDED = (1e-13, 1e-7)                  # a pivot ratio d_j / G_jj in this band could flip a rank by rounding

# Worst |scan_rule - scan_lstsq| / max(1, |lod|), measured on the CPU (test_scan_cpu.py prints it).  Over the cases with
# more than one residual degree of freedom the worst is 1.91e-14: MEASURED_FLOOR.  The cases with n = c + H leave one
# degree: rss1 is then down to 1e-8 of rss0 (LODs up to 71 from 18 samples) and rss0 - ess cancels that many digits in
# either route, so those whose own measured figure is above MEASURED_FLOOR carry it instead (MEASURED_SATURATED; the
# sixth, H2-n3, measured 1.27e-14).  These are the measured numbers themselves, not bounds on them.
MEASURED_FLOOR = 1.91e-14
MEASURED_SATURATED = {'H3-n7-c4-P63-M17': 1.21e-10, 'H8-n9-c1-P64-M17': 2.82e-9, 'H9-n13-c4-P65-M17': 6.81e-11,
                      'H10-n11-c1-P1-M17': 4.32e-13, 'H16-n18-c2-P130-M17': 1.43e-8}
# The same figure of every case of LARGE_CASES, each its own: the absolute rounding of (n / 2) log10(rss0 / rss1) grows
# with n, and the last degree of freedom of H17-n19 and H16-n80-c64 costs what it costs above.
MEASURED_LARGE = {'H8-n256-c1-P1-M17': 1.18e-14, 'H8-n257-c2-P65-M17': 9.83e-14, 'H9-n512-c2-P130-M75': 3.93e-13,
                  'H4-n129-c2-P64-M17': 5.54e-14, 'H17-n33-c1-P63-M17': 5.46e-15, 'H17-n300-c4-P65-M17': 9.56e-14,
                  'H17-n19-c2-P1-M17': 5.5e-13, 'H8-n130-c64-P64-M17': 3.63e-14, 'H16-n80-c64-P1-M17': 1.75e-12}
# The device against each host route: ten times the measured floor - the device adds the samples in another, fixed order
# (up to 70 of them in CASES, up to 512 in LARGE_CASES) and fuses nothing.
DEVICE_FACTOR = 10
# What test_scan_cpu.py allows the two host routes between themselves: the measured floor with headroom for another
# LAPACK build's rounding.  It bounds nothing on the device.
CPU_HEADROOM = 1.3


def measured_floor(case):
    return max(MEASURED_FLOOR, MEASURED_SATURATED.get(case_id(case), 0.0), MEASURED_LARGE.get(case_id(case), 0.0))


def cpu_bound(case):
    return CPU_HEADROOM * measured_floor(case)


def device_tol(case):
    return DEVICE_FACTOR * measured_floor(case)


POINTS = (1, 7, 9)                         # three chromosomes: a one-point chromosome and two tile edges
# (H, n, c, P, points per chromosome).  Between them: H 2, 3, 4, 8, 9, 10, 16 (both row paddings and their edges),
# n = c + H (one past the minimum), 31, 32, 33, 70 (both sides of the K chunk), c 1, 2, 4, P 1, 63, 64, 65, 130, and once
# a chromosome of 65 points.
CASES = [
    (2, 3, 1, 1, POINTS),
    (2, 32, 2, 64, POINTS),
    (3, 7, 4, 63, POINTS),
    (3, 33, 1, 65, POINTS),
    (4, 31, 2, 130, POINTS),
    (8, 9, 1, 64, POINTS),
    (8, 70, 4, 130, (1, 65, 9)),
    (8, 32, 2, 1, POINTS),
    (9, 33, 1, 63, POINTS),
    (9, 13, 4, 65, POINTS),
    (10, 31, 2, 64, POINTS),
    (10, 11, 1, 1, POINTS),
    (16, 70, 4, 65, POINTS),
    (16, 18, 2, 130, POINTS),
    (16, 32, 1, 63, POINTS),
]
# Cohorts past the 256-thread stride of scan_prepare_kernel's per-sample solve, the founder limit (H = 17: Hx = HP = 16,
# no padding row) and the covariate limit (c = 64), apart from CASES so that what is measured over CASES stays as it is.
LARGE_CASES = [
    (8, 256, 1, 1, POINTS),                # the solve's stride exactly full; 8 K chunks
    (8, 257, 2, 65, POINTS),               # one sample past it; 9 chunks
    (9, 512, 2, 130, (1, 65, 9)),          # two full laps of the solve; 16 chunks; Hx = HP = 8
    (4, 129, 2, 64, POINTS),               # a third lap of the lane sums (s = lane + 128)
    (17, 33, 1, 63, POINTS),               # H = 17
    (17, 300, 4, 65, POINTS),              # the same with the second lap of the solve
    (17, 19, 2, 1, POINTS),                # H = 17 at n = c + H
    (8, 130, 64, 64, POINTS),              # c = 64
    (16, 80, 64, 1, POINTS),               # c = 64 at n = c + H
]


def case_id(case):
    H, n, c, P, points = case
    return f'H{H}-n{n}-c{c}-P{P}-M{sum(points)}'


@functools.lru_cache(maxsize=None)
def build(case):
    """(D [n, M, H], Z [n, c], Y [n, P], special points) of a case.  Rows of D are positive and add up to 1.  Special
    grid points, all on the last chromosome:
      zero   founder 0 is exactly 0.0 in every sample
      equal  founders 0 and 1 are exactly equal (H >= 3)
      last   the dropped founder H - 1 is exactly 0.0, so the kept columns add up to the intercept
      twin   a copy of the point before it: two grid points with the same LODs, for the first-index rule
    Phenotype 0 follows founder 0 at the twin's original, so its peak on that chromosome is the tie."""
    H, n, c, P, points = case
    rng = np.random.default_rng(1000 * H + 10 * n + c)
    M = sum(points)
    D = rng.dirichlet(np.ones(H), size=(n, M))
    first = M - points[-1]
    special = {'zero': first + 1, 'last': first + 3, 'twin': first + 6}
    D[:, special['zero'], 0] = 0.0
    D[:, special['zero']] /= D[:, special['zero']].sum(axis=1, keepdims=True)
    if H >= 3:
        special['equal'] = first + 2
        D[:, special['equal'], 1] = D[:, special['equal'], 0]
    D[:, special['last'], H - 1] = 0.0
    D[:, special['last']] /= D[:, special['last']].sum(axis=1, keepdims=True)
    D[:, special['twin']] = D[:, special['twin'] - 1]
    Z = np.ones((n, c))
    Z[:, 1:] = rng.normal(size=(n, c - 1))
    if c >= 2:
        Z[:, 1] = rng.integers(0, 2, size=n)                    # a 0/1 covariate, like sex
        Z[0, 1], Z[1, 1] = 0.0, 1.0
    Y = rng.normal(size=(n, P))
    Y[:, 0] = 6.0 * D[:, special['twin'] - 1, 0] + 0.25 * rng.normal(size=n)
    for p in range(1, P, 7):                                    # some phenotypes with a locus behind them
        Y[:, p] += 3.0 * D[:, rng.integers(0, M), rng.integers(0, H)]
    for a in (D, Z, Y):
        a.setflags(write=False)
    return D, Z, Y, special


def lod_of(n, rss0, rss1):
    with np.errstate(divide='ignore', invalid='ignore'):
        lod = 0.5 * n * np.log10(rss0 / rss1)
    lod = np.where(rss1 <= 0.0, np.inf, lod)
    return np.where(rss0 == 0.0, 0.0, lod)


def factor(G, raw=None):
    """The Cholesky factor of G with the skip rule: (L, kept flags, pivot ratios d_j / G_jj; NaN where G_jj <= 0).
    raw[j]: the squared norm of column j before the covariates were projected out; G_jj <= PIVOT raw[j] counts as
    G_jj = 0 (the covariates are the columns before column 0), and its ratio is reported as G_jj / raw[j]."""
    k = len(G)
    if raw is not None:
        G = G.copy()
        gone = G.diagonal() <= PIVOT * raw
        share = np.where(gone & (raw > 0), G.diagonal() / np.where(raw > 0, raw, 1.0), np.nan)
        G[gone, gone] = 0.0
    L, keep, ratio = np.zeros((k, k)), np.zeros(k, dtype=bool), np.full(k, np.nan)
    for j in range(k):
        d = G[j, j]
        for i in range(j):
            if keep[i]:
                v = G[j, i]
                for t in range(i):
                    if keep[t]:
                        v -= L[j, t] * L[i, t]
                L[j, i] = v / L[i, i]
                d -= L[j, i] * L[j, i]
        if G[j, j] > 0.0:
            ratio[j] = d / G[j, j]
        elif raw is not None:
            ratio[j] = share[j]
        if G[j, j] > 0.0 and d > PIVOT * G[j, j]:
            keep[j] = True
            L[j, j] = np.sqrt(d)
        else:
            L[j, :] = 0.0
    return L, keep, ratio


def scan_rule(D, Z, Y):
    """lod [P, M], rank [M], pivot ratios [M, H - 1] by the rule."""
    n, M, H = D.shape
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    rss0 = (Yt * Yt).sum(axis=0)
    lod, rank, ratios = np.empty((Y.shape[1], M)), np.empty(M, dtype=np.int32), np.empty((M, H - 1))
    for m in range(M):
        X = D[:, m, :H - 1]
        Xt = X - Q @ (Q.T @ X)
        L, keep, ratios[m] = factor(Xt.T @ Xt, (X * X).sum(axis=0))
        W = np.zeros((H - 1, n))
        for j in np.flatnonzero(keep):
            W[j] = (Xt[:, j] - L[j, :j] @ W[:j]) / L[j, j]
        ess = ((W @ Yt) ** 2).sum(axis=0)
        lod[:, m] = lod_of(n, rss0, rss0 - ess)
        rank[m] = keep.sum()
    return lod, rank, ratios


def scan_lstsq(D, Z, Y):
    """lod [P, M], rank [M] (of X_m beside Z) by np.linalg.lstsq."""
    n, M, H = D.shape
    c = Z.shape[1]
    b0 = np.linalg.lstsq(Z, Y, rcond=1e-10)[0]
    r0 = Y - Z @ b0
    rss0 = (r0 * r0).sum(axis=0)
    lod, rank = np.empty((Y.shape[1], M)), np.empty(M, dtype=np.int32)
    for m in range(M):
        A = np.hstack([Z, D[:, m, :H - 1]])
        b, _, rk, _ = np.linalg.lstsq(A, Y, rcond=1e-10)
        r1 = Y - A @ b
        lod[:, m] = lod_of(n, rss0, (r1 * r1).sum(axis=0))
        rank[m] = rk - c
    return lod, rank


def peaks(lod, points):
    """(peak_lod [P, n_chrom], peak_index [P, n_chrom]): the first of the largest per chromosome."""
    off = np.concatenate(([0], np.cumsum(points)))
    peak = np.stack([lod[:, a:b].max(axis=1) for a, b in zip(off[:-1], off[1:])], axis=1)
    index = np.stack([a + lod[:, a:b].argmax(axis=1) for a, b in zip(off[:-1], off[1:])], axis=1)
    return peak, index.astype(np.int64)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(rule's lod, rank, ratios, lstsq's lod, rank) of a case, computed once."""
    D, Z, Y, _ = build(case)
    out = scan_rule(D, Z, Y) + scan_lstsq(D, Z, Y)
    for a in out:
        a.setflags(write=False)
    return out


def deviation(got, want):
    """Worst |got - want| / max(1, |want|); infinities must coincide."""
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])), initial=0.0))
