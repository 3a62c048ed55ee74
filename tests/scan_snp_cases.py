"""SNP sets and the three host computations of the SNP association scan (gbrs_scan_set_snps / gbrs_scan_snps,
GenomeScan.run_snps): plain numpy, no GPU.  The cohorts, covariates and phenotypes are those of
tests/scan_cases.py.

snp_dosage_rule restates where a SNP lies and its dosage, operation for operation: the device's dosages equal it bit for
bit.  snp_rule restates the test - projection on the covariates' basis, the threshold, w - with numpy's sums.  snp_lstsq
knows nothing of the rule: np.linalg.lstsq on [Z | x] with rcond=1e-10, and on Z alone for rss0.  None is the code under
test; the worst difference between the last two is the figure from which a case's tolerances are taken."""
import functools

import numpy as np

import scan_cases as base

PIVOT = base.PIVOT                         # the used rule's threshold: G > PIVOT raw
UNDECIDED = base.UNDECIDED                 # a ratio G / raw in this band could flip `used` by rounding
DEVICE_FACTOR = base.DEVICE_FACTOR         # the device against each host route: ten times the case's measured figure
CPU_HEADROOM = base.CPU_HEADROOM           # the two host routes between themselves

ALL_CASES = base.CASES + base.LARGE_CASES
# A cohort whose two grid points, 2 H n 8 = 166,400 bytes, exceed the 160 KB of LDS a gfx950 workgroup can have: the row
# kernel reads the cohort itself for every SNP.  Apart from ALL_CASES, so that what is measured over those stays as it is.
DIRECT = (8, 1300, 2, 2, base.POINTS)
case_id = base.case_id

# Worst |snp_rule - snp_lstsq| / max(1, |lod|) over the main SNP set of every case, measured on the CPU
# (test_scan_snp_cpu.py prints it): the measured numbers themselves, not bounds on them.
MEASURED = {
    'H2-n3-c1-P1-M17': 8.76e-15, 'H2-n32-c2-P64-M17': 7.16e-15, 'H3-n7-c4-P63-M17': 1.28e-13, 'H3-n33-c1-P65-M17': 6.35e-15,
    'H4-n31-c2-P130-M17': 8.22e-15, 'H8-n9-c1-P64-M17': 2e-15, 'H8-n70-c4-P130-M75': 2.02e-14, 'H8-n32-c2-P1-M17': 1.54e-15,
    'H9-n33-c1-P63-M17': 6.99e-15, 'H9-n13-c4-P65-M17': 2.61e-15, 'H10-n31-c2-P64-M17': 5.95e-15,
    'H10-n11-c1-P1-M17': 2.51e-15, 'H16-n70-c4-P65-M17': 1.69e-14, 'H16-n18-c2-P130-M17': 3.55e-15,
    'H16-n32-c1-P63-M17': 6.11e-15, 'H8-n256-c1-P1-M17': 2.47e-14, 'H8-n257-c2-P65-M17': 1.23e-13,
    'H9-n512-c2-P130-M75': 3.93e-13, 'H4-n129-c2-P64-M17': 4.83e-14, 'H17-n33-c1-P63-M17': 8.33e-15,
    'H17-n300-c4-P65-M17': 2.02e-13, 'H17-n19-c2-P1-M17': 1.44e-15, 'H8-n130-c64-P64-M17': 5e-14,
    'H16-n80-c64-P1-M17': 7.71e-15,
    'H8-n1300-c2-P2-M17': 1.07e-12,          # DIRECT
}
# Over the 24 main sets (67 SNPs each) `used` equals lstsq's rank everywhere; the smallest kept ratio G / raw is 7.9e-5
# and the largest skipped 4.4e-29, so no SNP lies in UNDECIDED and the tests exclude nothing.  The rule's dosages differ
# from the np.interp route by at most 1.4e-15.


def cpu_bound(case):
    return CPU_HEADROOM * MEASURED[case_id(case)]


def device_tol(case):
    return DEVICE_FACTOR * MEASURED[case_id(case)]


def grid_of(case):
    """Per chromosome, sorted random positions; chromosomes of 5 points or more have one duplicated position, at the
    indices k // 2 and k // 2 + 1."""
    H, n, c, P, points = case
    rng = np.random.default_rng(77000 + 1000 * H + 10 * n + c)
    grid = []
    for k in points:
        g = np.sort(rng.uniform(5.0, 95.0, size=k))
        if k >= 5:
            g[k // 2 + 1] = g[k // 2]
        g.setflags(write=False)
        grid.append(g)
    return grid


def _pack(case, per_chrom):
    """(grid, snp_pos, masks, labels) from per chromosome lists of (position, pattern, label)."""
    pos = [np.array([e[0] for e in entries], dtype=np.float64) for entries in per_chrom]
    masks = [np.array([e[1] for e in entries], dtype=np.uint32) for entries in per_chrom]
    labels = [e[2] for entries in per_chrom for e in entries]
    return grid_of(case), pos, masks, labels


@functools.lru_cache(maxsize=None)
def main_set(case):
    """(grid, snp_pos, masks, labels): the main SNP set of a case, every chromosome sorted by position.  Per chromosome
    of 5 points or more: a SNP before the first grid point and one after the last, on the first, the last and a middle
    point, on the duplicated position, between the duplicated position and its successor, 23 random positions, and a
    pattern with its complement at one position.  On the one-point chromosome: before, on and after the point.
    Patterns: all zeros, all ones and every one-hot among the 23, random ones elsewhere.  labels[j] names SNP j (handle
    order) where a test looks for it."""
    H, n, c, P, points = case
    rng = np.random.default_rng(78000 + 1000 * H + 10 * n + c)
    full = (1 << H) - 1
    mixed = lambda: int(rng.integers(1, full)) if full > 1 else 1            # neither all zeros nor all ones
    per_chrom = []
    for ci, (k, g) in enumerate(zip(points, grid_of(case))):
        if k < 5:
            entries = [(g[0] - 1.0, mixed(), f'{ci}:before'), (g[0], 1, f'{ci}:on'), (g[0] + 1.0, full ^ 1, f'{ci}:after')]
            per_chrom.append(entries)
            continue
        d = k // 2
        entries = [(g[0] - 1.5, mixed(), f'{ci}:before'), (g[-1] + 2.0, mixed(), f'{ci}:after'), (g[0], mixed(), f'{ci}:first'),
                   (g[-1], mixed(), f'{ci}:last'), (g[1], mixed(), f'{ci}:middle'), (g[d], mixed(), f'{ci}:duplicate'),
                   (0.5 * (g[d + 1] + g[d + 2]), mixed(), f'{ci}:past-duplicate')]
        pool = [0, full] + [1 << h for h in range(H)]
        for i, x in enumerate(rng.uniform(g[0], g[-1], size=23)):
            if i < len(pool):
                name = 'zeros' if i == 0 else 'ones' if i == 1 else f'onehot{i - 2}'
                entries.append((x, pool[i], f'{ci}:{name}'))
            else:
                entries.append((x, mixed(), f'{ci}:random'))
        x, m = rng.uniform(g[0], g[-1]), mixed()
        entries += [(x, m, f'{ci}:pattern'), (x, full ^ m, f'{ci}:complement')]
        entries.sort(key=lambda e: e[0])
        per_chrom.append(entries)
    return _pack(case, per_chrom)


@functools.lru_cache(maxsize=None)
def sized_set(case, count):
    """`count` SNPs with random patterns at sorted random positions, all on the second chromosome: around the row tile,
    and the other chromosomes have no SNPs."""
    H, n, c, P, points = case
    rng = np.random.default_rng(79000 + count)
    g = grid_of(case)[1]
    full = (1 << H) - 1
    x = np.sort(rng.uniform(g[0] - 1.0, g[-1] + 1.0, size=count))
    entries = [(x[i], int(rng.integers(1, full)) if full > 1 else 1, f'1:{i}') for i in range(count)]
    return _pack(case, [entries if ci == 1 else [] for ci in range(len(points))])


def descending_set(case):
    """The main set with every chromosome's SNPs in descending order of position."""
    grid, pos, masks, labels = main_set(case)
    off = np.concatenate(([0], np.cumsum([len(x) for x in pos])))
    flipped = [label for a, b in zip(off[:-1], off[1:]) for label in labels[a:b][::-1]]
    return grid, [x[::-1].copy() for x in pos], [m[::-1].copy() for m in masks], flipped


def locate(g, x):
    """(lo, hi, t) of the positions x on the grid g of one chromosome, by the rule."""
    k = len(g)
    lo = np.clip(np.searchsorted(g, x, 'right') - 1, 0, k - 1)
    hi = np.minimum(lo + 1, k - 1)
    gl, gh = g[lo], g[hi]
    inside = (gh > gl) & (x > gl)
    t = np.where(inside, (x - gl) / np.where(inside, gh - gl, 1.0), 0.0)
    return lo, hi, np.minimum(t, 1.0)


def snp_dosage_rule(D, points, grid, pos, masks):
    """X [n, M_snp], SNPs in handle order: x_s = 2.0 * (a_lo + t * (a_hi - a_lo)), the pattern's founders added in
    ascending order from 0.0 (adding 0.0 for a founder the pattern lacks changes no bit: the dosages are not negative)."""
    n, M, H = D.shape
    off = np.concatenate(([0], np.cumsum(points)))
    out = []
    for ci in range(len(points)):
        if len(pos[ci]) == 0:
            continue
        lo, hi, t = locate(grid[ci], pos[ci])
        a_lo, a_hi = np.zeros((n, len(lo))), np.zeros((n, len(lo)))
        for h in range(H):
            bit = ((masks[ci] >> np.uint32(h)) & np.uint32(1)).astype(bool)
            a_lo = a_lo + np.where(bit, D[:, off[ci] + lo, h], 0.0)
            a_hi = a_hi + np.where(bit, D[:, off[ci] + hi, h], 0.0)
        out.append(2.0 * (a_lo + t * (a_hi - a_lo)))
    return np.concatenate(out, axis=1) if out else np.zeros((n, 0))


def snp_dosage_interp(D, points, grid, pos, masks):
    """The same dosages by another route: 2 sum_h bit_h np.interp(x, g, D[s, :, h]).  np.interp needs increasing
    positions, so a chromosome with the duplicated position is two grids: the points up to the first of the equal pair
    serve the SNPs before that position, the points from the second on serve the others - the rule takes the last of
    the equal points for a SNP on them."""
    n, M, H = D.shape
    off = np.concatenate(([0], np.cumsum(points)))
    out = []
    for ci, k in enumerate(points):
        if len(pos[ci]) == 0:
            continue
        g, Dc = grid[ci], D[:, off[ci]:off[ci + 1]]
        same = np.flatnonzero(g[1:] == g[:-1])
        assert len(same) <= 1
        parts = [(slice(0, k), np.ones(len(pos[ci]), dtype=bool))]
        if len(same):
            d = int(same[0])
            parts = [(slice(0, d + 1), pos[ci] < g[d]), (slice(d + 1, k), pos[ci] >= g[d])]
        x = np.zeros((n, len(pos[ci])))
        for part, sel in parts:
            for h in range(H):
                bit = ((masks[ci][sel] >> np.uint32(h)) & np.uint32(1)).astype(np.float64)
                x[:, sel] += bit * np.stack([np.interp(pos[ci][sel], g[part], Dc[s, part, h]) for s in range(n)])
        out.append(2.0 * x)
    return np.concatenate(out, axis=1) if out else np.zeros((n, 0))


def snp_rule(X, Z, Y):
    """(lod [P, M_snp], used [M_snp], ratio G / raw [M_snp]; NaN where raw is 0) by the rule, with numpy's sums."""
    n = len(X)
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    rss0 = (Yt * Yt).sum(axis=0)
    raw = (X * X).sum(axis=0)
    Xt = X - Q @ (Q.T @ X)
    G = (Xt * Xt).sum(axis=0)
    used = (G > 0.0) & (G > PIVOT * raw)
    W = np.where(used, Xt / np.sqrt(np.where(used, G, 1.0)), 0.0)
    ess = (W.T @ Yt) ** 2                                   # [M_snp, P]
    lod = base.lod_of(n, rss0[None, :], rss0[None, :] - ess).T
    lod[:, ~used] = 0.0
    ratio = np.where(raw > 0.0, G / np.where(raw > 0.0, raw, 1.0), np.nan)
    return np.ascontiguousarray(lod), used, ratio


def snp_lstsq(X, Z, Y):
    """(lod [P, M_snp], rank of x beside Z [M_snp]) by np.linalg.lstsq."""
    n, c = Z.shape
    b0 = np.linalg.lstsq(Z, Y, rcond=1e-10)[0]
    r0 = Y - Z @ b0
    rss0 = (r0 * r0).sum(axis=0)
    lod, rank = np.empty((Y.shape[1], X.shape[1])), np.empty(X.shape[1], dtype=np.int32)
    for j in range(X.shape[1]):
        A = np.hstack([Z, X[:, j:j + 1]])
        b, _, rk, _ = np.linalg.lstsq(A, Y, rcond=1e-10)
        r1 = Y - A @ b
        lod[:, j] = base.lod_of(n, rss0, (r1 * r1).sum(axis=0))
        rank[j] = rk - c
    return lod, rank


def snp_peaks(lod, used, counts):
    """(peak_lod [P, n_chrom], peak_index [P, n_chrom]): the first of the largest over the used SNPs of a chromosome,
    NaN and -1 where it has none."""
    off = np.concatenate(([0], np.cumsum(counts)))
    P = len(lod)
    peak, index = np.full((P, len(counts)), np.nan), np.full((P, len(counts)), -1, dtype=np.int64)
    for ci, (a, b) in enumerate(zip(off[:-1], off[1:])):
        on = a + np.flatnonzero(used[a:b])
        if len(on):
            best = lod[:, on].argmax(axis=1)
            index[:, ci] = on[best]
            peak[:, ci] = lod[np.arange(P), on[best]]
    return peak, index


@functools.lru_cache(maxsize=None)
def expected(case):
    """(X, rule's lod, used, ratio, lstsq's lod, rank) of a case's main set, computed once."""
    D, Z, Y, _ = base.build(case)
    grid, pos, masks, _ = main_set(case)
    X = snp_dosage_rule(D, case[4], grid, pos, masks)
    out = (X,) + snp_rule(X, Z, Y) + snp_lstsq(X, Z, Y)
    for a in out:
        a.setflags(write=False)
    return out


def flat_snps(case):
    """The SNPs of the main set with the all-zeros or the all-ones pattern whose dosage is the same in every sample.  The
    all-ones pattern is flat where the rows of D add up to 1: next to the cohort's `equal` point, whose rows do not, it
    is an ordinary SNP."""
    X, labels = expected(case)[0], main_set(case)[3]
    return [j for j, label in enumerate(labels) if label.endswith((':zeros', ':ones')) and np.ptp(X[:, j]) < 1e-12]


def complement_pairs(case):
    """(a, b): a pattern and its complement at one position whose dosages add up to the same number in every sample (as
    they do wherever the rows of D add up to 1): equal LODs up to rounding."""
    X, labels = expected(case)[0], main_set(case)[3]
    pairs = [(labels.index(f'{ci}:pattern'), labels.index(f'{ci}:complement')) for ci, k in enumerate(case[4]) if k >= 5]
    return [(a, b) for a, b in pairs if np.ptp(X[:, a] + X[:, b]) < 1e-12]


deviation = base.deviation
