"""The permutation rule of the genome scan (gbrs_scan_permute, GenomeScan.permute) restated in numpy: no
GPU, and not the code under test.

permutations draws the keys with bootstrap_restate.philox4x32_10 and ranks them with np.lexsort; permuted_columns is
steps 1-3 of the rule; expected runs the permuted columns through the two host computations of tests/scan_cases.py
(scan_rule, the rule restated, and scan_lstsq, which knows nothing of it) and takes the maxima."""
import functools

import numpy as np

import scan_cases as cases
from bootstrap_restate import MASK32, philox4x32_10

# Worst |scan_rule - scan_lstsq| / max(1, |lod|) over every LOD (not only the maxima) of the permuted columns of the
# ordinary cases at B = N_PERM permutations under SEED, measured on the CPU: test_scan_perm_cpu.py prints the figure
# per case and the largest is written here as it came out.  It is the measured number itself, not a bound on it; the
# CPU test allows scan_cases.CPU_HEADROOM times it between the host routes, the device scan_cases.DEVICE_FACTOR times
# it against either (§27's argument: the device adds the samples in another, fixed order and fuses nothing).
MEASURED_FLOOR_PERM = 1.98e-14            # H8-n70-c4-P130-M75; the other eight cases measured 2.8e-15 .. 1.03e-14
N_PERM = 5
SEED = 20260
SEED_HIGH = (1 << 40) + 977               # a seed whose upper word is in use

# The cases with more than one residual degree of freedom.  With n = c + H a column's floor depends on how close the
# permuted residual comes to the design's span (scan_cases.MEASURED_SATURATED), so those stay out of the tolerance
# tests and in the exact ones.  Pivot ratios depend on D alone: no grid point is undecided here either.
ORDINARY = [case for case in cases.CASES if case[1] > case[2] + case[0]]
# The same of scan_cases.LARGE_CASES, and the same figure of each (B = N_PERM, SEED), its own as in
# scan_cases.MEASURED_LARGE: the absolute rounding of (n / 2) log10(rss0 / rss1) grows with n.
ORDINARY_LARGE = [case for case in cases.LARGE_CASES if case[1] > case[2] + case[0]]
MEASURED_PERM_LARGE = {'H8-n256-c1-P1-M17': 5.95e-14, 'H8-n257-c2-P65-M17': 1.23e-13, 'H9-n512-c2-P130-M75': 4.16e-13,
                       'H4-n129-c2-P64-M17': 4.34e-14, 'H17-n33-c1-P63-M17': 5.19e-15, 'H17-n300-c4-P65-M17': 8.65e-14,
                       'H8-n130-c64-P64-M17': 3.66e-14}
# The event ring's pass (test_scan_perm_gpu.py): the first RING_PHENO phenotypes of RING under RING_PERM permutations
# are nine chunks of 512 columns.  The figure is the same quantity over all 4,608 columns of that very run, and the
# device is held to scan_cases.DEVICE_FACTOR times it alone.
RING, RING_PHENO, RING_PERM = (3, 33, 1, 65, cases.POINTS), 9, 512
MEASURED_RING = 8.66e-15


def measured_floor_perm(case):
    """As scan_cases.measured_floor: the larger of the floor over ORDINARY and the case's own figure."""
    return max(MEASURED_FLOOR_PERM, MEASURED_PERM_LARGE.get(cases.case_id(case), 0.0))


def permutations(seed, B, n):
    """int32[B][n]: row b is the rank of (key_s, s) among the n pairs, key_s = (w0 << 32) | w1 of Philox4x32-10 on the
    counter (s, b) under the seed.  It depends on (seed, b, n) alone."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & MASK32, seed >> 32)
    s = np.arange(n, dtype=np.uint64)
    out = np.empty((B, n), dtype=np.int32)
    for b in range(B):
        w = philox4x32_10((s & np.uint64(MASK32), s >> np.uint64(32), np.full(n, b & MASK32, dtype=np.uint64),
                           np.full(n, b >> 32, dtype=np.uint64)), key)
        k = (w[0] << np.uint64(32)) | w[1]
        order = np.lexsort((s, k))                               # by key, ties by sample
        out[b, order] = np.arange(n, dtype=np.int32)
    return out


def permuted_columns(Z, Y, perm):
    """[n, P B], column p B + b: y~ = y - Q Q'y, y*[s] = y~[perm_b[s]], y*~ = y* - Q Q'y*."""
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    star = np.stack([Yt[row] for row in perm], axis=2)           # [n, P, B]
    star = star.reshape(len(Y), -1)
    return star - Q @ (Q.T @ star)


def masked_max(lod, points, mask=None):
    """The largest LOD over the grid points of the selected chromosomes, per column."""
    off = np.concatenate(([0], np.cumsum(points)))
    on = np.zeros(lod.shape[1], dtype=bool)
    for c, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if mask is None or mask[c]:
            on[a:b] = True
    return lod[:, on].max(axis=1)


@functools.lru_cache(maxsize=None)
def expected(case, B=N_PERM, seed=SEED):
    """(permutations [B, n], LODs of the permuted columns [P B, M] by scan_rule, the same by scan_lstsq), computed once."""
    D, Z, Y, _ = cases.build(case)
    perm = permutations(seed, B, case[1])
    columns = permuted_columns(Z, Y, perm)
    out = (perm, cases.scan_rule(D, Z, columns)[0], cases.scan_lstsq(D, Z, columns)[0])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_ring():
    """expected() of the event ring's pass: RING's first RING_PHENO phenotypes, RING_PERM permutations under SEED."""
    D, Z, Y, _ = cases.build(RING)
    perm = permutations(SEED, RING_PERM, RING[1])
    columns = permuted_columns(Z, Y[:, :RING_PHENO], perm)
    out = (perm, cases.scan_rule(D, Z, columns)[0], cases.scan_lstsq(D, Z, columns)[0])
    for a in out:
        a.setflags(write=False)
    return out


def expected_max(case, B=N_PERM, seed=SEED, mask=None):
    """(perm_max [P, B] by scan_rule, by scan_lstsq)."""
    _, rule, lstsq = expected(case, B, seed)
    return tuple(masked_max(lod, case[4], mask).reshape(case[3], B) for lod in (rule, lstsq))
