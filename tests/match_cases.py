"""Panels, the numpy restatement and the planted cohort of the match pass (gbrs_hmm_set_panel / gbrs_hmm_match,
`gbrs reconstruct --match-panel`): plain numpy, no GPU.

The restatement is the definition itself: per handle chromosome an einsum of the sample's and the entry's dosage rows and
the two sums of squares.  Every sum has K = points x H non-negative terms, so in any order, fused or not, it is within a
relative (K + 1) 2^-53 of the exact value, and two orders are within 4 K 2^-53 of each other (rtol(); atol 0: a sum of
zeros is 0.0)."""
import functools
import itertools

import numpy as np

import grid_cases


def rtol(points, H):
    return 4 * max(points * H, 1) * 2.0 ** -53


def handle_points(chroms, grid):
    """Grid points per handle chromosome (0 off the grid) and their first dosage rows."""
    points = [len(grid.points[c]) if c in grid.points else 0 for c in chroms]
    return points, [int(o) for o in np.concatenate(([0], np.cumsum(points)[:-1]))]


def restate(dosage, panel, points, offsets):
    """(cross [n, n_chrom, M], sample_norm [n, n_chrom], panel_norm [M, n_chrom]) of dosage [n, P, H] and the panel's
    arrays [P, H] in handle order."""
    dosage = np.asarray(dosage, dtype=np.float64)
    b = np.stack(panel)
    n, M, nc = dosage.shape[0], len(panel), len(points)
    cross, snorm, pnorm = np.zeros((n, nc, M)), np.zeros((n, nc)), np.zeros((M, nc))
    for c, (m, o) in enumerate(zip(points, offsets)):
        if m:
            cross[:, c, :] = np.einsum("sph,jph->sj", dosage[:, o:o + m], b[:, o:o + m])
            snorm[:, c] = np.einsum("sph,sph->s", dosage[:, o:o + m], dosage[:, o:o + m])
            pnorm[:, c] = np.einsum("jph,jph->j", b[:, o:o + m], b[:, o:o + m])
    return cross, snorm, pnorm


def random_panel(rng, M, P, H):
    """M entries of non-negative dosages whose rows add up to 1, like a real panel's."""
    return [np.ascontiguousarray(rng.dirichlet(np.ones(H), size=P)) for _ in range(M)]


def states(H):
    return list(itertools.combinations_with_replacement(range(H), 2))


def one_hot_panel(rng, M, P, H):
    """M entries whose rows are the dosages of one diplotype each: values in {0, 1/2, 1}."""
    pairs = np.array(states(H))
    out = []
    for _ in range(M):
        picked = pairs[rng.integers(0, len(pairs), size=P)]
        d = np.zeros((P, H))
        np.add.at(d, (np.arange(P), picked[:, 0]), 0.5)
        np.add.at(d, (np.arange(P), picked[:, 1]), 0.5)
        out.append(d)
    return out


def rounded(a):
    """The numbers a `%.6f` dosage table gives back."""
    return np.array([float("%.6f" % x) for x in np.asarray(a).ravel()]).reshape(np.shape(a))


def to_grid_order(array, chroms, grid):
    """An entry's rows from handle order to the grid file's order (every grid chromosome is on the handle)."""
    points, offsets = handle_points(chroms, grid)
    return np.concatenate([array[offsets[chroms.index(c)]:offsets[chroms.index(c)] + len(grid.points[c])] for c in grid.points])


def to_handle_order(array, chroms, grid):
    first, row = {}, 0
    for c in grid.points:
        first[c] = row
        row += len(grid.points[c])
    return np.concatenate([array[first[c]:first[c] + len(grid.points[c])] for c in chroms if c in grid.points])


def write_dosage_table(path, rows, haplotypes):
    with open(path, "w") as fh:
        fh.write("# " + "\t".join(haplotypes) + "\n")
        for r in rows:
            fh.write("\t".join("%.6f" % x for x in r) + "\n")
    return str(path)


def write_panel(workdir, ids, arrays_grid_order, haplotypes, name="panel.txt"):
    """A panel file and its dosage tables (arrays in the grid file's order).  Returns the panel file's path."""
    lines = ["# id\tpath", ""]
    for k, (panel_id, a) in enumerate(zip(ids, arrays_grid_order)):
        lines.append(f"{panel_id}\t{write_dosage_table(workdir / f'panel_{k}.tsv', a, haplotypes)}")
    (workdir / name).write_text("\n".join(lines) + "\n")
    return str(workdir / name)


# ---- the planted cohort --------------------------------------------------------------------------------------------------

PLANTED_H, PLANTED_STYLE, PLANTED_GRID, PLANTED_SAMPLES, PLANTED_UNRELATED = 8, "benign", "b", 7, 10
PLANTED_MARGIN = 1e-3


def planted_panel(own, seed):
    """(ids, arrays, position of every sample's own entry): the rounded dosages `own` [n, P, H] in an order shuffled by
    `seed`, among PLANTED_UNRELATED one-diplotype-per-point entries drawn with it."""
    rng = np.random.default_rng(seed)
    n, P, H = np.shape(own)
    arrays = [rounded(a) for a in own] + one_hot_panel(rng, PLANTED_UNRELATED, P, H)
    ids = [f"animal{s}" for s in range(n)] + [f"other{k}" for k in range(PLANTED_UNRELATED)]
    order = rng.permutation(len(arrays))
    return [ids[k] for k in order], [arrays[k] for k in order], [int(np.flatnonzero(order == s)[0]) for s in range(n)]


def margins(dosage, arrays, points, offsets):
    """Per sample (index of the best entry, second distance - best distance) from the restatement's sums."""
    from gbrs_amd.hmm import match_scores, rank_matches
    cross, snorm, pnorm = restate(dosage, arrays, points, offsets)
    distance, _ = match_scores(cross, snorm, pnorm, points, np.asarray(points) > 0)
    ranks = [rank_matches(list(range(len(arrays))), d) for d in distance]
    return [r["best"] for r in ranks], [r["margin"] for r in ranks], distance


@functools.lru_cache(maxsize=None)
def planted_seed():
    """The first seed for which the composed oracle of tests/grid_cases.py (reconstruct_arrays + interpolate + dosage)
    separates every sample's own entry from the next one by at least twice PLANTED_MARGIN."""
    p0 = grid_cases.problem(PLANTED_H, PLANTED_STYLE)
    grid = grid_cases.grids()[PLANTED_GRID]
    points, offsets = handle_points(p0.chroms, grid)
    own = np.stack([to_handle_order(grid_cases.expected_for(PLANTED_H, PLANTED_STYLE, s, PLANTED_GRID)[1], p0.chroms, grid)
                    for s in range(PLANTED_SAMPLES)])
    for seed in range(64):
        _, arrays, where = planted_panel(own, seed)
        best, margin, _ = margins(own, arrays, points, offsets)
        if best == where and min(margin) >= 2 * PLANTED_MARGIN:
            return seed
    raise AssertionError("no seed separates the planted cohort")
