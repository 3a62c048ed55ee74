"""SNP sets and the rule of the imputation pass (gbrs_hmm_set_snps / gbrs_hmm_impute, `gbrs reconstruct --snp-file`;
DESIGN.md §26) restated in plain numpy, no GPU.  Shapes, gene positions and the composed oracle: tests/grid_cases.py.

The rule, for one sample and one chromosome with posteriors gamma (S x n_genes), gene positions, SNP positions x in file
order and patterns m (bit h: founder h carries the alternative allele):
  knots, knot_gene = stable sort of [0.0, gene positions..., last SNP in file order + 1.0]; the end knots carry gene 0
                     and gene n_genes - 1
  D[i][h] = acc over the states g = (a, b) in state order of gamma[g][i] * (0.5 * ((a == h) + (b == h)))
  idx  = clip(searchsorted(knots, x, 'left'), 1, n_knots - 1);  g_lo = knot_gene[idx - 1], g_hi = knot_gene[idx]
  a_lo = 0.0; for h ascending: if bit h of m: a_lo += D[g_lo][h];  a_hi likewise from D[g_hi]
  slope = (a_hi - a_lo) / (x_hi - x_lo);  y = slope * (x - x_lo) + a_lo;  out = 2.0 * y
Every operation is one rounding, in this order (the library is built without FMA contraction)."""
import collections
import functools

import numpy as np

import grid_cases

WIDTH = 256         # lanes of the imputation kernel's workgroup: SNP counts of WIDTH - 1, WIDTH and WIDTH + 1 are cases
SEED = 2626

# positions: per chromosome the genes' positions; points: per chromosome WITH SNPs their positions in file order (the
# dict's order is the file's chromosome order)
SnpSet = collections.namedtuple("SnpSet", "positions points")


def knots_of(gene_positions, points):
    """(knots, knot_gene) of one chromosome: grid_knots.h restated."""
    where = np.asarray(gene_positions, dtype=np.float64)
    x = np.concatenate(([0.0], where, [float(points[-1]) + 1.0]))
    order = np.argsort(x, kind="stable")
    return x[order], np.clip(order - 1, 0, len(where) - 1)


def gene_dosage(gamma, H):
    """D (n_genes x H) from gamma (S x n_genes): dosage_kernel's loop, one product and one sum per state in state order."""
    gamma = np.asarray(gamma, dtype=np.float64)
    D = np.zeros((gamma.shape[1], H))
    for h in range(H):
        acc = np.zeros(gamma.shape[1])
        g = 0
        for a in range(H):
            for b in range(a, H):
                acc = acc + gamma[g] * (0.5 * ((a == h) + (b == h)))
                g += 1
        D[:, h] = acc
    return D


def fold(D_rows, masks, H):
    """sum over the founders of each pattern, ascending, of the rows of D; a founder outside the pattern adds 0.0."""
    acc = np.zeros(len(masks))
    for h in range(H):
        acc = acc + np.where((masks >> np.uint32(h)) & np.uint32(1), D_rows[:, h], 0.0)
    return acc


def impute_chromosome(gene_positions, gamma, points, masks, H):
    """The rule for one (sample, chromosome): float64[len(points)]."""
    points = np.asarray(points, dtype=np.float64)
    masks = np.asarray(masks, dtype=np.uint32)
    knots, knot_gene = knots_of(gene_positions, points)
    D = gene_dosage(gamma, H)
    idx = np.clip(np.searchsorted(knots, points, side="left"), 1, len(knots) - 1)
    x_lo, x_hi = knots[idx - 1], knots[idx]
    a_lo, a_hi = fold(D[knot_gene[idx - 1]], masks, H), fold(D[knot_gene[idx]], masks, H)
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = (a_hi - a_lo) / (x_hi - x_lo)
        y = slope * (points - x_lo) + a_lo
    return 2.0 * y


def impute(chroms, snps, masks, gamma_of, H):
    """The rule for one sample over the chromosomes `chroms` (handle order): the SNPs of the handle's chromosomes one after
    the other, which is DiplotypeHMM.impute's column order.  gamma_of(c): the (S x n_genes) posteriors of chromosome c."""
    parts = [impute_chromosome(snps.positions[c], gamma_of(c), snps.points[c], masks[c], H) for c in chroms if c in snps.points]
    return np.concatenate(parts) if parts else np.zeros(0)


def bits_of(masks, H):
    """(M x H) 0.0 / 1.0 from uint32 patterns."""
    return ((np.asarray(masks, dtype=np.uint32)[:, None] >> np.arange(H, dtype=np.uint32)) & np.uint32(1)).astype(np.float64)


def pattern_text(mask, H):
    return "".join("1" if (int(mask) >> h) & 1 else "0" for h in range(H))


@functools.lru_cache(maxsize=None)
def snp_sets():
    """name -> SnpSet.  "a", "b", "unsorted": the grids of grid_cases.grids() as SNP positions (before the first and after
    the last gene, exactly on a gene position, on positions two and three genes share, 0.0, a chromosome without SNPs, the
    one-gene chromosome, file order different from the handle's, knots that need the stable sort).  "n255", "n256", "n257":
    that many SNPs on "X" - a workgroup short by one, full, and one lane into a second - with one position given twice,
    and a few on "2".  "descending": file order from the largest position down, so the end knot (last SNP in file order
    + 1.0) sorts in among the genes."""
    rng = np.random.default_rng(SEED)
    w = grid_cases.gene_positions()
    sets = {name: SnpSet(g.positions, g.points) for name, g in grid_cases.grids().items()}
    for count in (WIDTH - 1, WIDTH, WIDTH + 1):
        x = np.sort(rng.uniform(0.0, w["X"][-1] + 2.0, size=count - 1))
        x = np.insert(x, 100, x[100])                                        # one position twice, neighbours in the file
        sets[f"n{count}"] = SnpSet(w, {"X": x, "2": np.array([w["2"][0], 0.0, w["2"][1] + 0.25])})
    sets["descending"] = SnpSet(w, {
        "X": np.sort(rng.uniform(w["X"][3], w["X"][-1], size=70))[::-1].copy(),
        "4": np.sort(np.concatenate((rng.uniform(w["4"][0], w["4"][-1], size=9), [w["4"][10], w["4"][-1]])))[::-1].copy(),
    })
    for s in sets.values():
        for x in s.points.values():
            x.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def masks_for(name, H):
    """{chromosome: uint32 patterns} of a set for H founders: all zeros, all ones, every one-hot, then random, in turn along
    the file; the SNP after a repeated position gets another pattern than its twin by construction of the turn."""
    rng = np.random.default_rng(SEED + 31 * H + sum(map(ord, name)))
    full = (1 << H) - 1
    fixed = [0, full] + [1 << h for h in range(H)]
    out, k = {}, 0
    for c, x in snp_sets()[name].points.items():
        m = np.empty(len(x), dtype=np.uint32)
        for j in range(len(x)):
            turn = (k + j) % (len(fixed) + 3)
            m[j] = fixed[turn] if turn < len(fixed) else rng.integers(0, full + 1)
        k += len(x) + 1
        m.setflags(write=False)
        out[c] = m
    return out


NEEDS_SORTED_KNOTS = ("unsorted", "descending")     # sets whose knots are not ascending as they come


def _expected_sorted(p, snps, res):
    """grid_cases.expected for a set whose knots need the stable sort, which oracle.postproc_oracle.interpolate leaves to
    its caller: the same 36-state interpolation (interp1d's operations) on the sorted knots, then the oracle's dosage."""
    from oracle import postproc_oracle
    rows = []
    for c, x in snps.points.items():
        if c not in res:
            continue
        knots, knot_gene = knots_of(snps.positions[c], x)
        y = res[c]["gamma"][:, knot_gene]
        idx = np.searchsorted(knots, x).clip(1, len(knots) - 1)
        slope = (y[:, idx] - y[:, idx - 1]) / (knots[idx] - knots[idx - 1])[None, :]
        rows.append((slope * (x - knots[idx - 1])[None, :] + y[:, idx - 1]).T)
    return postproc_oracle.dosage(np.vstack(rows), len(p.hap_names))


def composed(p, snps, masks, res=None, sorted_knots=False):
    """The composed oracle for one sample: grid_cases.expected with the SNP set as the grid, then 2 * (dosage * bits)
    summed over the founders; the SNPs in the set's own (file) chromosome order.  sorted_knots: for the sets of
    NEEDS_SORTED_KNOTS, with `res` given."""
    H = len(p.hap_names)
    if sorted_knots:
        dosage = _expected_sorted(p, snps, res)
    else:
        _, dosage = grid_cases.expected(p, grid_cases.Grid(snps.positions, snps.points), res)
    bits = np.vstack([bits_of(masks[c], H) for c in snps.points if c in p.chroms])
    return 2.0 * (dosage * bits).sum(-1)


def handle_order(chroms, snps, values):
    """`values` over the set's SNPs in file chromosome order -> in the order of the chromosomes `chroms`."""
    first, row = {}, 0
    for c, x in snps.points.items():
        first[c] = row
        row += len(x)
    parts = [values[..., first[c]:first[c] + len(snps.points[c])] for c in chroms if c in snps.points]
    return np.concatenate(parts, axis=-1)


def write_snp_file(path, H, points, masks, extra=()):
    """A SNP file (id, chr, bp, cM, pattern) with the chromosomes in the order of `points`; `extra`: further
    (chromosome, cM, pattern) lines at the end.  Returns the path."""
    with open(path, "w") as fh:
        fh.write("id\tchr\tbp\tcM\tpattern\n")
        k = 0
        for c, xs in points.items():
            for x, m in zip(xs, masks[c]):
                fh.write(f"snp{k}\t{c}\t{int(x * 1e6)}\t{repr(float(x))}\t{pattern_text(m, H)}\n")
                k += 1
        for c, x, pattern in extra:
            fh.write(f"snp{k}\t{c}\t{int(x * 1e6)}\t{repr(float(x))}\t{pattern}\n")
            k += 1
    return str(path)
