"""Inputs for the edge tests of the four small device operations (alignment counts, compress, interpolate, dosage), and
a numpy restatement of the row key that `gbrs compress` sorts by.  No GPU import: tests/test_small_ops_cpu.py checks the
generators and the oracles here, the *_edges_gpu.py files run the same inputs on the device.

A case is a `Case`: canonical CSC arrays per haplotype (`indptr` uint32[L + 1], `indices` uint32[nnz], row ids ascending
inside a column), an optional integer-valued `count`, and an optional `locus_group` (int32[L], -1 = in no gene) with
`num_out` genes."""
from dataclasses import dataclass
from math import fsum

import numpy as np


@dataclass
class Case:
    R: int
    L: int
    H: int
    indptr: list
    indices: list
    count: object = None
    locus_group: object = None
    num_out: int = 0

    @property
    def N(self):
        return int(sum(len(i) for i in self.indices))

    def with_groups(self, locus_group, num_out):
        return Case(self.R, self.L, self.H, self.indptr, self.indices, self.count,
                    np.asarray(locus_group, dtype=np.int32), int(num_out))


def csc_from_triplets(R, L, H, rows, loci, haps, count=None):
    """Canonical CSC arrays from (row, locus, hap) entries; a repeated entry is an error of the caller."""
    rows, loci, haps = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (rows, loci, haps))
    assert len(rows) == len(loci) == len(haps)
    if len(rows):
        assert 0 <= rows.min() and rows.max() < R and 0 <= loci.min() and loci.max() < L
        assert 0 <= haps.min() and haps.max() < H
    indptr, indices = [], []
    edges = np.arange(L + 1, dtype=np.int64)
    for h in range(H):
        sel = haps == h
        r, l = rows[sel], loci[sel]
        order = np.lexsort((r, l))
        r, l = r[order], l[order]
        assert not ((r[1:] == r[:-1]) & (l[1:] == l[:-1])).any(), "repeated (row, locus, hap) entry"
        indices.append(r.astype(np.uint32))
        indptr.append(np.searchsorted(l, edges).astype(np.uint32))
    if count is not None:
        count = np.asarray(count, dtype=np.float64)
        assert count.shape == (R,) and (count == np.rint(count)).all()
    return Case(R, L, H, indptr, indices, count)


def csc_from_masks(R, L, H, rows, loci, masks, count=None):
    """Canonical CSC arrays from (row, locus, mask) entries: bit h of `mask` = the row aligns to (locus, hap h)."""
    rows, loci, masks = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (rows, loci, masks))
    assert len(rows) == len(loci) == len(masks)
    assert (masks > 0).all() and (masks < (1 << H)).all()
    rr, ll, hh = [], [], []
    for h in range(H):
        sel = ((masks >> h) & 1) == 1
        rr.append(rows[sel]); ll.append(loci[sel]); hh.append(np.full(int(sel.sum()), h, dtype=np.int64))
    return csc_from_triplets(R, L, H, np.concatenate(rr), np.concatenate(ll), np.concatenate(hh), count)


def csc_from_rows(L, H, row_list, count=None):
    """`row_list[r]` = [(locus, mask), ...] of row r (an empty list = a row without alignments)."""
    rows, loci, masks = [], [], []
    for r, pairs in enumerate(row_list):
        for l, m in pairs:
            rows.append(r); loci.append(l); masks.append(m)
    return csc_from_masks(len(row_list), L, H, rows, loci, masks, count)


def triplets_of(case):
    """(rows, loci, haps) of a case, in column order."""
    rows, loci, haps = [], [], []
    for h in range(case.H):
        ptr = case.indptr[h].astype(np.int64)
        rows.append(case.indices[h].astype(np.int64))
        loci.append(np.repeat(np.arange(case.L, dtype=np.int64), np.diff(ptr)))
        haps.append(np.full(len(rows[-1]), h, dtype=np.int64))
    return np.concatenate(rows), np.concatenate(loci), np.concatenate(haps)


# ---- brute force: plain Python over sets, for the oracles' own tests -------------------------------------------------
def brute_counts(case, grouped):
    """Alignment counts the slow way: per row the set of (locus', hap) it touches."""
    Lo = case.num_out if grouped else case.L
    w = np.ones(case.R) if case.count is None else case.count
    touched = [set() for _ in range(case.R)]
    for r, l, h in zip(*triplets_of(case)):
        lo = int(case.locus_group[l]) if grouped else int(l)
        if lo >= 0:
            touched[int(r)].add((lo, int(h)))
    aln, uniq, lu = np.zeros((case.H, Lo)), np.zeros((case.H, Lo)), np.zeros(Lo)
    for r, ent in enumerate(touched):
        for lo, h in ent:
            aln[h, lo] += w[r]
        if len(ent) == 1:
            (lo, h), = ent
            uniq[h, lo] += w[r]
        loc = {lo for lo, _ in ent}
        if len(loc) == 1:
            lu[loc.pop()] += w[r]
    return aln, uniq, lu


def brute_compress(case):
    """Equivalence classes the slow way: dict of frozenset((locus, hap)) in first-seen order."""
    w = np.ones(case.R) if case.count is None else case.count
    ent = [set() for _ in range(case.R)]
    for r, l, h in zip(*triplets_of(case)):
        ent[int(r)].add((int(l), int(h)))
    classes = {}
    for r in range(case.R):
        k = frozenset(ent[r])
        classes[k] = classes.get(k, 0.0) + w[r]
    rows, loci, haps = [], [], []
    for cid, k in enumerate(classes):
        for l, h in k:
            rows.append(cid); loci.append(l); haps.append(h)
    out = csc_from_triplets(max(len(classes), 1), case.L, case.H, rows, loci, haps)
    return len(classes), out.indptr, out.indices, np.array(list(classes.values()), dtype=np.float64)


# ---- the row key of compress (row_key_kernel in gbrs_amd/csrc/em_layout.hip) -----------------------------------------
# Restated only so that the collision cases can assert that they collide.  key = 24 bits of the first locus (shifted down
# when the locus ids need more than 24 bits) | 24 bits of a hash of the loci | 16 bits of a hash of the masks.
KEY_LOCUS_SEED, KEY_MASK_SEED = 0x811C9DC5, 0x01000193
_M32 = np.uint64(0xFFFFFFFF)


def mix32(h, v):
    """mix32 of the kernel on uint64 arrays that hold 32-bit values."""
    h = np.asarray(h, dtype=np.uint64)
    v = np.asarray(v, dtype=np.uint64)
    h = h ^ ((v + np.uint64(0x9E3779B9) + ((h << np.uint64(6)) & _M32) + (h >> np.uint64(2))) & _M32)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    return h ^ (h >> np.uint64(13))


def bits_for(max_value):
    b = 1
    while b < 64 and (max_value >> b):
        b += 1
    return b


def row_keys(L, loci, masks):
    """Keys of n rows that all have k (locus, mask) pairs: loci, masks are (n, k) arrays, loci ascending along k."""
    loci = np.asarray(loci, dtype=np.uint64).reshape(len(loci), -1)
    masks = np.asarray(masks, dtype=np.uint64).reshape(len(masks), -1)
    hl = np.full(len(loci), KEY_LOCUS_SEED, dtype=np.uint64)
    hm = np.full(len(loci), KEY_MASK_SEED, dtype=np.uint64)
    for j in range(loci.shape[1]):
        hl = mix32(hl, loci[:, j])
        hm = mix32(hm, masks[:, j])
    lbits = bits_for(L - 1)
    shift = np.uint64(lbits - 24 if lbits > 24 else 0)
    primary = (loci[:, 0] >> shift) & np.uint64(0xFFFFFF)
    return (primary << np.uint64(40)) | ((hl & np.uint64(0xFFFFFF)) << np.uint64(16)) | (hm & np.uint64(0xFFFF))


def shared_key_count(keys):
    """How many of the given rows share their key with another of them."""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


# ---- compress cases ----------------------------------------------------------------------------------------------------
def _copies_shuffled(rng, n_distinct, max_copies):
    """Row -> distinct-row index: every distinct row 1..max_copies times, shuffled."""
    which = np.repeat(np.arange(n_distinct), rng.integers(1, max_copies + 1, size=n_distinct))
    rng.shuffle(which)
    return which


def h16_collision_masks():
    """12,000 distinct 16-haplotype masks (seed fixed: the CPU test asserts how many share a key)."""
    rng = np.random.default_rng(16)
    masks = rng.choice(np.arange(1, 1 << 16), size=12_000, replace=False)
    return masks.astype(np.int64)


def h16_collision_case(with_count):
    """H = 16, L = 3, one-locus rows on locus 1: 12,000 distinct masks, each 1-3 times, shuffled (about 24k rows)."""
    masks = h16_collision_masks()
    rng = np.random.default_rng(161)
    which = _copies_shuffled(rng, len(masks), 3)
    R = len(which)
    count = rng.integers(1, 5, size=R).astype(np.float64) if with_count else None
    return csc_from_masks(R, 3, 16, np.arange(R), np.ones(R, dtype=np.int64), masks[which], count)


def h8_collision_pairs():
    """255 x 40 mask pairs on loci (0, 1) at H = 8: every mask of locus 0 with 40 distinct masks of locus 1."""
    rng = np.random.default_rng(8)
    first = np.repeat(np.arange(1, 256), 40)
    second = np.concatenate([rng.choice(np.arange(1, 256), size=40, replace=False) for _ in range(255)])
    return np.stack((first, second), axis=1).astype(np.int64)


def h8_collision_case():
    """H = 8, two-locus rows on loci (0, 1): 10,200 mask pairs, each 1-2 times, shuffled, with 300 empty rows mixed in."""
    pairs = h8_collision_pairs()
    rng = np.random.default_rng(81)
    which = _copies_shuffled(rng, len(pairs), 2)
    which = np.concatenate((which, np.full(300, -1)))
    rng.shuffle(which)
    first_live = int(np.flatnonzero(which >= 0)[0])
    which[[0, first_live]] = which[[first_live, 0]]                    # the first row is not an empty one
    R = len(which)
    live = np.flatnonzero(which >= 0)
    rows = np.concatenate((live, live))
    loci = np.concatenate((np.zeros(len(live), dtype=np.int64), np.ones(len(live), dtype=np.int64)))
    masks = np.concatenate((pairs[which[live], 0], pairs[which[live], 1]))
    return csc_from_masks(R, 2, 8, rows, loci, masks)


def three_rows_one_key():
    """Three distinct H = 16 masks on locus 1 (L = 3) whose rows share one key, found with the restated key."""
    masks = np.arange(1, 1 << 16, dtype=np.int64)
    keys = row_keys(3, np.ones(len(masks), dtype=np.int64), masks)
    uniq, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    first = int(np.flatnonzero(cnt >= 3)[0])
    found = masks[inv == first][:3]
    assert len(found) == 3
    return [int(m) for m in found]


def interleaved_case():
    """Rows A B C A B C ... (four copies each) of three rows under one key: three classes of count 4, in the order A, B, C."""
    a, b, c = three_rows_one_key()
    return csc_from_rows(3, 16, [[(1, m)] for m in (a, b, c) * 4])


def long_row_case():
    """A row on 3,000 loci, its identical twin, and a third row that differs in the mask of the last locus only."""
    rng = np.random.default_rng(3000)
    L, H = 3100, 4
    loci = np.sort(rng.choice(L, size=3000, replace=False))
    masks = rng.integers(1, 1 << H, size=3000)
    other = masks.copy()
    other[-1] = masks[-1] % ((1 << H) - 1) + 1        # another non-zero mask
    assert other[-1] != masks[-1]
    rows = [list(zip(loci.tolist(), masks.tolist())), [(5, 1)], list(zip(loci.tolist(), other.tolist())),
            list(zip(loci.tolist(), masks.tolist())), []]
    return csc_from_rows(L, H, rows)


BIG_L = (1 << 24) + 3


def large_l_case(L=BIG_L):
    """L just past 2^24 (the key's first-locus field is shifted), H = 2, R = 2,000.  Two-locus rows: the first locus is 2k or
    2k + 1 (one 24-bit field after the shift), the second one of the top loci >= 2^24; one-locus rows sit on a top locus,
    whose shifted first-locus field wraps to that of loci 0 and 1.  Half of the entries are on loci >= 2^24."""
    assert bits_for(L - 1) > 24
    rng = np.random.default_rng(24)
    top = np.arange(1 << 24, L)
    rows, loci, masks = [], [], []
    for r in range(2000):
        kind = r % 10
        if kind == 9:
            continue                                               # an empty row
        hi = int(rng.choice(top))
        if kind < 7:
            rows += [r, r]
            loci += [2 * int(rng.integers(0, 40)) + int(rng.integers(0, 2)), hi]
            masks += [int(rng.integers(1, 4)), int(rng.integers(1, 4))]
        else:
            rows.append(r); loci.append(hi); masks.append(int(rng.integers(1, 4)))
    return csc_from_masks(2000, L, 2, rows, loci, masks)


# ---- counts cases ------------------------------------------------------------------------------------------------------
def random_group_map(rng, L, num_out, ungrouped):
    """locus -> gene in no particular order, `ungrouped` of the loci in no gene."""
    g = rng.integers(0, num_out, size=L).astype(np.int32)
    g[rng.choice(L, size=ungrouped, replace=False)] = -1
    return g


def _random_pairs(rng, R, L, n_pairs):
    flat = rng.choice(R * L, size=min(n_pairs, R * L), replace=False)
    return flat // L, flat % L


def _sparse_masks(rng, H, n):
    """Non-zero masks of one to three set bits (any of the H bits, the top one included)."""
    m = np.zeros(n, dtype=np.int64)
    for _ in range(3):
        m |= np.int64(1) << rng.integers(0, H, size=n)
    return m


def counts_hap_case(H, with_count=True):
    """R = 4,000, L = 70, about 30k entries, a gene map that leaves ten loci out."""
    rng = np.random.default_rng(100 + H)
    R, L = 4000, 70
    rows, loci = _random_pairs(rng, R, L, 30_000 if H == 1 else 11_000)
    count = rng.integers(1, 6, size=R).astype(np.float64) if with_count else None
    case = csc_from_masks(R, L, H, rows, loci, _sparse_masks(rng, H, len(rows)), count)
    return case.with_groups(random_group_map(rng, L, 25, 10), 25)


def counts_row_case(R):
    """L = 9, H = 3; three loci in no gene; row R - 1 aligns to every locus, in a different haplotype set each."""
    rng = np.random.default_rng(200 + R)
    L, H = 9, 3
    rows, loci = _random_pairs(rng, max(R - 1, 0), L, 3000) if R > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    masks = rng.integers(1, 1 << H, size=len(rows))
    rows = np.concatenate((rows, np.full(L, R - 1)))
    loci = np.concatenate((loci, np.arange(L)))
    masks = np.concatenate((masks, np.arange(L) % 7 + 1))
    count = rng.integers(1, 4, size=R).astype(np.float64)
    case = csc_from_masks(R, L, H, rows, loci, masks, count)
    return case.with_groups([0, 0, -1, 1, 2, -1, 1, 3, -1], 4)


def counts_entry_case(N):
    """Exactly N entries, H = 3, L = 12: the first three and the last three columns of every haplotype are empty, the
    first haplotype's entries all sit in column 5."""
    rng = np.random.default_rng(300 + N)
    L, H = 12, 3
    n0 = (N + 2) // 3
    R = max(n0, 8) + 3
    cells = np.array([(h, l, r) for h in (1, 2) for l in range(3, 9) for r in range(R)])
    pick = cells[rng.choice(len(cells), size=N - n0, replace=False)] if N > n0 else np.zeros((0, 3), dtype=np.int64)
    rows = np.concatenate((np.arange(n0), pick[:, 2]))
    loci = np.concatenate((np.full(n0, 5), pick[:, 1]))
    haps = np.concatenate((np.zeros(n0, dtype=np.int64), pick[:, 0]))
    case = csc_from_triplets(R, L, H, rows, loci, haps)
    assert case.N == N
    return case.with_groups([0, 0, 0, 1, -1, 1, 2, 2, 0, 3, 3, 3], 4)


def counts_hand_case():
    """Five rows with weights 2, 3, 5, 7, 11 on three loci (loci 0 and 1 = the two isoforms of gene 0, locus 2 = gene 1)
    and two haplotypes: row 0 on both isoforms in haplotype 0, row 1 on locus 2 in both haplotypes, row 2 everywhere,
    rows 3 and 4 empty.  Returns the case and the expected (aln, allele_unique, locus_unique) per level."""
    case = csc_from_rows(3, 2, [[(0, 1), (1, 1)], [(2, 3)], [(0, 3), (1, 3), (2, 3)], [], []],
                         count=[2, 3, 5, 7, 11]).with_groups([0, 0, 1], 2)
    isoforms = (np.array([[7., 7., 8.], [5., 5., 8.]]), np.zeros((2, 3)), np.array([0., 0., 3.]))
    genes = (np.array([[7., 8.], [5., 8.]]), np.array([[2., 0.], [0., 0.]]), np.array([2., 3.]))
    return case, isoforms, genes


def counts_map_case():
    """R = 500, L = 20, H = 4: the matrix that the group-map and the several-queries tests put different maps on."""
    rng = np.random.default_rng(400)
    R, L, H = 500, 20, 4
    rows, loci = _random_pairs(rng, R, L, 2500)
    return csc_from_masks(R, L, H, rows, loci, rng.integers(1, 1 << H, size=len(rows)),
                          rng.integers(1, 4, size=R).astype(np.float64))


def group_maps(L=20):
    """name -> (locus_group, num_out) for counts_map_case."""
    rng = np.random.default_rng(401)
    return {
        "all_ungrouped": (np.full(L, -1, dtype=np.int32), 3),
        "one_gene": (np.zeros(L, dtype=np.int32), 1),
        "three_genes": (random_group_map(rng, L, 3, 4), 3),
        "fifty_genes": (random_group_map(rng, L, 50, 2), 50),            # more genes than loci: most have no locus
        "descending": (np.arange(L, dtype=np.int32)[::-1] // 2, L // 2),
    }


# ---- interpolate cases -------------------------------------------------------------------------------------------------
STATE_COUNTS = (1, 3, 36, 136)


def gamma_columns(S, n, seed):
    """S x n positive columns that sum to 1."""
    g = np.random.default_rng(seed).random((S, n)) + 1e-3
    return g / g.sum(axis=0)


def interp_positions():
    """name -> (gene positions (ascending, duplicates allowed), grid positions)."""
    rng = np.random.default_rng(7)
    genes = np.sort(rng.random(40) * 100.0 + 0.5)
    mids = 0.5 * (genes[1:] + genes[:-1])
    many_genes = np.sort(rng.random(500) * 90.0 + 0.25)
    tiny = np.array([1e-9, 2e-9, 3e-9, 0.5, 0.5 + 1e-9, 0.5 + 2e-9, 7.0, 1e6, 1e6 + 1e-9, 1e9])
    return {
        "on_knots": (genes, np.sort(np.concatenate((genes[::3], mids[::4])))),
        "grid_zero": (genes, np.concatenate(([0.0], mids[:5], [genes[-1] + 0.5]))),
        "two_at_one_position": (np.array([1.0, 2.5, 2.5, 4.0, 6.0]), np.array([1.75, 2.5, 3.0, 4.0, 5.0])),
        "three_at_one_position": (np.array([1.0, 4.0, 4.0, 4.0, 6.0]), np.array([0.5, 4.0, 4.5, 6.0, 6.5])),
        "one_gene": (np.array([3.0]), np.array([0.0, 1.0, 3.0, 3.5])),
        "before_first_gene": (np.array([10.25, 10.5, 10.75]), np.array([9.875, 10.0, 10.125])),
        "after_last_gene": (np.array([1.0, 2.0, 5.0]), np.array([6.0, 7.0, 9.0])),
        "one_grid_point": (genes, np.array([genes[-1] - 0.25])),
        "many_grid_points": (many_genes, np.sort(rng.random(3000) * 100.0)),
        "wide_range": (tiny, np.array([5e-10, 1e-9, 1.5e-9, 2.5e-9, 0.25, 0.5 + 1e-9, 0.5 + 1.5e-9, 3.0, 5e5,
                                       1e6 + 5e-10, 5e8, 1e9])),
    }


def interp_case(name, S):
    x_gene, x_grid = interp_positions()[name]
    return x_gene, gamma_columns(S, len(x_gene), 1000 + S), x_grid


# ---- dosage cases ------------------------------------------------------------------------------------------------------
def genotype_pairs(H):
    """(a, b) with a <= b, a outer: the order of the diplotype states (combinations_with_replacement)."""
    return [(a, b) for a in range(H) for b in range(a, H)]


def dosage_one_hot(H):
    """All S one-hot rows and the dosage by the hand rule: genotype (a, b) gives 0.5 to a and 0.5 to b, 1.0 to a = b."""
    pairs = genotype_pairs(H)
    expected = np.zeros((len(pairs), H))
    for g, (a, b) in enumerate(pairs):
        expected[g, a] += 0.5
        expected[g, b] += 0.5
    return np.eye(len(pairs)), expected


def dosage_random(H, n_rows):
    """Non-negative rows that sum to 1, and the dosage with every output element summed by math.fsum (halving and the
    products with 1.0 are exact, so the fsum is the correctly rounded exact value)."""
    S = H * (H + 1) // 2
    rows = np.random.default_rng(500 + 31 * H + n_rows).random((n_rows, S))
    rows /= rows.sum(axis=1, keepdims=True)
    terms = [[(g, 0.5 * ((a == h) + (b == h))) for g, (a, b) in enumerate(genotype_pairs(H)) if h in (a, b)]
             for h in range(H)]
    expected = np.zeros((n_rows, H))
    for r in range(n_rows):
        p = rows[r].tolist()
        for h in range(H):
            expected[r, h] = fsum(p[g] * w for g, w in terms[h])
    return rows, expected


def dosage_rtol(H):
    """2 S 2^-53: the bound for a length-S sum of non-negative products taken in any order, against the exact sum."""
    return 2 * (H * (H + 1) // 2) * 2.0 ** -53
