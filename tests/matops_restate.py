"""numpy restatement of the structure edits behind `get-common-alignments`, `combine`, `pull-out-unique-reads` and
`stencil` (gbrs_amd/matops.py), checked against the imported reference by scripts/gen_golden_matops.py.  Test
infrastructure: numpy alone, one (column, row) key per stored entry; every result has its row ids ascending inside
every column, which is what scipy returns for the reference's operations."""
import numpy as np


def entry_keys(ip, ix, R):
    """column * R + row of every stored entry, in storage order."""
    col = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(np.asarray(ip, dtype=np.int64)))
    return col * int(R) + np.asarray(ix, dtype=np.int64)


def from_keys(keys, L, R):
    """(indptr, indices) of the distinct keys, columns and the row ids inside them ascending."""
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    ip = np.searchsorted(keys // int(R), np.arange(L + 1)).astype(np.uint32)
    return ip, (keys % int(R)).astype(np.uint32)


def canonical(R, L, H, indptr, indices):
    out = [from_keys(entry_keys(indptr[h], indices[h], R), L, R) for h in range(H)]
    return [o[0] for o in out], [o[1] for o in out]


def intersect(R, L, H, a, b):
    """a, b = (indptr list, indices list): the entries both hold (Sparse3DMatrix.__mul__ on incidence matrices)."""
    ip, ix = [], []
    for h in range(H):
        common = np.intersect1d(entry_keys(a[0][h], a[1][h], R), entry_keys(b[0][h], b[1][h], R))
        p, i = from_keys(common, L, R)
        ip.append(p)
        ix.append(i)
    return ip, ix


def append_rows(Ra, Rb, L, H, a, b):
    """The rows of a, then the rows of b (Sparse3DMatrix.combine: vstack per haplotype)."""
    R = Ra + Rb
    ip, ix = [], []
    for h in range(H):
        ka = entry_keys(a[0][h], a[1][h], R)
        kb = entry_keys(b[0][h], np.asarray(b[1][h], dtype=np.int64) + Ra, R)
        p, i = from_keys(np.concatenate((ka, kb)), L, R)
        ip.append(p)
        ix.append(i)
    return ip, ix


def unique_rows(R, L, H, indptr, indices, locus_group=None, ignore_haplotype=False):
    """bool[R]: the reads get_unique_reads keeps (AlignmentPropertyMatrix.py:389-411), at the gene level - after
    bundle(reset=True) - when locus_group (int[L], -1 = in no group) is given."""
    G = L if locus_group is None else int(np.max(locus_group)) + 1
    rows, keys = [], []
    for h in range(H):
        col = np.repeat(np.arange(L, dtype=np.int64), np.diff(np.asarray(indptr[h], dtype=np.int64)))
        g = col if locus_group is None else np.asarray(locus_group, dtype=np.int64)[col]
        ok = g >= 0
        rows.append(np.asarray(indices[h], dtype=np.int64)[ok])
        keys.append(g[ok] if ignore_haplotype else h * G + g[ok])
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    pairs = np.unique(rows * (H * G) + keys)          # distinct (row, key)
    return np.bincount(pairs // (H * G), minlength=R) == 1


def keep_rows(R, L, H, indptr, indices, keep):
    """pull_alignments_from (AlignmentPropertyMatrix.py:372-387): the entries of the rows with keep set."""
    ip, ix = [], []
    for h in range(H):
        k = entry_keys(indptr[h], indices[h], R)
        p, i = from_keys(k[keep[k % R]], L, R)
        ip.append(p)
        ix.append(i)
    return ip, ix


def mask_columns(R, L, H, indptr, indices, allowed):
    """multiply(gtmask, axis=2) + eliminate_zeros (gbrs/emase_utils.py:271-273) with gtmask[h, l] = bit h of allowed[l]."""
    ip, ix = [], []
    for h in range(H):
        k = entry_keys(indptr[h], indices[h], R)
        on = ((np.asarray(allowed, dtype=np.int64)[k // R] >> h) & 1).astype(bool)
        p, i = from_keys(k[on], L, R)
        ip.append(p)
        ix.append(i)
    return ip, ix


def make_case(R, H, L, seed, thin=0.2, drop=1 / 3, add=0.002):
    """The fixture recipe: synth.make_em_problem with a seeded `thin` share of the rows cut down to one entry each (so
    that allele-level unique reads exist), genes of 1-4 consecutive loci with the last loci in no gene, a second operand
    made by dropping `drop` of the entries and adding `add` random ones, a two-haplotype call per gene."""
    from gbrs_amd import synth
    inc = synth.make_em_problem(R=R, H=H, L=L, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    rows = np.concatenate([inc.indices[h].astype(np.int64) for h in range(H)])
    cols = np.concatenate([np.repeat(np.arange(L, dtype=np.int64), np.diff(inc.indptr[h].astype(np.int64))) for h in range(H)])
    haps = np.concatenate([np.full(len(inc.indices[h]), h, dtype=np.int64) for h in range(H)])
    thin_rows = rng.random(R) < thin
    order = rng.permutation(len(rows))
    first = np.zeros(len(rows), dtype=bool)
    _, where = np.unique(rows[order], return_index=True)      # one entry per row, chosen at random
    first[order[where]] = True
    keep = ~thin_rows[rows] | first
    rows, cols, haps = rows[keep], cols[keep], haps[keep]

    def csc(rows, cols, haps):
        ip, ix = [], []
        for h in range(H):
            sel = haps == h
            p, i = from_keys(cols[sel] * R + rows[sel], L, R)
            ip.append(p)
            ix.append(i)
        return ip, ix
    a = csc(rows, cols, haps)
    stay = rng.random(len(rows)) >= drop
    n_add = max(3 * H, int(add * len(rows)))            # dealt over the haplotypes: each gets some that a lacks
    rows_b = np.concatenate((rows[stay], rng.integers(0, R, size=n_add)))
    cols_b = np.concatenate((cols[stay], rng.integers(0, L, size=n_add)))
    haps_b = np.concatenate((haps[stay], np.arange(n_add, dtype=np.int64) % H))
    b = csc(rows_b, cols_b, haps_b)
    sizes, at = [], 0
    while at < L - max(2, L // 20):                     # the last loci stay in no gene
        s = int(rng.integers(1, 5))
        s = min(s, L - max(2, L // 20) - at)
        sizes.append(s)
        at += s
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    groups = [list(range(int(s), int(s + n))) for s, n in zip(starts, sizes)]
    locus_group = np.full(L, -1, dtype=np.int32)
    for g, members in enumerate(groups):
        locus_group[members] = g
    calls = [(int(x), int(y)) for x, y in rng.integers(0, H, size=(len(groups), 2))]
    allowed = np.zeros(L, dtype=np.uint32)
    for members, (x, y) in zip(groups, calls):
        allowed[members] = (1 << x) | (1 << y)
    return dict(R=R, H=H, L=L, a=a, b=b, groups=groups, locus_group=locus_group, calls=calls, allowed=allowed)


def nnz(m):
    return [len(i) for i in m[1]]


def check_not_vacuous(c, results):
    """The conditions every fixture must meet (asserted by the generator, repeated by the tests)."""
    R, H = c["R"], c["H"]
    na, nb, nc = nnz(c["a"]), nnz(c["b"]), nnz(results["common"])
    for h in range(H):
        assert 0 < nc[h] < min(na[h], nb[h]), (h, nc[h], na[h], nb[h])
    for key in ("keep_plain_allele", "keep_plain_locus", "keep_group_allele", "keep_group_locus"):
        share = float(np.mean(results[key]))
        assert 0.05 <= share <= 0.95, (key, share)
    ns = sum(nnz(results["stencil"]))
    assert 0 < ns < sum(na), (ns, sum(na))


def restate_all(c):
    R, H, L = c["R"], c["H"], c["L"]
    a, b = c["a"], c["b"]
    out = dict(common=intersect(R, L, H, a, b), combined=append_rows(R, R, L, H, a, b),
               stencil=mask_columns(R, L, H, a[0], a[1], c["allowed"]))
    for tag, grp in (("plain", None), ("group", c["locus_group"])):
        for lvl, ign in (("allele", False), ("locus", True)):
            keep = unique_rows(R, L, H, a[0], a[1], grp, ign)
            out[f"keep_{tag}_{lvl}"] = keep
            out[f"uniq_{tag}_{lvl}"] = keep_rows(R, L, H, a[0], a[1], keep)
    return out
