"""numpy restatement of `count-shared-multireads-pairwise` (gbrs_amd/matops.py, emase/emase_utils.py:142-176), checked
against the imported reference by scripts/gen_golden_shared_counts.py.  Test infrastructure: numpy alone.

The pattern matrix P is R x n: P[r, c] = 1 when read r has a stored entry at column c in any haplotype.  A column is a
locus (n = L) or, with a locus-to-group map, a gene (n = G; entries of loci in no gene drop out).  The result is
C = P^T P as CSR with both triangles and the column ids ascending inside every row: one distinct (row, column) key per
entry, then every ordered pair of the columns of a row, counted."""
import numpy as np


def pattern_keys(R, L, H, indptr, indices, locus_group=None, num_groups=0):
    """(distinct row * n + column keys, ascending; n)."""
    n = L if locus_group is None else int(num_groups)
    keys = []
    for h in range(H):
        col = np.repeat(np.arange(L, dtype=np.int64), np.diff(np.asarray(indptr[h], dtype=np.int64)))
        row = np.asarray(indices[h], dtype=np.int64)
        if locus_group is not None:
            col = np.asarray(locus_group, dtype=np.int64)[col]
            row, col = row[col >= 0], col[col >= 0]
        keys.append(row * n + col)
    return np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64), n


def shared_counts(R, L, H, indptr, indices, locus_group=None, num_groups=0):
    """(indptr int64[n + 1], indices int64[nnz], data int64[nnz], n)."""
    keys, n = pattern_keys(R, L, H, indptr, indices, locus_group, num_groups)
    row, col = keys // n, keys % n
    length = np.bincount(row, minlength=R)                         # columns per read
    start = np.concatenate(([0], np.cumsum(length)))[:-1]
    per_entry = length[row]                                        # entry k pairs with every entry of its row
    first = np.repeat(np.arange(len(keys), dtype=np.int64), per_entry)
    within = np.arange(int(per_entry.sum()), dtype=np.int64) - np.repeat(np.cumsum(per_entry) - per_entry, per_entry)
    second = np.repeat(start[row], per_entry) + within
    pairs, counts = np.unique(col[first] * n + col[second], return_counts=True)
    ip = np.searchsorted(pairs // n, np.arange(n + 1)).astype(np.int64)
    return ip, (pairs % n).astype(np.int64), counts.astype(np.int64), n


def dense(indptr, indices, data, n):
    out = np.zeros((n, n), dtype=np.int64)
    out[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    return out


def make_case(R, H, L, seed, mean_extra=1.5, empty=0.05, wide=0):
    """A sample in which multi-locus reads are common: a read hits 1 + Poisson(mean_extra) distinct loci inside a
    window of 8 around a random locus (so the same pairs of loci come up again and again), each of them in a random
    non-empty set of haplotypes; an `empty` share of the reads has no entry; with `wide` > 0 read 1 hits that many
    distinct loci all over.  Genes are 1-4 consecutive loci and the last loci are in no gene, as in
    matops_restate.make_case.  Returns R, H, L, a = (indptr list, indices list), groups, locus_group."""
    rng = np.random.default_rng(seed)
    k = 1 + rng.poisson(mean_extra, size=R)
    k[rng.random(R) < empty] = 0
    k[0] = 0                                                       # a row with no entry, whatever the draw
    rows = np.repeat(np.arange(R, dtype=np.int64), k)
    centre = np.repeat(rng.integers(0, L, size=R), k)
    cols = (centre + rng.integers(0, 8, size=len(rows))) % L
    if wide:
        assert R > 1 and wide <= L
        other = rows != 1
        rows = np.concatenate((rows[other], np.full(wide, 1, dtype=np.int64)))
        cols = np.concatenate((cols[other], rng.permutation(L)[:wide]))
    rl = np.unique(rows * L + cols)                                # distinct (read, locus)
    sets = rng.integers(1, 1 << H, size=len(rl))                   # non-empty haplotype set of each
    ip, ix = [], []
    for h in range(H):
        sel = rl[((sets >> h) & 1).astype(bool)]
        order = np.argsort((sel % L) * R + sel // L, kind="stable")
        sel = sel[order]
        ip.append(np.searchsorted(sel % L, np.arange(L + 1)).astype(np.uint32))
        ix.append((sel // L).astype(np.uint32))
    sizes, at = [], 0
    tail = max(2, L // 20)                                         # the last loci stay in no gene
    while at < L - tail:
        s = min(int(rng.integers(1, 5)), L - tail - at)
        sizes.append(s)
        at += s
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    groups = [list(range(int(s), int(s + m))) for s, m in zip(starts, sizes)]
    locus_group = np.full(L, -1, dtype=np.int32)
    for g, members in enumerate(groups):
        locus_group[members] = g
    return dict(R=R, H=H, L=L, a=(ip, ix), groups=groups, locus_group=locus_group)


def restate_both(c):
    """{'isoform': (indptr, indices, data, n), 'gene': ...}"""
    R, H, L = c["R"], c["H"], c["L"]
    return dict(isoform=shared_counts(R, L, H, c["a"][0], c["a"][1]),
                gene=shared_counts(R, L, H, c["a"][0], c["a"][1], c["locus_group"], len(c["groups"])))


def check_not_vacuous(c, results):
    """The conditions every fixture and every generated case must meet."""
    R, H, L = c["R"], c["H"], c["L"]
    for level in ("isoform", "gene"):
        ip, ix, data, n = results[level]
        off = np.repeat(np.arange(n), np.diff(ip)) != ix
        assert int(off.sum()) >= 20, (level, int(off.sum()))
        assert int(np.max(np.asarray(data)[off])) >= 2, level
    keys, _ = pattern_keys(R, L, H, c["a"][0], c["a"][1])
    per_read = np.bincount(keys // L, minlength=R)
    assert per_read.max() >= 4                                     # a read with at least 4 distinct loci
    assert (per_read == 0).any()                                   # a row with no entries
    per_locus = np.bincount(keys % L, minlength=L)
    assert (per_locus[np.asarray(c["locus_group"]) < 0] > 0).any()  # a locus in no group that has entries
