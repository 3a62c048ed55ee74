"""What `gbrs bam2ec --mate-file` computes, restated from the contracts it joins: tests/bam2emase_restate.restate on
each end of a pair (the `bam2emase` rules), the reference's test on the two name arrays (emase/emase_utils.py:262),
the (column, read) sets of the two ends intersected per haplotype (the reference's `A * B` on incidence matrices),
the items' reads one after the other, then oracle.compress_oracle.compress over the stacked rows.  Also the
second-end generator of the GPU tests.  Nothing here touches the code under test."""
import numpy as np

from bam2emase_restate import restate
from oracle.compress_oracle import compress


def common_entries(L, R, a, b):
    """a, b: (indptr, indices) of one haplotype's CSC matrix (R reads x L loci) -> (indptr, indices) of the entries
    both have, read ids ascending inside a column."""
    keys = []
    for ip, ix in (a, b):
        col = np.repeat(np.arange(L, dtype=np.int64), np.diff(np.asarray(ip).astype(np.int64)))
        keys.append(col * max(R, 1) + np.asarray(ix).astype(np.int64))
    both = np.intersect1d(keys[0], keys[1])                 # sorted: by column, then by read
    return (np.searchsorted(both // max(R, 1), np.arange(L + 1)).astype(np.uint32), (both % max(R, 1)).astype(np.uint32))


def restate_pair(first, second, haplotypes, loci, delim='_'):
    """Both ends restated, their names compared, their entries intersected -> the dict of restate()."""
    a = restate(first['ref_names'], first['names'], first['refids'], first['flags'], haplotypes, loci, delim)
    b = restate(second['ref_names'], second['names'], second['refids'], second['flags'], haplotypes, loci, delim)
    if a['rname'] != b['rname']:
        raise ValueError("The read ID's are not compatible.")
    L, H, R = a['shape']
    out = dict(a, indptr=[], indices=[])
    for h in range(H):
        ip, ix = common_entries(L, R, (a['indptr'][h], a['indices'][h]), (b['indptr'][h], b['indices'][h]))
        out['indptr'].append(ip)
        out['indices'].append(ix)
    return out


def restate_classes(items, haplotypes, loci, delim='_'):
    """items: a dict(ref_names, names, refids, flags) for a single-end file or a (first, second) tuple of two for a
    pair, in the order they are given.
    -> dict(shape=(L, H, max(num_ecs, 1)), hname, lname, indptr[h], indices[h], count, num_reads, num_ecs)."""
    hname = list(haplotypes) if len(haplotypes) else ['h0']
    L, H = len(loci), len(hname)
    rows, cols = [[] for _ in range(H)], [[] for _ in range(H)]
    off = 0
    for f in items:
        if isinstance(f, tuple):
            one = restate_pair(f[0], f[1], haplotypes, loci, delim)
        else:
            one = restate(f['ref_names'], f['names'], f['refids'], f['flags'], haplotypes, loci, delim)
        for h in range(H):
            ptr = one['indptr'][h].astype(np.int64)
            cols[h].append(np.repeat(np.arange(L, dtype=np.int64), np.diff(ptr)))
            rows[h].append(one['indices'][h].astype(np.int64) + off)            # later items' rows follow
        off += one['shape'][2]
    indptr, indices = [], []
    for h in range(H):
        r, c = np.concatenate(rows[h]), np.concatenate(cols[h])
        order = np.lexsort((r, c))
        indices.append(r[order].astype(np.uint32))
        indptr.append(np.searchsorted(c[order], np.arange(L + 1)).astype(np.uint32))
    n, ip, ix, counts = compress(off, L, H, indptr, indices)
    return dict(shape=(L, H, max(n, 1)), hname=hname, lname=list(loci), indptr=ip, indices=ix,
                count=counts if n else np.zeros(1), num_reads=off, num_ecs=n)


def entry_counts(first, second, haplotypes, loci):
    """(entries of the first end, of the second end, common ones, reads with entries in both ends and none in
    common): what a test checks before it trusts a pair to exercise anything."""
    a = restate(first['ref_names'], first['names'], first['refids'], first['flags'], haplotypes, loci)
    b = restate(second['ref_names'], second['names'], second['refids'], second['flags'], haplotypes, loci)
    c = restate_pair(first, second, haplotypes, loci)
    R = a['shape'][2]
    has = [np.zeros(R, dtype=bool) for _ in range(3)]
    for k, m in enumerate((a, b, c)):
        for ix in m['indices']:
            has[k][ix] = True
    n = [sum(len(ix) for ix in m['indices']) for m in (a, b, c)]
    return n[0], n[1], n[2], int((has[0] & has[1] & ~has[2]).sum())


def second_end(case, seed):
    """The second end of a make_case case of tests/test_bam2ec_gpu.py: the same read names; per read every distinct
    kept reference sequence survives with p = 0.7, one more usable sequence is added with p = 0.3, and with p = 0.1 -
    or when nothing survived - the read is unaligned in this end (a single flag-4 record).  Reads in shuffled order,
    records in shuffled order within a read."""
    rng = np.random.default_rng([seed, 2])
    n_usable = len(case['ref_names']) - 3
    kept = {}
    for nm, r, f in zip(case['names'], case['refids'], case['flags']):
        refs = kept.setdefault(nm, [])
        if f != 4 and f != 8 and r not in refs:
            refs.append(r)
    names, refids, flags = [], [], []
    reads = list(kept)
    for k in rng.permutation(len(reads)).tolist():
        nm = reads[k]
        mine = [r for r in kept[nm] if rng.random() < 0.7]
        if rng.random() < 0.3:
            extra = int(rng.integers(0, n_usable))
            if extra not in mine:
                mine.append(extra)
        if rng.random() < 0.1 or not mine:
            names.append(nm); refids.append(-1); flags.append(4)
            continue
        for j, r in enumerate(rng.permutation(mine).tolist()):
            names.append(nm); refids.append(int(r)); flags.append(0 if j == 0 else 256)
    return dict(case, names=names, refids=refids, flags=flags)
