"""What `gbrs bam2ec` computes, restated from the two contracts it joins: tests/bam2emase_restate.restate per file
(the `bam2emase` rules), the files' reads one after the other (gbrs/emase_utils.py:46-77 iterates file by file, so
the same name in two files is two reads), then oracle.compress_oracle.compress - pinned to the reference's own
compress() by tests/golden/compress_*.npz - over the stacked rows.  Nothing here touches the code under test."""
import numpy as np

from bam2emase_restate import restate
from oracle.compress_oracle import compress


def restate_classes(files, haplotypes, loci, delim='_'):
    """files: one dict(ref_names, names, refids, flags) per BAM file, in the order they are given.
    -> dict(shape=(L, H, max(num_ecs, 1)), hname, lname, indptr[h], indices[h], count, num_reads, num_ecs)."""
    hname = list(haplotypes) if len(haplotypes) else ['h0']
    L, H = len(loci), len(hname)
    rows, cols = [[] for _ in range(H)], [[] for _ in range(H)]
    off = 0
    for f in files:
        one = restate(f['ref_names'], f['names'], f['refids'], f['flags'], haplotypes, loci, delim)
        for h in range(H):
            ptr = one['indptr'][h].astype(np.int64)
            cols[h].append(np.repeat(np.arange(L, dtype=np.int64), np.diff(ptr)))
            rows[h].append(one['indices'][h].astype(np.int64) + off)            # later files' rows follow
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
