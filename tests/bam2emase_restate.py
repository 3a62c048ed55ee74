"""What `gbrs bam2emase` computes (emase/AlignmentMatrixFactory.py:26-142), restated over the arrays a test gave
to the BAM writer: sorted(set(names)) for the read ids, the whole-word flag test, split at the delimiter,
coo_matrix(...).tocsc() per haplotype.  Raises what the reference's dict lookups / unpacking raise."""
import numpy as np
from scipy.sparse import coo_matrix


def restate(ref_names, names, refids, flags, haplotypes, loci, delim='_'):
    """-> dict(shape=(L, H, R), hname, lname, rname (list of str), indptr[h], indices[h])."""
    hname = list(haplotypes) if len(haplotypes) else ['h0']
    rname = sorted(set(names))
    rid = {n: k for k, n in enumerate(rname)}
    lid = {n: k for k, n in enumerate(loci)}
    ent = {h: ([], []) for h in hname}
    for n, r, f in zip(names, refids, flags):
        if f != 4 and f != 8:
            if r < 0:
                raise KeyError('record without a reference sequence')
            if len(haplotypes):
                locus, hap = ref_names[r].split(delim)
            else:
                locus, hap = ref_names[r], hname[0]
            ent[hap][0].append(rid[n])
            ent[hap][1].append(lid[locus])
    out = dict(shape=(len(loci), len(hname), len(rname)), hname=hname, lname=list(loci), rname=rname, indptr=[], indices=[])
    for h in hname:
        m = coo_matrix((np.ones(len(ent[h][0])), (np.array(ent[h][0], dtype=np.int64), np.array(ent[h][1], dtype=np.int64))),
                       shape=(len(rname), len(loci))).tocsc()
        out['indptr'].append(m.indptr.astype(np.uint32))
        out['indices'].append(m.indices.astype(np.uint32))
    return out
