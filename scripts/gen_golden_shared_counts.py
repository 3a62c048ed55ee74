#!/usr/bin/env python3
"""Generate tests/golden/sharedreads_<case>.npz by running the imported reference.

Build container only (the reference's sources and scipy are not on the GPU machines); no test, smoke() or bench.py
calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_shared_counts.py

Per case (tests/shared_counts_restate.py:make_case) the reference's own `get_num_shared_multireads`
(emase/emase_utils.py:142-146) runs on the matrix as loaded and again after `_bundle_inline(reset=True)`, as
`count_shared_multireads_pairwise` does (:166-173).  Each result must equal the numpy restatement exactly - the same
stored positions, the same counts, no stored zero - and the case must not be vacuous
(shared_counts_restate.check_not_vacuous).  The reference is imported with empty stand-ins for the modules its other
commands need (`tables`, `pysam`, `Bio`).  The fixtures hold plain arrays only, in the smallest integer types that fit.
"""
import os
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF_SRC)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

WORK = tempfile.mkdtemp(prefix="gbrs_golden_shared_")
os.environ["GBRS_DATA"] = WORK


def _stand_in(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules.setdefault(name, mod)
    return sys.modules[name]


_stand_in("tables")
_stand_in("pysam")
bio = _stand_in("Bio")
bio.SeqIO = _stand_in("Bio.SeqIO")
_stand_in("Bio.Seq", Seq=object)
_stand_in("Bio.SeqRecord", SeqRecord=object)

from gbrs.emase.AlignmentPropertyMatrix import AlignmentPropertyMatrix as RefAPM  # noqa: E402
from gbrs.emase.emase_utils import get_num_shared_multireads  # noqa: E402

import shared_counts_restate as rs  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


def ref_apm(c, grpfile):
    R, H, L = c["R"], c["H"], c["L"]
    apm = RefAPM(shape=(L, H, R), haplotype_names=[chr(65 + h) for h in range(H)],
                 locus_names=[f"T{l:05d}" for l in range(L)], grpfile=grpfile)
    ip, ix = c["a"]
    for h in range(H):
        apm.data[h] = sp.csc_matrix((np.ones(len(ix[h])), ix[h].astype(np.int64), ip[h].astype(np.int64)), shape=(R, L))
    apm.finalized = True
    return apm


def as_sorted_csr(m, name):
    """(indptr, indices, data) of the reference's result with the column ids of every row put in ascending order."""
    assert sp.issparse(m) and m.dtype == np.float64, (name, type(m), m.dtype)
    m = sp.csr_matrix(m)
    m.sort_indices()
    assert (m.data != 0).all() and (m.data == np.round(m.data)).all(), (name, "stored zero or fraction")
    assert (abs(m - m.T)).nnz == 0, (name, "not symmetric")
    return m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data.astype(np.int64)


def smallest(a):
    a = np.asarray(a)
    for t in (np.uint8, np.uint16, np.uint32):
        if a.size == 0 or (a.min() >= 0 and a.max() <= np.iinfo(t).max):
            return a.astype(t)
    return a.astype(np.int64)


def write_case(name, R, H, L, seed):
    c = rs.make_case(R, H, L, seed)
    want = rs.restate_both(c)
    rs.check_not_vacuous(c, want)
    grpfile = os.path.join(WORK, f"{name}.g2t.tsv")
    with open(grpfile, "w") as fh:
        for g, members in enumerate(c["groups"]):
            fh.write(f"G{g:05d}\t" + "\t".join(f"T{l:05d}" for l in members) + "\n")
    aln_mat = ref_apm(c, grpfile)
    got = dict(isoform=as_sorted_csr(get_num_shared_multireads(aln_mat), "isoform"))
    assert got["isoform"][0].shape == (L + 1,)
    aln_mat._bundle_inline(reset=True)                             # emase_utils.py:169
    got["gene"] = as_sorted_csr(get_num_shared_multireads(aln_mat), "gene")
    assert got["gene"][0].shape == (len(c["groups"]) + 1,)
    out = dict(num_rows=R, num_haps=H, num_loci=L, num_groups=len(c["groups"]),
               locus_group=c["locus_group"].astype(np.int8 if len(c["groups"]) < 128 else np.int16),
               a_indptr=smallest(np.stack(c["a"][0])), a_indices=smallest(np.concatenate(c["a"][1])))
    for level in ("isoform", "gene"):
        for k, part in enumerate(("indptr", "indices", "data")):
            assert np.array_equal(got[level][k], want[level][k]), (name, level, part)
            out[f"{level}_{part}"] = smallest(got[level][k])
    path = os.path.join(GOLD, f"sharedreads_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"sharedreads_{name}: R={R} H={H} L={L} G={len(c['groups'])} entries={sum(len(i) for i in c['a'][1])} "
          f"nnz isoform/gene={len(got['isoform'][1])}/{len(got['gene'][1])} "
          f"max count off the diagonal={[int(rs.dense(*want[v]).__sub__(np.diag(np.diag(rs.dense(*want[v])))).max()) for v in want]} "
          f"size={os.path.getsize(path)} B")


def main():
    os.makedirs(GOLD, exist_ok=True)
    for name, R, H, L, seed in (("h1", 900, 1, 60, 11), ("h8", 700, 8, 48, 12), ("h16", 500, 16, 36, 13)):
        write_case(name, R, H, L, seed)


if __name__ == "__main__":
    main()
