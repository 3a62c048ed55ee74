#!/usr/bin/env python3
"""Generate tests/golden/matops_<case>.npz by running the imported reference.

Build container only (the reference's sources and scipy are not on the GPU machines); no test, smoke() or bench.py
calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_matops.py

Per case (tests/matops_restate.py:make_case) the reference computes `A * B` (get-common-alignments), `A.combine(B)`,
`get_unique_reads` for both values of ignore_haplotype, the `bundle(reset=True)` -> `get_unique_reads` ->
`pull_alignments_from` chain of pull_out_unique_reads with a group file, and - `stencil` has no runnable reference -
`multiply(gtmask, axis=2)` + `eliminate_zeros()` with the mask built as quantify builds it
(gbrs/emase_utils.py:260-273).  Every result must have its row ids ascending inside every column as scipy returned it
(nothing is sorted here) and must equal the numpy restatement exactly; the fixtures must not be vacuous
(matops_restate.check_not_vacuous).  Index arrays are stored as uint16 to keep the files at tens of kilobytes.
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

WORK = tempfile.mkdtemp(prefix="gbrs_golden_matops_")
os.environ["GBRS_DATA"] = WORK
sys.modules.setdefault("tables", types.ModuleType("tables"))

from gbrs.emase.AlignmentPropertyMatrix import AlignmentPropertyMatrix as RefAPM  # noqa: E402

import matops_restate as rs  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


def ref_apm(c, m, R, grpfile=None):
    H, L = c["H"], c["L"]
    apm = RefAPM(shape=(L, H, R), haplotype_names=[chr(65 + h) for h in range(H)],
                 locus_names=[f"T{l:05d}" for l in range(L)], grpfile=grpfile)
    for h in range(H):
        apm.data[h] = sp.csc_matrix((np.ones(len(m[1][h])), m[1][h].astype(np.int64), m[0][h].astype(np.int64)),
                                    shape=(R, L))
    apm.finalized = True
    apm.rname = np.array([f"r{k}" for k in range(R)])
    return apm


def structure(apm, name):
    """(indptr list, indices list) exactly as scipy holds them: CSC, no explicit zeros, ascending columns."""
    ip, ix = [], []
    for h, d in enumerate(apm.data):
        assert sp.isspmatrix_csc(d), (name, h, type(d))
        assert (d.data != 0).all(), (name, h, "explicit zeros left")
        for l in np.flatnonzero(np.diff(d.indptr) > 1):
            col = d.indices[d.indptr[l]:d.indptr[l + 1]]
            assert (np.diff(col) > 0).all(), (name, h, l, "column not ascending")
        ip.append(d.indptr.astype(np.uint32))
        ix.append(d.indices.astype(np.uint32))
    return ip, ix


def same(got, want, name):
    for h in range(len(want[0])):
        assert np.array_equal(got[0][h], want[0][h]), (name, h, "indptr")
        assert np.array_equal(got[1][h], want[1][h]), (name, h, "indices")


def write_case(name, R, H, L, seed):
    c = rs.make_case(R, H, L, seed)
    want = rs.restate_all(c)
    rs.check_not_vacuous(c, want)
    grpfile = os.path.join(WORK, f"{name}.g2t.tsv")
    with open(grpfile, "w") as fh:
        for g, members in enumerate(c["groups"]):
            fh.write(f"G{g:05d}\t" + "\t".join(f"T{l:05d}" for l in members) + "\n")
    A, B = ref_apm(c, c["a"], R), ref_apm(c, c["b"], R)
    got = dict(common=structure(A * B, "common"), combined=structure(A.combine(B), "combined"))
    assert A.combine(B).shape == (L, H, 2 * R)
    for lvl, ign in (("allele", False), ("locus", True)):
        got[f"uniq_plain_{lvl}"] = structure(ref_apm(c, c["a"], R).get_unique_reads(ignore_haplotype=ign), lvl)
        # emase_utils.py:297-308
        aln_mat = ref_apm(c, c["a"], R, grpfile=grpfile)
        aln_mat_g = aln_mat.bundle(reset=True, shallow=False)
        aln_mat_g_uniq = aln_mat_g.get_unique_reads(ignore_haplotype=ign, shallow=False)
        num_alns_per_read = aln_mat_g_uniq.sum(axis=RefAPM.Axis.LOCUS).sum(axis=RefAPM.Axis.HAPLOTYPE)
        used = np.asarray(num_alns_per_read > 0).ravel()
        assert np.array_equal(used, want[f"keep_group_{lvl}"]), (name, lvl, "kept reads with groups")
        got[f"uniq_group_{lvl}"] = structure(aln_mat.pull_alignments_from(used, shallow=False), "group " + lvl)
    gtmask = np.zeros((H, L))
    for members, call in zip(c["groups"], c["calls"]):          # gbrs/emase_utils.py:262-268
        gtmask[tuple(np.meshgrid(np.array(call), np.array(members)))] = 1.0
    S = ref_apm(c, c["a"], R)
    S.multiply(gtmask, axis=2)
    for h in range(H):
        S.data[h].eliminate_zeros()
    got["stencil"] = structure(S, "stencil")
    for key, m in got.items():
        same(want[key], m, f"{name}:{key}")
    small = np.uint16
    assert 2 * R < 65536 and L < 65536
    out = dict(num_rows=R, num_haps=H, num_loci=L, locus_group=c["locus_group"], allowed=c["allowed"],
               calls=np.asarray(c["calls"], dtype=np.int32),
               group_ptr=np.concatenate(([0], np.cumsum([len(g) for g in c["groups"]]))).astype(np.int64),
               group_members=np.concatenate([np.asarray(g, dtype=np.int64) for g in c["groups"]]))
    for key in ("keep_plain_allele", "keep_plain_locus", "keep_group_allele", "keep_group_locus"):
        out[key] = np.packbits(want[key])
    for key, m in dict(a=c["a"], b=c["b"], **got).items():
        # one member per matrix and kind (a zip member costs more than these arrays): indptr (H x (L + 1)), the
        # haplotypes' indices one after another (split by indptr[:, -1])
        out[f"{key}_indptr"] = np.stack([m[0][h] for h in range(H)]).astype(small)
        out[f"{key}_indices"] = np.concatenate([m[1][h] for h in range(H)]).astype(small)
    path = os.path.join(GOLD, f"matops_{name}.npz")
    np.savez_compressed(path, **out)
    kept = {k: int(want[k].sum()) for k in want if k.startswith("keep_")}
    print(f"matops_{name}: R={R} H={H} L={L} nnz a/b/common={sum(rs.nnz(c['a']))}/{sum(rs.nnz(c['b']))}/"
          f"{sum(rs.nnz(got['common']))} kept={kept} stencil={sum(rs.nnz(got['stencil']))} "
          f"size={os.path.getsize(path)} B")


def main():
    os.makedirs(GOLD, exist_ok=True)
    for name, R, H, L, seed in (("h8", 400, 8, 40, 1), ("h2", 600, 2, 50, 2), ("h16", 250, 16, 30, 3)):
        write_case(name, R, H, L, seed)


if __name__ == "__main__":
    main()
