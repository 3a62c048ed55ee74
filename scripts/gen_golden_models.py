#!/usr/bin/env python3
"""Generate tests/golden/emmodel_m<k>_<case>.npz (multiread models 1, 2, 3) by running the imported reference.

Build container only (the reference's sources are not on the GPU machines); no test, smoke() or bench.py calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_models.py

The reference does not run models 1-3 as it stands: normalize_reads for the LOCUS, GROUP and HAPLOGROUP axes
(emase/AlignmentPropertyMatrix.py:316-366) divides with np.divide(sparse, sparse), which scipy answers with a dense
numpy.matrix, and the next sparse call on it fails.  Every division there is meant elementwise on the stored entries
of the numerator, so this script replaces the `np` name inside that one module with a proxy whose divide() does
exactly that for two sparse arguments (everything else is numpy's), runs the reference's EMfactory unmodified
otherwise, and asserts that it agrees with the closed-form restatement of tests/em_models_restate.py to 1e-12.
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

WORK = tempfile.mkdtemp(prefix="gbrs_golden_models_")
os.environ["GBRS_DATA"] = WORK
sys.modules.setdefault("tables", types.ModuleType("tables"))

import gbrs.emase.AlignmentPropertyMatrix as ref_apm_mod  # noqa: E402
from gbrs.emase.AlignmentPropertyMatrix import AlignmentPropertyMatrix as RefAPM  # noqa: E402
from gbrs.emase.EMfactory import EMfactory as RefEM  # noqa: E402

from em_models_restate import ModelsEM  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SNAP_ITERS = (1, 2, 5)


class _NumpyWithElementwiseSparseDivide:
    """numpy, except that divide(sparse, sparse) divides the stored entries of the numerator."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def divide(a, b, *args, **kw):
        if sp.issparse(a) and sp.issparse(b) and not args and not kw:
            return a.tocsc().astype(np.float64)._binopt(b.tocsc(), '_eldiv_')
        return np.divide(a, b, *args, **kw)


ref_apm_mod.np = _NumpyWithElementwiseSparseDivide()


def make_case(R, H, L, n_groups, seed, with_count=False, with_len=False, mask=False, with_values=False):
    """Reads of 1-3 loci drawn across the whole locus range (so they cross genes), every locus of a read with its own
    haplotype mask; genes of 1-4 consecutive loci, the last loci in no group.  mask: a called pair of haplotypes per gene
    and per ungrouped locus; mask="called": per gene only, so that the loci in no group keep nothing (what a genotype file
    for `gbrs quantify -G` gives them, since it can only call genes)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 5, size=n_groups)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    assert sizes.sum() < L, "some loci must stay ungrouped"
    groups = [list(range(int(s), int(s + n))) for s, n in zip(starts, sizes)]
    pop = rng.lognormal(0.0, 1.5, size=L)
    pop /= pop.sum()
    cols = [[] for _ in range(H)]            # (locus, row) per haplotype
    for r in range(R):
        k = int(rng.integers(1, 4))
        loci = np.unique(rng.choice(L, size=k, p=pop))
        for l in loci:
            m = rng.random(H) < 0.6
            if not m.any():
                m[rng.integers(0, H)] = True
            for h in np.flatnonzero(m):
                cols[h].append((int(l), r))
    indptr, indices = [], []
    for h in range(H):
        a = np.array(sorted(cols[h]), dtype=np.int64).reshape(-1, 2)
        indptr.append(np.searchsorted(a[:, 0], np.arange(L + 1)).astype(np.uint32))
        indices.append(a[:, 1].astype(np.uint32))
    count = rng.integers(1, 6, size=R).astype(np.float64) if with_count else None
    raw_len = np.round(rng.lognormal(6.5, 0.5, size=L))
    eff_len = np.maximum(raw_len - 100 + 1, 1.0)[None, :].repeat(H, 0) if with_len else None
    gtmask = None
    if mask:
        gtmask = np.zeros((H, L))
        gene_sets = groups + ([] if mask == "called" else [[l] for l in range(int(sizes.sum()), L)])
        for members in gene_sets:
            a, b = rng.integers(0, H, size=2)
            gtmask[np.ix_([a, b], members)] = 1.0
    values = [rng.random(len(ix)) + 0.25 for ix in indices] if with_values else None
    return dict(R=R, H=H, L=L, indptr=indptr, indices=indices, count=count, raw_len=raw_len, eff_len=eff_len,
                groups=groups, gtmask=gtmask, values=values)


def ref_factory(c, grpfile, lenfile, pseudocount):
    R, H, L = c["R"], c["H"], c["L"]
    apm = RefAPM(shape=(L, H, R), haplotype_names=[chr(65 + h) for h in range(H)],
                 locus_names=[f"T{l:07d}" for l in range(L)], grpfile=grpfile)
    for h in range(H):
        v = np.ones(len(c["indices"][h])) if c["values"] is None else c["values"][h].copy()
        apm.data[h] = sp.csc_matrix((v, c["indices"][h].astype(np.int64), c["indptr"][h].astype(np.int64)),
                                    shape=(R, L))
    apm.finalized = True
    if c["count"] is not None:
        apm.count = c["count"].copy()
    if c["gtmask"] is not None:
        apm.multiply(c["gtmask"], axis=2)
        for h in range(H):
            apm.data[h].eliminate_zeros()
    em = RefEM(apm)
    em.prepare(pseudocount=pseudocount, lenfile=lenfile)
    return em


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def write_case(name, c, pseudocount=0.0, tol=1e-4, max_iters=200):
    R, H, L = c["R"], c["H"], c["L"]
    case_dir = os.path.join(WORK, name)
    os.makedirs(case_dir)
    grpfile = os.path.join(case_dir, "g2t.tsv")
    with open(grpfile, "w") as fh:
        for i, members in enumerate(c["groups"]):
            fh.write(f"G{i:07d}\t" + "\t".join(f"T{l:07d}" for l in members) + "\n")
    lenfile = None
    if c["eff_len"] is not None:
        lenfile = os.path.join(case_dir, "lengths.info")
        with open(lenfile, "w") as fh:
            for l in range(L):
                for h in range(H):
                    fh.write(f"T{l:07d}_{chr(65 + h)}\t{int(c['raw_len'][l])}\n" if H > 1 else
                             f"T{l:07d}\t{int(c['raw_len'][l])}\n")
    cpu = ModelsEM(R, L, H, c["indptr"], c["indices"], c["count"], c["eff_len"], c["groups"], c["gtmask"])

    # the four models separate after one step on every case
    theta0 = ref_factory(c, grpfile, lenfile, pseudocount).allelic_expression.copy()
    # (with one haplotype X = S and V = U, so models 1, 2 and 3 coincide there: that case only separates them from 4)
    one = {m: cpu.step(theta0, m)[0] for m in (1, 2, 3, 4)}
    for a in (1, 2, 3, 4):
        for b in range(a + 1, 5):
            if H > 1 or b == 4:
                assert rel(one[a], one[b]) > 1e-3, f"{name}: models {a} and {b} agree after one step"

    for model in (1, 2, 3):
        em = ref_factory(c, grpfile, lenfile, pseudocount)
        assert np.array_equal(em.allelic_expression, theta0)
        out = dict(theta0=theta0.copy(), model=model)
        # the loop of EMfactory.run, with the snapshots taken on the way
        np.seterr(all='raise', under='ignore')
        hist, snaps, target = [], {}, 1000000.0 * tol
        err_sum = 1000000.0
        while err_sum > target and len(hist) < max_iters:
            prev = em.get_allelic_expression().sum(axis=0)
            prev *= 1000000.0 / prev.sum()
            em.update_allelic_expression(model=model)
            curr = em.get_allelic_expression().sum(axis=0)
            curr *= 1000000.0 / curr.sum()
            err_sum = np.abs(curr - prev).sum()
            hist.append(err_sum)
            if len(hist) in SNAP_ITERS:
                snaps[len(hist)] = em.allelic_expression.copy()
        np.seterr(all='warn')
        # the same through the reference's own run()
        em_run = ref_factory(c, grpfile, lenfile, pseudocount)
        em_run.run(model=model, tol=tol, max_iters=max_iters, verbose=False)
        np.seterr(all='warn')
        assert np.array_equal(em_run.allelic_expression, em.allelic_expression), f"{name} m{model}: run() differs"

        def on_iter(i, theta):
            if i in snaps:
                assert rel(theta, snaps[i]) < 1e-12, (name, model, i, rel(theta, snaps[i]))
        theta_c, counts_c, hist_c = cpu.run(theta0.copy(), model, tol, max_iters, on_iter=on_iter)
        assert len(hist_c) == len(hist), (name, model, len(hist_c), len(hist))
        assert rel(theta_c, em.allelic_expression) < 1e-12, (name, model)
        ref_counts = np.asarray(em.probability.sum(axis=RefAPM.Axis.READ))
        assert rel(counts_c, ref_counts) < 1e-12
        # the stopping iteration is not a near miss: the restatement and the device must stop at the same step
        if len(hist) < max_iters:
            assert hist[-1] < target * (1 - 1e-6) and (len(hist) < 2 or hist[-2] > target * (1 + 1e-6)), (name, model)
        gene_theta = np.asarray(em.get_allelic_expression(at_group_level=True))
        gene_counts = np.asarray(ref_counts * em.grp_conv_mat)
        texts = {}
        for key, fn in (("isoforms_tpm", lambda p: em.report_depths(filename=p, tpm=True)),
                        ("isoforms_counts", lambda p: em.report_read_counts(filename=p)),
                        ("genes_tpm", lambda p: em.report_depths(filename=p, tpm=True, grp_wise=True)),
                        ("genes_counts", lambda p: em.report_read_counts(filename=p, grp_wise=True))):
            path = os.path.join(case_dir, f"m{model}_{key}")
            fn(path)
            texts[key] = open(path).read()
        out.update(
            num_rows=R, num_loci=L, num_haps=H, pseudocount=pseudocount, tol=tol, max_iters=max_iters,
            has_count=c["count"] is not None, has_len=c["eff_len"] is not None, has_mask=c["gtmask"] is not None,
            count=c["count"] if c["count"] is not None else np.zeros(0),
            eff_len=c["eff_len"] if c["eff_len"] is not None else np.zeros((0, 0)),
            raw_length=c["raw_len"],
            gtmask=c["gtmask"] if c["gtmask"] is not None else np.zeros((0, 0)),
            group_ptr=np.concatenate(([0], np.cumsum([len(g) for g in c["groups"]]))).astype(np.int64),
            group_members=np.concatenate([np.asarray(g, dtype=np.int64) for g in c["groups"]]),
            theta_final=snaps_final(em), expected_counts=ref_counts, gene_theta=gene_theta, gene_counts=gene_counts,
            num_iters=len(hist), err_history=np.asarray(hist),
            **{f"theta_iter{k}": v for k, v in snaps.items()},
            **{f"text_{k}": np.array(v) for k, v in texts.items()},
        )
        for h in range(H):
            out[f"indptr{h}"] = c["indptr"][h]
            out[f"indices{h}"] = c["indices"][h]
            if c["values"] is not None:
                out[f"values{h}"] = c["values"][h]
        path = os.path.join(GOLD, f"emmodel_m{model}_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"emmodel_m{model}_{name}: R={R} H={H} L={L} iters={len(hist)} size={os.path.getsize(path)} B")


_final = {}


def snaps_final(em):
    """theta after the last step, before the TPM report rescaled it in place (EMfactory.py:352-354)."""
    return _final.pop(id(em))


def main():
    os.makedirs(GOLD, exist_ok=True)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    # report_depths(tpm=True) rescales allelic_expression in place: keep the final theta before the reports
    orig = RefEM.report_depths

    def keep_then_report(self, *a, **kw):
        _final.setdefault(id(self), self.allelic_expression.copy())
        return orig(self, *a, **kw)
    RefEM.report_depths = keep_then_report
    cases = [
        ("h8_len", lambda: make_case(1500, 8, 90, 20, 101, with_len=True), {}),
        ("h2_count", lambda: make_case(1200, 2, 60, 14, 102, with_count=True), {}),
        ("h16_len_count", lambda: make_case(600, 16, 40, 9, 103, with_count=True, with_len=True), {}),
        ("h1_len", lambda: make_case(800, 1, 50, 12, 104, with_len=True), {}),
        ("h8_mask", lambda: make_case(1500, 8, 90, 20, 105, mask=True, with_len=True), {}),
        ("h4_pseudo_values", lambda: make_case(1000, 4, 70, 16, 106, with_values=True), dict(pseudocount=0.5)),
        ("h8_maxiter", lambda: make_case(1500, 8, 90, 20, 107, with_count=True), dict(tol=0.0, max_iters=7)),
        ("h8_called", lambda: make_case(1500, 8, 90, 20, 108, mask="called", with_len=True), {}),
    ]
    for name, make, kw in cases:
        if only in (None, name):
            write_case(name, make(), **kw)

if __name__ == "__main__":
    main()
