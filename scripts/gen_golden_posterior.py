#!/usr/bin/env python3
"""Generate tests/golden/posterior_<case>.npz: the read-level posteriors the imported reference holds in
probability.data[h] after the last E-step of EMfactory.run's loop, multiread models 1-4.

Build container only, like scripts/gen_golden_models.py, whose cases (make_case), reference driver (ref_factory) and
elementwise-divide proxy for models 1-3 it reuses; no test, smoke() or bench.py calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_posterior.py

The inputs of a case are those of tests/golden/emmodel_m1_<case>.npz (asserted equal); the fixture holds, per model k,
    m{k}_theta_before   theta (H x L) before the last step: the theta whose E-step the posteriors belong to
    m{k}_post{h}        float64[nnz_h] lined up with the masked indices of haplotype h (tests/posterior_restate.py:
                        masked_structure), each value taken from the reference's matrix by (row, column)
    m{k}_num_iters      steps of the run
and for model 4 also m4_theta_final and m4_expected_counts.  Asserted on the way: the reference's stored structure is
the masked input structure, reference and closed form (tests/posterior_restate.py) agree to 1e-12, and the stopping
iteration of model 4 is not a near miss.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden_models as gm  # noqa: E402  (sets the import paths, loads the reference and the divide proxy)
from em_models_restate import ModelsEM, fixture_inputs  # noqa: E402
from posterior_restate import masked_structure, posterior  # noqa: E402

CASES = ("h8_len", "h2_count", "h16_len_count", "h1_len", "h8_mask", "h4_pseudo_values", "h8_maxiter", "h8_called")


def write_case(name, c, pseudocount=0.0, tol=1e-4, max_iters=200):
    R, H, L = c["R"], c["H"], c["L"]
    case_dir = os.path.join(gm.WORK, "post_" + name)
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

    # the regenerated inputs are the stored fixture's
    with np.load(os.path.join(gm.GOLD, f"emmodel_m1_{name}.npz")) as g:
        fR, fL, fH, f_ptr, f_idx, f_count, f_len, f_groups, f_mask, f_values = fixture_inputs(g)
        assert (fR, fL, fH) == (R, L, H)
        assert float(g["pseudocount"]) == pseudocount and float(g["tol"]) == tol and int(g["max_iters"]) == max_iters
        for h in range(H):
            assert np.array_equal(f_ptr[h], c["indptr"][h]) and np.array_equal(f_idx[h], c["indices"][h])
            assert (f_values is None) == (c["values"] is None)
            if f_values is not None:
                assert np.array_equal(f_values[h], c["values"][h])
        for a, b in ((f_count, c["count"]), (f_len, c["eff_len"]), (f_mask, c["gtmask"])):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
        assert [list(map(int, m)) for m in f_groups] == [list(m) for m in c["groups"]]

    cpu = ModelsEM(R, L, H, c["indptr"], c["indices"], c["count"], c["eff_len"], c["groups"], c["gtmask"])
    m_ptr, m_idx = masked_structure(L, H, c["indptr"], c["indices"], c["gtmask"])
    out = {}
    smallest = np.inf
    for model in (1, 2, 3, 4):
        em = gm.ref_factory(c, grpfile, lenfile, pseudocount)
        np.seterr(all='raise', under='ignore')
        hist, target, err_sum = [], 1000000.0 * tol, 1000000.0
        theta_before = None
        while err_sum > target and len(hist) < max_iters:        # the loop of EMfactory.run
            theta_before = em.allelic_expression.copy()
            prev = em.get_allelic_expression().sum(axis=0)
            prev *= 1000000.0 / prev.sum()
            em.update_allelic_expression(model=model)
            curr = em.get_allelic_expression().sum(axis=0)
            curr *= 1000000.0 / curr.sum()
            err_sum = np.abs(curr - prev).sum()
            hist.append(err_sum)
        np.seterr(all='warn')
        assert theta_before is not None
        if model == 4 and len(hist) < max_iters:                 # not a near miss (gen_golden_models.py:188-189)
            assert hist[-1] < target * (1 - 1e-6) and (len(hist) < 2 or hist[-2] > target * (1 + 1e-6)), (name, model)
        closed = posterior(cpu, theta_before, model)
        out[f"m{model}_theta_before"] = theta_before
        out[f"m{model}_num_iters"] = len(hist)
        for h in range(H):
            mat = em.probability.data[h].tocsc()
            mat.sort_indices()
            ptr = m_ptr[h].astype(np.int64)
            col = np.repeat(np.arange(L), np.diff(ptr))
            row = m_idx[h].astype(np.int64)
            # the stored structure is the masked input structure
            order = np.lexsort((row, col))
            assert np.array_equal(mat.indptr.astype(np.int64), ptr), (name, model, h)
            assert np.array_equal(mat.indices.astype(np.int64), row[order]), (name, model, h)
            post = np.empty(len(row))
            post[order] = mat.data                               # by (row, column)
            d = np.abs(post - closed[h]) / np.maximum(np.abs(closed[h]), 1e-300)
            assert len(d) == 0 or d.max() < 1e-12, (name, model, h, d.max())
            if (post > 0).any():
                smallest = min(smallest, post[post > 0].min())
            out[f"m{model}_post{h}"] = post
        if model == 4:
            out["m4_theta_final"] = em.allelic_expression.copy()
            out["m4_expected_counts"] = np.asarray(em.probability.sum(axis=gm.RefAPM.Axis.READ))
    path = os.path.join(gm.GOLD, f"posterior_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"posterior_{name}: R={R} H={H} L={L} iters={[int(out[f'm{k}_num_iters']) for k in (1, 2, 3, 4)]} "
          f"smallest posterior {smallest:.3g} size={os.path.getsize(path)} B")


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    cases = {
        "h8_len": (lambda: gm.make_case(1500, 8, 90, 20, 101, with_len=True), {}),
        "h2_count": (lambda: gm.make_case(1200, 2, 60, 14, 102, with_count=True), {}),
        "h16_len_count": (lambda: gm.make_case(600, 16, 40, 9, 103, with_count=True, with_len=True), {}),
        "h1_len": (lambda: gm.make_case(800, 1, 50, 12, 104, with_len=True), {}),
        "h8_mask": (lambda: gm.make_case(1500, 8, 90, 20, 105, mask=True, with_len=True), {}),
        "h4_pseudo_values": (lambda: gm.make_case(1000, 4, 70, 16, 106, with_values=True), dict(pseudocount=0.5)),
        "h8_maxiter": (lambda: gm.make_case(1500, 8, 90, 20, 107, with_count=True), dict(tol=0.0, max_iters=7)),
        "h8_called": (lambda: gm.make_case(1500, 8, 90, 20, 108, mask="called", with_len=True), {}),
    }
    for name in CASES:
        if only in (None, name):
            make, kw = cases[name]
            write_case(name, make(), **kw)


if __name__ == "__main__":
    main()
