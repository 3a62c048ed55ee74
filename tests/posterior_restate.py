"""Closed-form numpy restatement of the read-level posterior of the EMASE multiread models 1-4: the f and D_r of
em_models_restate.ModelsEM.step, returned per stored entry instead of summed over the reads.

For a stored entry (read r, haplotype h, locus l of gene g) the posterior of an E-step that starts from theta is
theta[h, l] * f / D_r; an entry whose theta is 0 has posterior 0 (the reference keeps an explicit zero there in model 4
and drops the entry in models 1-3).  `count` plays no part.
"""
import numpy as np

from em_models_restate import ModelsEM


def masked_structure(L, H, indptr, indices, gtmask=None):
    """(indptr, indices) per haplotype after a `-G` mask: the surviving columns in locus order, the entries of a
    column in the order given."""
    out_ptr, out_idx = [], []
    for h in range(H):
        ptr = np.asarray(indptr[h], dtype=np.int64)
        width = np.diff(ptr)
        keep_col = np.ones(L, dtype=bool) if gtmask is None else np.asarray(gtmask)[h] != 0
        out_idx.append(np.asarray(indices[h])[np.repeat(keep_col, width)].astype(np.uint32))
        out_ptr.append(np.concatenate(([0], np.cumsum(np.where(keep_col, width, 0)))).astype(np.uint32))
    return out_ptr, out_idx


def posterior(em: ModelsEM, theta, model):
    """Per-haplotype list of float64[nnz_h]: the posterior of every stored (masked) entry of `em` in an E-step of
    `model` that starts from theta (H x L), in the order of the masked index arrays."""
    H = em.H
    t_all = theta[em.h, em.l]
    live = t_all > 0
    r, h, l, g = em.r[live], em.h[live], em.l[live], em.g[live]
    t = t_all[live]
    if model == 4:
        D = np.bincount(r, weights=t, minlength=em.R)
        f = np.ones(len(t))
    else:
        Y = np.zeros((em.n_genes, H))
        np.add.at(Y, em.gene, theta.T)
        T = Y.sum(axis=1)
        U = theta.sum(axis=0)
        rg = em._seg(r, g)
        first_rg = np.unique(rg, return_index=True)[1]
        D = np.bincount(r[first_rg], weights=T[g[first_rg]], minlength=em.R)
        if model == 3:
            S = np.bincount(rg, weights=t)
            f = T[g] / S[rg]
        elif model == 2:
            rl = em._seg(r, l)
            V = np.bincount(rl, weights=t)
            first_rl = np.unique(rl, return_index=True)[1]
            W = np.bincount(rg[first_rl], weights=U[l[first_rl]], minlength=rg.max() + 1)
            f = U[l] * T[g] / (V[rl] * W[rg])
        elif model == 1:
            rgh = em._seg(r, g, h)
            X = np.bincount(rgh, weights=t)
            first = np.unique(rgh, return_index=True)[1]
            Z = np.bincount(rg[first], weights=Y[g[first], h[first]], minlength=rg.max() + 1)
            f = Y[g, h] * T[g] / (X[rgh] * Z[rg])
        else:
            raise ValueError(model)
    post = np.zeros(len(t_all))
    post[live] = t * f / D[r]
    # ModelsEM lays the entries out haplotype by haplotype, each in the order of its masked index array
    bounds = np.searchsorted(em.h, np.arange(H + 1))
    return [post[bounds[k]:bounds[k + 1]] for k in range(H)]
