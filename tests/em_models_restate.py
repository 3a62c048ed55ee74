"""Closed-form numpy restatement of the EMASE multiread models 1-4 (emase/EMfactory.py:160-208) on the stored
entries of the alignment incidence, for the emmodel_*.npz fixtures and the tests that read them.

For a stored entry (read r, haplotype h, locus l of gene g) with theta[h, l] > 0 the posterior is
theta[h, l] * f / D_r (multiread models):
    model 4   f = 1,                              D_r = sum of theta over the read's entries
    model 3   f = T_g / S[r, g]
    model 2   f = U_l T_g / (V[r, l] W[r, g])
    model 1   f = Y[h, g] T_g / (X[r, g, h] Z[r, g])
and for models 1-3 D_r = sum of T_g over the genes the read touches.  Entries whose theta is 0 take no part.
"""
import numpy as np


def fixture_inputs(g):
    """(R, L, H, indptr, indices, count, eff_len, groups, gtmask, values) of an emmodel_*.npz fixture."""
    H, L, R = int(g["num_haps"]), int(g["num_loci"]), int(g["num_rows"])
    indptr = [g[f"indptr{h}"] for h in range(H)]
    indices = [g[f"indices{h}"] for h in range(H)]
    count = g["count"] if bool(g["has_count"]) else None
    eff_len = g["eff_len"] if bool(g["has_len"]) else None
    gp, gm = g["group_ptr"], g["group_members"]
    groups = [list(gm[gp[i]:gp[i + 1]]) for i in range(len(gp) - 1)]
    gtmask = g["gtmask"] if bool(g["has_mask"]) else None
    values = [g[f"values{h}"] for h in range(H)] if "values0" in g else None
    return R, L, H, indptr, indices, count, eff_len, groups, gtmask, values


class ModelsEM:
    """Entries of the (masked) incidence and the EM of the reference's run() loop on them."""

    def __init__(self, R, L, H, indptr, indices, count, eff_len, groups, gtmask=None):
        self.R, self.L, self.H = R, L, H
        rows, haps, locs = [], [], []
        for h in range(H):
            ptr = np.asarray(indptr[h], dtype=np.int64)
            loc = np.repeat(np.arange(L), np.diff(ptr))
            keep = np.ones(len(loc), dtype=bool) if gtmask is None else gtmask[h, loc] != 0
            rows.append(np.asarray(indices[h], dtype=np.int64)[keep])
            locs.append(loc[keep])
            haps.append(np.full(int(keep.sum()), h, dtype=np.int64))
        self.r, self.h, self.l = np.concatenate(rows), np.concatenate(haps), np.concatenate(locs)
        self.count = np.ones(R) if count is None else np.asarray(count, dtype=np.float64)
        self.eff_len = eff_len
        gene = np.full(L, -1, dtype=np.int64)
        for i, members in enumerate(groups):
            gene[np.asarray(members, dtype=np.int64)] = i
        free = np.flatnonzero(gene < 0)
        gene[free] = len(groups) + np.arange(len(free))
        self.gene, self.n_genes = gene, len(groups) + len(free)
        self.g = gene[self.l]

    @staticmethod
    def _seg(*keys):
        """Segment id of every entry for the composite key (dense, 0-based)."""
        k = np.stack(keys, axis=1)
        _, inv = np.unique(k, axis=0, return_inverse=True)
        return inv.ravel()

    def step(self, theta, model):
        """(theta', expected counts) after one step of `model`."""
        H, L = self.H, self.L
        t = theta[self.h, self.l]
        live = t > 0
        r, h, l, g = self.r[live], self.h[live], self.l[live], self.g[live]
        t = t[live]
        if model == 4:
            D = np.bincount(r, weights=t, minlength=self.R)
            f = np.ones(len(t))
        else:
            Y = np.zeros((self.n_genes, H))
            np.add.at(Y, self.gene, theta.T)
            T = Y.sum(axis=1)
            U = theta.sum(axis=0)
            rg = self._seg(r, g)
            first_rg = np.unique(rg, return_index=True)[1]
            D = np.bincount(r[first_rg], weights=T[g[first_rg]], minlength=self.R)
            if model == 3:
                S = np.bincount(rg, weights=t)
                f = T[g] / S[rg]
            elif model == 2:
                rl = self._seg(r, l)
                V = np.bincount(rl, weights=t)
                first_rl = np.unique(rl, return_index=True)[1]
                W = np.bincount(rg[first_rl], weights=U[l[first_rl]], minlength=rg.max() + 1)
                f = U[l] * T[g] / (V[rl] * W[rg])
            elif model == 1:
                rgh = self._seg(r, g, h)
                X = np.bincount(rgh, weights=t)
                first = np.unique(rgh, return_index=True)[1]
                Z = np.bincount(rg[first], weights=Y[g[first], h[first]], minlength=rg.max() + 1)
                f = Y[g, h] * T[g] / (X[rgh] * Z[rg])
            else:
                raise ValueError(model)
        A = np.zeros((H, L))
        np.add.at(A, (h, l), self.count[r] * f / D[r])
        counts = theta * A
        new = counts / self.eff_len if self.eff_len is not None else counts.copy()
        return new, counts

    def run(self, theta, model, tol, max_iters, on_iter=None):
        """The loop of EMfactory.run (EMfactory.py:264-278): (theta, expected counts, err history)."""
        err_sum, target, hist, counts = 1000000.0, 1000000.0 * tol, [], None
        while err_sum > target and len(hist) < max_iters:
            prev = theta.sum(axis=0)
            prev = prev * (1000000.0 / prev.sum())
            theta, counts = self.step(theta, model)
            curr = theta.sum(axis=0)
            curr = curr * (1000000.0 / curr.sum())
            err_sum = np.abs(curr - prev).sum()
            hist.append(err_sum)
            if on_iter is not None:
                on_iter(len(hist), theta)
        return theta, counts, hist

    def group_sums(self, x, groups):
        """(H x G) sums over the members of every group."""
        return np.stack([x[:, np.asarray(m, dtype=np.int64)].sum(axis=1) for m in groups], axis=1)
