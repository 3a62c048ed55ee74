"""numpy restatement of the alignment tensor's arithmetic (emase/Sparse3DMatrix.py reset / multiply / copy,
emase/AlignmentPropertyMatrix.py normalize_reads / sum), the table of operations the tensor_*.npz fixtures record, and
the driver that runs one of them on anything with the tensor's interface: the reference (scripts/gen_golden_tensor.py),
this restatement (test_tensor_cpu.py) and gbrs_amd.tensor.DeviceTensor (test_tensor_gpu.py).

The entries are kept flat, in the order of the per-haplotype CSC arrays one haplotype after the other.  An entry whose
value is 0 when normalize_reads runs on the LOCUS, GROUP or HAPLOGROUP axis is eliminated (the reference's
eliminate_zeros() drops it from the sparse structure): it keeps 0 from then on, reset() included.
"""
import numpy as np

LOCUS, HAPLOTYPE, READ, GROUP, HAPLOGROUP = range(5)


def locus_genes(L, groups):
    """gene of every locus: the groups in order, then every locus in no group as a gene of its own (the blocks of the
    reference's t2t_mat, EMfactory.py:48-59)."""
    gene = np.full(L, -1, dtype=np.int64)
    for g, members in enumerate(groups or []):
        gene[np.asarray(members, dtype=np.int64)] = g
    free = np.flatnonzero(gene < 0)
    gene[free] = len(groups or []) + np.arange(len(free))
    return gene


class TensorRestate:
    def __init__(self, R, L, H, indptr, indices, values=None, count=None, groups=None):
        self.R, self.L, self.H = R, L, H
        self.sizes = [len(ix) for ix in indices]
        self.off = np.concatenate(([0], np.cumsum(self.sizes))).astype(np.int64)
        self.row = np.concatenate([np.asarray(ix, dtype=np.int64) for ix in indices]) if H else np.zeros(0, np.int64)
        self.loc = np.concatenate([np.repeat(np.arange(L), np.diff(np.asarray(p, dtype=np.int64))) for p in indptr])
        self.hap = np.repeat(np.arange(H), self.sizes)
        self.val = (np.ones(len(self.row)) if values is None
                    else np.concatenate([np.asarray(v, dtype=np.float64) for v in values]))
        self.elim = np.zeros(len(self.row), dtype=bool)
        self.count = None if count is None else np.asarray(count, dtype=np.float64)
        self.groups = groups
        self.gene = locus_genes(L, groups)

    def copy(self):
        c = object.__new__(TensorRestate)
        c.__dict__.update(self.__dict__)
        c.val, c.elim = self.val.copy(), self.elim.copy()
        return c

    def reset(self):
        self.val = np.where(self.elim, 0.0, 1.0)

    def multiply(self, m, axis=None):
        if isinstance(m, TensorRestate):
            f = m.val
        else:
            m = np.asarray(m, dtype=np.float64)
            if m.ndim == 1:
                f = {1: lambda: m[self.loc], 2: lambda: m[self.row]}[axis]()
            else:
                f = {0: lambda: m[self.row, self.hap], 2: lambda: m[self.hap, self.loc]}[axis]()
        self.val = np.where(self.elim, 0.0, self.val * f)

    def normalize_reads(self, axis, grouping_mat=None):
        if axis in (GROUP, HAPLOGROUP) and self.groups is None and grouping_mat is None:
            raise RuntimeError('Group information matrix is missing.')
        if axis in (LOCUS, GROUP, HAPLOGROUP):
            self.elim = self.elim | (self.val == 0.0)
        g = self.gene[self.loc]
        key = {READ: self.row,
               HAPLOTYPE: self.row * self.H + self.hap,
               LOCUS: self.row * self.L + self.loc,
               GROUP: self.row * self.L + g,
               HAPLOGROUP: (self.row * self.L + g) * self.H + self.hap}[axis]
        _, inv = np.unique(key, return_inverse=True)
        den = np.bincount(inv, weights=self.val, minlength=inv.max() + 1 if len(inv) else 0)[inv]
        live = ~self.elim
        bad = live & (den == 0.0)
        ok = live & ~bad
        self.val[ok] = self.val[ok] / den[ok]
        if bad.any():
            raise FloatingPointError('invalid value encountered in divide')

    def sum(self, axis):
        if axis == READ:
            w = self.val if self.count is None else self.val * self.count[self.row]
            return np.bincount(self.hap * self.L + self.loc, weights=w, minlength=self.H * self.L).reshape(self.H, self.L)
        if axis == LOCUS:
            return np.bincount(self.row * self.H + self.hap, weights=self.val,
                               minlength=self.R * self.H).reshape(self.R, self.H)
        raise NotImplementedError

    def values(self, h):
        return self.val[self.off[h]:self.off[h + 1]].copy()

    def live(self, h):
        return ~self.elim[self.off[h]:self.off[h + 1]]

    def nnz(self):
        return int((~self.elim).sum())


# ---- the recorded operations -----------------------------------------------------------------------------------------
# A step is (method, argument...); a multiplier is named by its key in the fixture.  Every operation starts from the
# fixture's stored values (5 % of them 0 where the case has any).  `mul_locus` starts from reset(): the reference's
# product with a diagonal matrix (Sparse3DMatrix.py:328-333) drops a stored entry whose result is 0, which is not part of
# the tensor's contract; `squared` multiplies by a copy after normalize_reads(GROUP) has eliminated the zeros, for the
# same reason (scipy's elementwise product keeps no zero either).
OPS = {
    "reset": [("reset",)],
    "mul_locus": [("reset",), ("multiply", "m_locus", 1)],
    "mul_read": [("multiply", "m_read", 2)],
    "mul_read_hap": [("multiply", "m_rh", 0)],
    "mul_hap_locus": [("multiply", "m_hl", 2)],
    "norm_read": [("normalize_reads", READ)],
    "norm_haplotype": [("normalize_reads", HAPLOTYPE)],
    "norm_locus": [("normalize_reads", LOCUS)],
    "norm_group": [("normalize_reads", GROUP)],
    "norm_haplogroup": [("normalize_reads", HAPLOGROUP)],
    # eliminated entries stay out after reset(); a copy multiplies its source
    "squared": [("normalize_reads", GROUP), ("reset",), ("multiply", "m_hl", 2), ("multiply_copy",)],
}
NEEDS_GROUPS = ("norm_group", "norm_haplogroup", "squared")
WITH_SUMS = ("reset", "norm_read", "squared")        # sum(READ) and sum(LOCUS) recorded with these (and with the inputs)
FROM_RESTATEMENT = ("norm_haplotype",)               # scipy 1.15 refuses the IntEnum axis at AlignmentPropertyMatrix.py:332


def case_ops(g):
    return [op for op in OPS if bool(g["has_groups"]) or op not in NEEDS_GROUPS]


def run_steps(t, steps, g):
    """Run the steps of one operation on `t` (anything with the tensor's methods); returns t."""
    for step in steps:
        if step[0] == "reset":
            t.reset()
        elif step[0] == "multiply":
            t.multiply(np.asarray(g[step[1]]), axis=step[2])
        elif step[0] == "normalize_reads":
            t.normalize_reads(step[1])
        elif step[0] == "multiply_copy":
            c = t.copy()
            t.multiply(c)
            if hasattr(c, "close"):
                c.close()
        else:
            raise KeyError(step[0])
    return t


def fixture_inputs(g):
    """(R, L, H, indptr, indices, values, count, groups) of a tensor_*.npz fixture."""
    L, H, R = (int(x) for x in g["shape"])
    indptr = [g[f"indptr{h}"] for h in range(H)]
    indices = [g[f"indices{h}"] for h in range(H)]
    values = [g[f"values{h}"] for h in range(H)]
    count = g["count"] if bool(g["has_count"]) else None
    groups = None
    if bool(g["has_groups"]):
        gp, gm = g["group_ptr"], g["group_members"]
        groups = [[int(x) for x in gm[gp[i]:gp[i + 1]]] for i in range(len(gp) - 1)]
    return R, L, H, indptr, indices, values, count, groups


def restatement(g):
    R, L, H, indptr, indices, values, count, groups = fixture_inputs(g)
    return TensorRestate(R, L, H, indptr, indices, values, count, groups)


def flat_values(t, H):
    return np.concatenate([np.asarray(t.values(h), dtype=np.float64) for h in range(H)])


def flat_live(t, H):
    return np.concatenate([np.asarray(t.live(h), dtype=bool) for h in range(H)])
