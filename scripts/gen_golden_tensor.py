#!/usr/bin/env python3
"""Generate tests/golden/tensor_<case>.npz by running the imported reference's tensor arithmetic.

Build container only (the reference's sources are not on the GPU machines); no test, smoke() or bench.py calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_tensor.py

Every file holds the inputs (shape, indptr{h}, indices{h}, values{h}, count, groups, the multipliers) and, for every
operation of tests/tensor_restate.py OPS, the reference's values scattered back onto the input structure (`<op>_val`,
0 where the reference dropped the entry) and which entries it still stores (`<op>_live`); `<op>_sum_read` and
`<op>_sum_locus` for the operations of WITH_SUMS and for the inputs (`input_sum_*`).

As in scripts/gen_golden_models.py the `np` name inside the reference's AlignmentPropertyMatrix module is a proxy whose
divide(sparse, sparse) divides the stored entries of the numerator, and `tables` is a stand-in.  normalize_reads on the
HAPLOTYPE axis does not run under scipy 1.15 (it refuses the IntEnum axis at AlignmentPropertyMatrix.py:332), so
`norm_haplotype_*` comes from the restatement of lines 328-334 (`from_restatement` names it).  Everything else is asserted
to agree with the restatement to 1e-12 before it is written.
"""
import os
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.environ.get("GBRS_REFERENCE_SRC", "/root/reference/src")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF_SRC)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

WORK = tempfile.mkdtemp(prefix="gbrs_golden_tensor_")
os.environ["GBRS_DATA"] = WORK
sys.modules.setdefault("tables", types.ModuleType("tables"))

import gbrs.emase.AlignmentPropertyMatrix as ref_apm_mod  # noqa: E402
from gbrs.emase.AlignmentPropertyMatrix import AlignmentPropertyMatrix as RefAPM  # noqa: E402
from gbrs.emase.EMfactory import EMfactory as RefEM  # noqa: E402

import tensor_restate as tr  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
# few distinct values, all exact in binary: the files deflate well and a wrong factor is still a wrong number
PALETTE = np.array([0.5, 0.75, 1.25, 1.5, 2.0, 3.0])


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


class RefTensor:
    """The reference's AlignmentPropertyMatrix behind the interface run_steps() drives."""

    def __init__(self, c, apm=None, t2t=None):
        self.c = c
        if apm is not None:
            self.apm, self.t2t = apm, t2t
            return
        self.apm = self._make()
        self.t2t = None
        if c["groups"] is not None:
            em = RefEM(self._make())           # t2t_mat as EMfactory.prepare builds it, on a throw-away tensor
            with np.errstate(all="ignore"):
                em.prepare()
            self.t2t = em.t2t_mat

    def _make(self):
        c = self.c
        R, H, L = c["R"], c["H"], c["L"]
        grpfile = None
        if c["groups"] is not None:
            grpfile = os.path.join(tempfile.mkdtemp(dir=WORK), "g2t.tsv")
            with open(grpfile, "w") as fh:
                for i, members in enumerate(c["groups"]):
                    fh.write(f"G{i:07d}\t" + "\t".join(f"T{l:07d}" for l in members) + "\n")
        apm = RefAPM(shape=(L, H, R), haplotype_names=[f"H{h:02d}" for h in range(H)],
                     locus_names=[f"T{l:07d}" for l in range(L)], grpfile=grpfile)
        for h in range(H):
            apm.data[h] = sp.csc_matrix((c["values"][h].copy(), c["indices"][h].astype(np.int64),
                                         c["indptr"][h].astype(np.int64)), shape=(R, L))
        apm.finalized = True
        if c["count"] is not None:
            apm.count = c["count"].copy()
        return apm

    def reset(self):
        self.apm.reset()

    def multiply(self, m, axis=None):
        self.apm.multiply(m.apm if isinstance(m, RefTensor) else m, axis=axis)

    def normalize_reads(self, axis):
        self.apm.normalize_reads(axis=RefAPM.Axis(axis), grouping_mat=self.t2t)

    def copy(self):
        return RefTensor(self.c, self.apm.copy(), self.t2t)

    def sum(self, axis):
        return np.asarray(self.apm.sum(axis=RefAPM.Axis(axis)))

    def scatter(self):
        """values and live mask on the input structure, the haplotypes one after the other"""
        c = self.c
        R = c["R"]
        vals, lives = [], []
        for h in range(c["H"]):
            col = np.repeat(np.arange(c["L"], dtype=np.int64), np.diff(c["indptr"][h].astype(np.int64)))
            key = col * R + c["indices"][h].astype(np.int64)
            order = np.argsort(key, kind="stable")
            assert len(np.unique(key)) == len(key)
            m = self.apm.data[h].tocoo()
            mkey = m.col.astype(np.int64) * R + m.row.astype(np.int64)
            assert len(np.unique(mkey)) == len(mkey), "the reference stores an entry twice"
            pos = np.searchsorted(key[order], mkey)
            assert (pos < len(key)).all() and (key[order][pos] == mkey).all(), "the reference grew an entry"
            v = np.zeros(len(key))
            live = np.zeros(len(key), dtype=bool)
            v[order[pos]] = m.data
            live[order[pos]] = True
            vals.append(v)
            lives.append(live)
        return np.concatenate(vals), np.concatenate(lives)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- cases -----------------------------------------------------------------------------------------------------------
def consecutive_groups(rng, n_groups, L, lo=1, hi=5):
    sizes = rng.integers(lo, hi, size=n_groups)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    assert sizes.sum() < L, "some loci must stay ungrouped"
    return [list(range(int(s), int(s + n))) for s, n in zip(starts, sizes)]


def build_case(R, H, L, triples, rng, groups=None, with_count=False, zeros=0.05, descending_hap=None):
    """triples: set of (row, hap, locus).  Stored values from PALETTE; a share of them 0, never all of a read's entries of
    one haplotype (so that READ and HAPLOTYPE meet no 0/0 on the inputs)."""
    t = np.array(sorted(triples), dtype=np.int64).reshape(-1, 3)
    indptr, indices, values = [], [], []
    for h in range(H):
        e = t[t[:, 1] == h]
        order = np.lexsort((e[:, 0], e[:, 2]))             # by locus, rows ascending inside a column
        if h == descending_hap:
            order = np.lexsort((-e[:, 0], e[:, 2]))
        e = e[order]
        indptr.append(np.searchsorted(e[:, 2], np.arange(L + 1)).astype(np.uint32))
        indices.append(e[:, 0].astype(np.uint32))
        v = rng.choice(PALETTE, size=len(e))
        left = np.bincount(e[:, 0], minlength=R)            # nonzero entries of (row, h) still standing
        for k in rng.permutation(len(e))[:int(round(zeros * len(e) * 2))]:
            if left[e[k, 0]] > 1:
                v[k] = 0.0
                left[e[k, 0]] -= 1
        values.append(v)
    return dict(R=R, H=H, L=L, indptr=indptr, indices=indices, values=values, groups=groups,
                count=rng.integers(1, 6, size=R).astype(np.float64) if with_count else None,
                m_locus=rng.choice(PALETTE, size=L), m_read=rng.choice(PALETTE, size=R),
                m_rh=rng.choice(PALETTE, size=(R, H)), m_hl=rng.choice(PALETTE, size=(H, L)))


def random_reads(rng, rows, H, L, pop, p_hap, max_loci=3):
    out = set()
    for r in rows:
        for l in np.unique(rng.choice(L, size=int(rng.integers(1, max_loci + 1)), p=pop)):
            m = rng.random(H) < p_hap
            if not m.any():
                m[rng.integers(0, H)] = True
            out.update((int(r), int(h), int(l)) for h in np.flatnonzero(m))
    return out


def case_main():
    rng = np.random.default_rng(201)
    R, H, L, busy, empty_locus = 1537, 8, 97, 5, 50
    groups = consecutive_groups(rng, 30, L - 4)
    pop = rng.lognormal(0.0, 2.2, size=L)                   # skewed: many columns of 0-2 entries
    pop[[busy, empty_locus]] = 0.0
    pop /= pop.sum()
    rows = [r for r in range(R) if not 100 <= r < 110]
    triples = random_reads(rng, rows, H, L, pop, 0.3)
    for h in range(H):                                      # a column of about R / 2 entries in every haplotype
        triples.update((int(r), h, busy) for r in rows if rng.random() < 0.5)
    return build_case(R, H, L, triples, rng, groups, with_count=True, descending_hap=3)


def case_h1():
    rng = np.random.default_rng(202)
    R, H, L = 65, 1, 3
    return build_case(R, H, L, random_reads(rng, range(R), H, L, np.full(L, 1 / L), 1.0, max_loci=2), rng)


def case_h16():
    rng = np.random.default_rng(203)
    R, H, L = 300, 16, 40
    pop = rng.lognormal(0.0, 1.2, size=L)
    return build_case(R, H, L, random_reads(rng, range(R), H, L, pop / pop.sum(), 0.4), rng,
                      consecutive_groups(rng, 12, L), with_count=True)


def case_longrow():
    rng = np.random.default_rng(204)
    R, H, L, long_row = 40, 8, 400, 7
    groups = [list(range(3 * g, 3 * g + 3)) for g in range(130)]           # loci 390-399 in no group
    triples = random_reads(rng, [r for r in range(R) if r != long_row], H, L, np.full(L, 1 / L), 0.4)
    mine = []
    for g in rng.choice(130, size=90, replace=False):
        for l in rng.choice(groups[g], size=2, replace=False):
            mine += [(long_row, int(h), int(l)) for h in rng.choice(H, size=4, replace=False)]
    mine = [mine[k] for k in rng.permutation(len(mine))[:700]]
    assert len({m[2] // 3 for m in mine}) == 90
    triples.update(mine)
    return build_case(R, H, L, triples, rng, groups)


def case_empty():
    return build_case(10, 2, 4, set(), np.random.default_rng(205))


CASES = dict(main=case_main, h1=case_h1, h16=case_h16, longrow=case_longrow, empty=case_empty)


def write_case(name, c):
    H = c["H"]
    g = dict(shape=np.array([c["L"], H, c["R"]], dtype=np.int64),
             has_count=c["count"] is not None, count=c["count"] if c["count"] is not None else np.zeros(0),
             has_groups=c["groups"] is not None,
             group_ptr=np.concatenate(([0], np.cumsum([len(x) for x in c["groups"] or []]))).astype(np.int64),
             group_members=np.array([l for x in c["groups"] or [] for l in x], dtype=np.int64),
             m_locus=c["m_locus"], m_read=c["m_read"], m_rh=c["m_rh"], m_hl=c["m_hl"],
             from_restatement=np.array(tr.FROM_RESTATEMENT))
    for h in range(H):
        g[f"indptr{h}"], g[f"indices{h}"], g[f"values{h}"] = c["indptr"][h], c["indices"][h], c["values"][h]
    assert tr.fixture_inputs(g)[7] == c["groups"]
    worst = 0.0

    def sums(prefix, ref, cpu):
        nonlocal worst
        for key, axis in (("sum_read", tr.READ), ("sum_locus", tr.LOCUS)):
            a, b = ref.sum(axis), cpu.sum(axis)
            assert a.shape == b.shape, (name, prefix, key, a.shape, b.shape)
            worst = max(worst, rel(b, a))
            g[f"{prefix}_{key}"] = a

    sums("input", RefTensor(c), tr.restatement(g))
    for op in tr.case_ops(g):
        cpu = tr.run_steps(tr.restatement(g), tr.OPS[op], g)
        if op in tr.FROM_RESTATEMENT:
            g[f"{op}_val"], g[f"{op}_live"] = tr.flat_values(cpu, H), tr.flat_live(cpu, H)
            continue
        with np.errstate(all="raise", under="ignore"):
            ref = tr.run_steps(RefTensor(c), tr.OPS[op], g)
        val, live = ref.scatter()
        assert np.array_equal(live, tr.flat_live(cpu, H)), (name, op, "live masks differ")
        worst = max(worst, rel(tr.flat_values(cpu, H), val))
        g[f"{op}_val"], g[f"{op}_live"] = val, live
        if op in tr.WITH_SUMS:
            sums(op, ref, cpu)
    assert worst < 1e-12, (name, worst)
    path = os.path.join(GOLD, f"tensor_{name}.npz")
    np.savez_compressed(path, **g)
    n = sum(len(x) for x in c["indices"])
    zeros = sum(int((v == 0).sum()) for v in c["values"])
    widths = np.concatenate([np.diff(p.astype(np.int64)) for p in c["indptr"]])
    print(f"tensor_{name}: R={c['R']} H={H} L={c['L']} N={n} stored zeros={zeros} widest column={widths.max() if n else 0} "
          f"columns of 0-2 entries={(widths <= 2).sum()} longest row="
          f"{np.bincount(np.concatenate(c['indices']).astype(np.int64)).max() if n else 0} "
          f"worst rel diff vs restatement={worst:.1e} size={os.path.getsize(path)} B")


def main():
    os.makedirs(GOLD, exist_ok=True)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    for name, make in CASES.items():
        if only in (None, name):
            write_case(name, make())


if __name__ == "__main__":
    main()
