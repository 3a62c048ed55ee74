"""gbrs_amd.tensor.DeviceTensor (gbrs_tensor_*, gbrs_amd/csrc/tensor.hip) against the tensor_*.npz fixtures made by running
the reference, and the reference's E-step composed from the operators against the EM fixtures (needs an MI355X)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_files, load_golden
import em_models_restate
import tensor_restate as tr

pytestmark = pytest.mark.gpu

RTOL = 1e-9               # the project's bound for EM quantities; the restatement meets 1e-12 against the reference
FIXTURES = golden_files("tensor")
IDS = [p.split("/")[-1][:-4] for p in FIXTURES]
EM_FIXTURES = golden_files("emmodel") + golden_files("em")
EM_IDS = [p.split("/")[-1][:-4] for p in EM_FIXTURES]


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=1e-300)


def make_apm(R, L, H, indptr, indices, values, count, groups):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count, values=values)
    if groups is not None:
        apm.groups = groups
        apm.num_groups = len(groups)
    return apm


def device_tensor(g):
    return make_apm(*tr.fixture_inputs(g)).on_device()


def main_fixture():
    return load_golden([p for p in FIXTURES if p.endswith("tensor_main.npz")][0])


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_operations_match_reference_fixture(path):
    g = load_golden(path)
    H = int(g["shape"][1])
    n = sum(len(g[f"indices{h}"]) for h in range(H))
    with device_tensor(g) as t:
        assert t.nnz() == n
        close(t.sum(t.Axis.READ), g["input_sum_read"])
        close(t.sum(t.Axis.LOCUS), g["input_sum_locus"])
    for op in tr.case_ops(g):
        runs = []
        for _ in range(2):
            with device_tensor(g) as t:
                tr.run_steps(t, tr.OPS[op], g)
                runs.append((tr.flat_values(t, H), tr.flat_live(t, H), t.nnz(per_haplotype=True), t.sum(t.Axis.LOCUS),
                             t.sum(t.Axis.READ)))
        val, live, nnz, sum_locus, sum_read = runs[0]
        close(val, g[f"{op}_val"])
        assert np.array_equal(live, g[f"{op}_live"]), op
        off = np.concatenate(([0], np.cumsum([len(g[f"indices{h}"]) for h in range(H)])))
        assert [int(x) for x in nnz] == [int(g[f"{op}_live"][off[h]:off[h + 1]].sum()) for h in range(H)], op
        if op in tr.WITH_SUMS:
            close(sum_read, g[f"{op}_sum_read"])
            close(sum_locus, g[f"{op}_sum_locus"])
        # everything but sum(READ) adds in a fixed order
        assert val.tobytes() == runs[1][0].tobytes() and np.array_equal(live, runs[1][1]), op
        assert sum_locus.tobytes() == runs[1][3].tobytes(), op
        close(sum_read, runs[1][4])


def e_step(t, model, theta, t2t):
    """EMfactory.update_probability_at_read_level (EMfactory.py:159-208) on the device tensor; the host multiplies theta
    by the gene relation."""
    A = t.Axis
    t.reset()
    t.multiply(theta, axis=A.READ)
    if model == 1:
        t.normalize_reads(axis=A.HAPLOGROUP)
        haplogroup_sum = theta @ t2t
        t.multiply(haplogroup_sum, axis=A.READ)
        t.normalize_reads(axis=A.GROUP)
        t.multiply(haplogroup_sum.sum(axis=0), axis=A.HAPLOTYPE)
    elif model == 2:
        t.normalize_reads(axis=A.LOCUS)
        t.multiply(theta.sum(axis=0), axis=A.HAPLOTYPE)
        t.normalize_reads(axis=A.GROUP)
        t.multiply((theta @ t2t).sum(axis=0), axis=A.HAPLOTYPE)
    elif model == 3:
        t.normalize_reads(axis=A.GROUP)
        t.multiply((theta @ t2t).sum(axis=0), axis=A.HAPLOTYPE)
    t.normalize_reads(axis=A.READ)


@pytest.mark.parametrize("path", EM_FIXTURES, ids=EM_IDS)
def test_reference_e_step_composed_from_the_operators(path):
    g = load_golden(path)
    model = int(g["model"]) if "model" in g else 4
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = em_models_restate.fixture_inputs(g)
    groups = [[int(x) for x in m] for m in groups]
    apm = make_apm(R, L, H, indptr, indices, values, count, groups)
    if gtmask is not None:
        apm.set_haplotype_mask(((gtmask != 0).astype(np.uint32) << np.arange(H, dtype=np.uint32)[:, None])
                               .sum(axis=0).astype(np.uint32))
    t2t = np.eye(L)
    for members in groups:
        t2t[np.ix_(members, members)] = 1.0
    theta = g["theta0"].copy()
    with apm.on_device() as t:
        for k in (1, 2):
            e_step(t, model, theta, t2t)
            theta = t.sum(t.Axis.READ)
            if eff_len is not None:
                theta = theta / eff_len
            close(theta, g[f"theta_iter{k}"])


def test_eliminated_entries_stay_out_and_copies_are_independent():
    g = main_fixture()
    H = int(g["shape"][1])
    with device_tensor(g) as t:
        n = t.nnz()
        t.normalize_reads(axis=t.Axis.GROUP)
        dead = ~g["norm_group_live"]
        assert dead.any() and t.nnz() == n - int(dead.sum())
        t.reset()
        ones = tr.flat_values(t, H)
        assert np.array_equal(ones, np.where(dead, 0.0, 1.0))
        t.multiply(g["m_hl"], axis=2)
        before = tr.flat_values(t, H)
        assert (before[dead] == 0.0).all() and (before[~dead] != 0.0).all()
        cpu = tr.run_steps(tr.restatement(g), tr.OPS["squared"][:3], g)
        close(t.sum(t.Axis.READ), cpu.sum(tr.READ))
        with t.copy() as c:
            assert np.array_equal(tr.flat_values(c, H), before) and np.array_equal(tr.flat_live(c, H), ~dead)
            t.multiply(c)                                   # squares the values ...
            close(tr.flat_values(t, H), g["squared_val"])
            close(t.sum(t.Axis.READ), g["squared_sum_read"])
            assert np.array_equal(tr.flat_values(c, H), before)          # ... of t alone
            c.reset()
            c.multiply(g["m_read"], axis=2)
            close(tr.flat_values(t, H), g["squared_val"])
            assert c.nnz() == t.nnz() == n - int(dead.sum())
        # the structure outlives the copy, and a tensor multiplies itself
        t.multiply(t)
        close(tr.flat_values(t, H), g["squared_val"] ** 2)
        for h in range(H):                                 # set_values leaves the eliminated entries at 0
            t.set_values(h, np.full(len(g[f"indices{h}"]), 2.0))
        assert np.array_equal(tr.flat_values(t, H), np.where(dead, 0.0, 2.0))


def test_zero_denominator_raises_and_leaves_the_entries():
    g = main_fixture()
    L, H, R = (int(x) for x in g["shape"])
    rows = [g[f"indices{h}"].astype(np.int64) for h in range(H)]
    r0 = int(np.flatnonzero(np.bincount(rows[0], minlength=R) >= 2)[0])       # a read with two entries of haplotype 0
    for axis in (tr.READ, tr.HAPLOTYPE):
        # all of the read's entries 0
        m = np.ones(R)
        m[r0] = 0.0
        with device_tensor(g) as t:
            t.multiply(m, axis=2)
            cpu = tr.restatement(g)
            cpu.multiply(m, axis=2)
            with pytest.raises(FloatingPointError):
                cpu.normalize_reads(axis)
            with pytest.raises(FloatingPointError, match="invalid value encountered in divide"):
                t.normalize_reads(axis=axis)
            val = tr.flat_values(t, H)
            assert (val[np.concatenate(rows) == r0] == 0.0).all() and np.isfinite(val).all()
            close(val, cpu.val)                            # every other read is normalised
            assert t.nnz() == len(val)
            t.reset()                                      # the error does not stick to the handle
            t.normalize_reads(axis=axis)
        # 0 by cancellation: the entries keep their values
        v0 = g["values0"].copy()
        mine = np.flatnonzero(rows[0] == r0)
        v0[mine] = 0.0
        v0[mine[0]], v0[mine[1]] = 1.5, -1.5
        with device_tensor(g) as t:
            for h in range(1, H if axis == tr.READ else 1):
                vh = g[f"values{h}"].copy()
                vh[rows[h] == r0] = 0.0
                t.set_values(h, vh)
            t.set_values(0, v0)
            with pytest.raises(FloatingPointError):
                t.normalize_reads(axis=axis)
            assert np.array_equal(t.values(0)[mine], v0[mine])


def test_abi_status_codes(hip_lib):
    from gbrs_amd import _lib
    g = main_fixture()
    L, H, R = (int(x) for x in g["shape"])
    out = np.zeros((H, L))
    for st in (hip_lib.gbrs_tensor_reset(None), hip_lib.gbrs_tensor_normalize(None, 2),
               hip_lib.gbrs_tensor_sum_reads(None, _lib.ptr(out)), hip_lib.gbrs_tensor_multiply(None, 1, _lib.ptr(out), L),
               hip_lib.gbrs_tensor_nnz(None, _lib.ptr(out)), hip_lib.gbrs_tensor_copy(None, C.byref(C.c_void_p()))):
        assert st == _lib.GBRS_ERR_INVALID
    assert b"NULL" in hip_lib.gbrs_last_error()
    assert hip_lib.gbrs_tensor_destroy(None) == _lib.GBRS_OK
    with device_tensor(g) as t:
        h = t._handle()
        for axis in (-1, 5):
            assert hip_lib.gbrs_tensor_normalize(h, axis) == _lib.GBRS_ERR_INVALID
        assert b"axis" in hip_lib.gbrs_last_error()
        m = np.ones(R * H)
        for form, n in ((1, L + 1), (2, R - 1), (3, R), (4, L), (0, L), (5, L), (9, L)):
            assert hip_lib.gbrs_tensor_multiply(h, form, _lib.ptr(m), n) == _lib.GBRS_ERR_INVALID
        assert hip_lib.gbrs_tensor_multiply(h, 1, None, L) == _lib.GBRS_ERR_INVALID
        assert hip_lib.gbrs_tensor_values(h, H, _lib.ptr(m), None, 0) == _lib.GBRS_ERR_INVALID
        assert hip_lib.gbrs_tensor_values(h, 0, _lib.ptr(m), None, 1) == _lib.GBRS_ERR_INVALID
        ptr, mem = np.array([0, 2, 4], dtype=np.int64), np.array([3, 4, 4, 5], dtype=np.int64)
        assert hip_lib.gbrs_tensor_set_groups(h, 2, _lib.ptr(ptr), _lib.ptr(mem)) == _lib.GBRS_ERR_INVALID
        assert b"locus 4 is in two groups (0 and 1)" in hip_lib.gbrs_last_error()
        mem[2] = L
        assert hip_lib.gbrs_tensor_set_groups(h, 2, _lib.ptr(ptr), _lib.ptr(mem)) == _lib.GBRS_ERR_INVALID
        assert b"out of range" in hip_lib.gbrs_last_error()
        with make_apm(*tr.fixture_inputs(g)).on_device() as other:
            assert hip_lib.gbrs_tensor_multiply_tensor(h, other._handle()) == _lib.GBRS_ERR_UNSUPPORTED
            with pytest.raises(NotImplementedError, match="another structure"):
                t.multiply(other)
        t.normalize_reads(axis=t.Axis.GROUP)              # the failed calls left the handle and its genes as they were
        close(tr.flat_values(t, H), g["norm_group_val"])
    # a row id beyond num_rows never reaches the device
    R1, L1, H1, indptr, indices, values, count, groups = tr.fixture_inputs(g)
    bad = [ix.copy() for ix in indices]
    bad[2][5] = R1
    hh = C.c_void_p()
    st = hip_lib.gbrs_tensor_create(R1, L1, H1, _lib.ptr_table(indptr), _lib.ptr_table(bad), None, None, 0, C.byref(hh))
    assert st == _lib.GBRS_ERR_INVALID and not hh and b"row id" in hip_lib.gbrs_last_error()


def test_grouping_matrix_replaces_the_genes():
    g = main_fixture()
    L, H, R = (int(x) for x in g["shape"])
    R_, L_, H_, indptr, indices, values, count, groups = tr.fixture_inputs(g)
    t2t = np.eye(L)
    for members in groups:
        t2t[np.ix_(members, members)] = 1.0
    with make_apm(R, L, H, indptr, indices, values, count, None).on_device() as t:
        with pytest.raises(RuntimeError, match="Group information matrix is missing."):
            t.normalize_reads(axis=t.Axis.GROUP)
        with t.copy() as c:
            c.normalize_reads(axis=c.Axis.HAPLOGROUP, grouping_mat=t2t)
            close(tr.flat_values(c, H), g["norm_haplogroup_val"])
        t.normalize_reads(axis=t.Axis.GROUP, grouping_mat=t2t)
        close(tr.flat_values(t, H), g["norm_group_val"])
    with device_tensor(g) as t:                           # the identity relation: every locus a gene, GROUP is LOCUS
        t.normalize_reads(axis=t.Axis.GROUP, grouping_mat=np.eye(L))
        close(tr.flat_values(t, H), g["norm_locus_val"])
        t.reset()
        t.multiply(g["m_hl"], axis=2)
        t.normalize_reads(axis=t.Axis.GROUP)              # back to the tensor's own groups
        cpu = tr.restatement(g)
        cpu.normalize_reads(tr.LOCUS)
        cpu.reset()
        cpu.multiply(g["m_hl"], axis=2)
        cpu.normalize_reads(tr.GROUP)
        close(tr.flat_values(t, H), cpu.val)


def test_operations_after_close():
    g = main_fixture()
    t = device_tensor(g)
    c = t.copy()
    t.close()
    t.close()
    for call in (t.reset, t.nnz, lambda: t.values(0), lambda: t.sum(2), lambda: t.normalize_reads(2), t.copy,
                 lambda: t.multiply(g["m_locus"], axis=1), lambda: c.multiply(t)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    c.normalize_reads(axis=c.Axis.READ)                   # the copy keeps the shared structure alive
    close(tr.flat_values(c, int(g["shape"][1])), g["norm_read_val"])
    c.close()
