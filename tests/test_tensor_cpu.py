"""The numpy restatement of the alignment tensor's arithmetic against the tensor_*.npz fixtures (made by running the
reference, scripts/gen_golden_tensor.py), and the host-side checks of gbrs_amd.tensor.  No device."""
import numpy as np
import pytest

from conftest import golden_files, load_golden
import tensor_restate as tr

FIXTURES = golden_files("tensor")
IDS = [p.split("/")[-1][:-4] for p in FIXTURES]
TOL = 1e-12


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=TOL, atol=1e-300)


def test_fixture_set():
    assert IDS == ["tensor_empty", "tensor_h1", "tensor_h16", "tensor_longrow", "tensor_main"]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_restatement_matches_reference(path):
    """Every recorded operation, from the fixture's inputs.  `norm_haplotype` is the restatement's own record (the
    reference's HAPLOTYPE branch does not run under the scipy that made the fixtures): there it only pins the file."""
    g = load_golden(path)
    H = int(g["shape"][1])
    assert list(g["from_restatement"]) == list(tr.FROM_RESTATEMENT)
    t = tr.restatement(g)
    close(t.sum(tr.READ), g["input_sum_read"])
    close(t.sum(tr.LOCUS), g["input_sum_locus"])
    assert t.nnz() == sum(len(g[f"indices{h}"]) for h in range(H))
    for op in tr.case_ops(g):
        t = tr.run_steps(tr.restatement(g), tr.OPS[op], g)
        close(tr.flat_values(t, H), g[f"{op}_val"])
        assert np.array_equal(tr.flat_live(t, H), g[f"{op}_live"]), op
        assert t.nnz() == int(g[f"{op}_live"].sum())
        if op in tr.WITH_SUMS:
            close(t.sum(tr.READ), g[f"{op}_sum_read"])
            close(t.sum(tr.LOCUS), g[f"{op}_sum_locus"])


def test_fixtures_hold_what_the_kernels_can_get_wrong():
    g = load_golden([p for p in FIXTURES if p.endswith("tensor_main.npz")][0])
    L, H, R = (int(x) for x in g["shape"])
    assert (L, H, R) == (97, 8, 1537)
    widths = np.concatenate([np.diff(g[f"indptr{h}"].astype(np.int64)) for h in range(H)])
    assert widths.max() > 3 * 256 - 64 and (widths <= 2).sum() > 64          # a column across workgroups; many per wavefront
    rows = np.concatenate([g[f"indices{h}"] for h in range(H)])
    assert not np.isin(np.arange(100, 110), rows).any()                     # empty rows
    assert any((np.diff(g[f"indices{h}"].astype(np.int64)) < 0).sum() > 100 for h in range(H))   # one haplotype descending
    zeros = sum(int((g[f"values{h}"] == 0).sum()) for h in range(H))
    assert 0.03 * len(rows) < zeros < 0.08 * len(rows)
    assert not g["norm_group_live"].all() and g["norm_read_live"].all()     # only LOCUS / GROUP / HAPLOGROUP eliminate
    assert int(g["group_members"].max()) < L - 1                            # the last loci are in no group
    g = load_golden([p for p in FIXTURES if p.endswith("tensor_longrow.npz")][0])
    rows = np.concatenate([g[f"indices{h}"] for h in range(8)])
    assert np.bincount(rows).max() == 700


# ---- host-side checks of gbrs_amd.tensor ---------------------------------------------------------------------------------
class Coo:
    """What tensor.groups_from_relation reads of a scipy sparse matrix."""

    def __init__(self, dense):
        self.shape = dense.shape
        self.row, self.col = np.nonzero(dense)
        self.data = dense[self.row, self.col]

    def tocoo(self):
        return self


def relation(L, groups):
    m = np.eye(L)
    for g in groups:
        m[np.ix_(g, g)] = 1.0
    return m


def test_multiplier_shapes():
    from gbrs_amd import tensor
    shape = (7, 2, 5)                                   # (L, H, R)
    assert tensor.multiply_form(np.ones(7), 1, shape)[0] == 1
    assert tensor.multiply_form(np.ones(5), tensor.Axis.READ, shape)[0] == 2
    assert tensor.multiply_form(np.ones((5, 2)), 0, shape)[0] == 3
    form, m = tensor.multiply_form(np.asfortranarray(np.arange(14.0).reshape(2, 7)), 2, shape)
    assert form == 4 and m.flags.c_contiguous and m[1, 0] == 7.0
    for m, axis in ((np.ones(5), 1), (np.ones(7), 2), (np.ones((2, 5)), 0), (np.ones((7, 2)), 2), (np.ones((2, 2, 2)), 0),
                    (np.ones(7), 3), (np.ones((2, 7)), None)):
        with pytest.raises(RuntimeError) as e:
            tensor.multiply_form(m, axis, shape)
        assert not isinstance(e.value, NotImplementedError)


def test_forms_that_are_not_implemented_say_which():
    from gbrs_amd import tensor
    shape = (7, 2, 5)
    with pytest.raises(NotImplementedError, match="1-D multiplier on axis 0"):
        tensor.multiply_form(np.ones(2), 0, shape)
    with pytest.raises(NotImplementedError, match="reads x loci"):
        tensor.multiply_form(np.ones((5, 7)), 1, shape)
    with pytest.raises(NotImplementedError, match="sparse"):
        tensor.multiply_form(Coo(np.ones((5, 7))), 1, shape)
    closed = object.__new__(tensor.DeviceTensor)        # no handle: these forms fail before they would need one
    closed.shape = shape
    with pytest.raises(NotImplementedError, match="HAPLOTYPE"):
        closed.sum(tensor.Axis.HAPLOTYPE)
    for name in ("add", "__add__", "__sub__", "__mul__", "bundle", "get_cross_section"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(closed, name)(np.ones(7))
    closed._h = None


def test_grouping_matrix_must_be_a_block_relation():
    from gbrs_amd import tensor
    L, groups = 9, [[1, 2, 3], [5, 7]]
    for make in (lambda m: m, Coo):
        assert tensor.groups_from_relation(make(relation(L, groups)), L) == groups
        assert tensor.groups_from_relation(make(np.eye(L)), L) == []
    m = relation(L, groups)
    m[1, 5] = 1.0                                       # not symmetric
    bad = [m.copy()]
    m[5, 1] = 1.0                                       # symmetric, not transitive
    bad.append(m.copy())
    m = relation(L, groups)
    m[8, 8] = 0.0                                       # a locus that is not related to itself
    bad.append(m)
    for m in bad:
        for make in (lambda x: x, Coo):
            with pytest.raises(RuntimeError, match="block relation"):
                tensor.groups_from_relation(make(m), L)
    with pytest.raises(RuntimeError, match="must be 9 x 9"):
        tensor.groups_from_relation(np.eye(8), L)


def test_group_axes_need_groups():
    from gbrs_amd import tensor
    A = tensor.Axis
    assert [int(a) for a in A] == [0, 1, 2, 3, 4] and A.LOCUS == 0 and A.READ == 2 and A.HAPLOGROUP == 4
    for axis in (A.GROUP, A.HAPLOGROUP):
        with pytest.raises(RuntimeError, match="Group information matrix is missing."):
            tensor.genes_for(axis, None, None, 5)
        assert tensor.genes_for(axis, None, ((0, 1),), 5) == ((0, 1),)
        assert tensor.genes_for(axis, relation(5, [[2, 4]]), ((0, 1),), 5) == [[2, 4]]
    for axis in (A.LOCUS, A.HAPLOTYPE, A.READ):
        assert tensor.genes_for(axis, None, None, 5) is None
    with pytest.raises(RuntimeError, match="axis should be"):
        tensor.genes_for(5, None, None, 5)
    with pytest.raises(RuntimeError, match="Group information matrix is missing."):
        tr.restatement(load_golden([p for p in FIXTURES if p.endswith("tensor_h1.npz")][0])).normalize_reads(tr.GROUP)


def test_alignment_matrix_hands_out_a_device_tensor():
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.tensor import DeviceTensor
    assert callable(AlignmentPropertyMatrix.on_device)
    assert {"reset", "multiply", "normalize_reads", "sum", "copy", "values", "live", "nnz", "close"} <= set(dir(DeviceTensor))
