"""Alignment counts on the device at the edges of its key packing, its sort and its column search, against the CPU
oracle (integer sums: exact).  Every case runs through gbrs_alignment_counts and through an AlignmentCounter, at the
isoform level and, where the case has a gene map, at the gene level (needs an MI355X)."""
import ctypes as C

import numpy as np
import pytest

import small_ops_cases as cases

pytestmark = pytest.mark.gpu


def make_apm(c):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    return AlignmentPropertyMatrix(shape=(c.L, c.H, c.R), indptr=c.indptr, indices=c.indices, count=c.count,
                                   haplotype_names=[f"h{h:02d}" for h in range(c.H)],
                                   locus_names=[f"T{l:05d}" for l in range(c.L)])


def set_groups(apm, locus_group, num_out):
    locus_group = np.asarray(locus_group)
    apm.groups = [np.flatnonzero(locus_group == g).tolist() for g in range(num_out)]
    apm.gname = np.array([f"G{g:05d}" for g in range(num_out)])
    apm.num_groups = num_out


def expected(c, locus_group=None, num_out=None):
    from oracle.counts_oracle import alignment_counts
    return alignment_counts(c.R, c.L, c.H, c.indptr, c.indices, c.count, locus_group, num_out)


def assert_counts(got, exp, what):
    for name, g, e in zip(("aln", "allele_unique", "locus_unique"), got[:3], exp):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def check_case(c, maps=None):
    """Both entry points, isoform level and every gene map, against the oracle; returns the oracle's values per level."""
    from gbrs_amd.counts import AlignmentCounter, alignment_counts
    if maps is None:
        maps = {} if c.locus_group is None else {"genes": (c.locus_group, c.num_out)}
    apm = make_apm(c)
    out = {"isoforms": expected(c)}
    assert_counts(alignment_counts(apm), out["isoforms"], "one-shot isoforms")
    with AlignmentCounter(apm) as counter:
        assert_counts(counter.counts(False), out["isoforms"], "counter isoforms")
        for name, (group, num_out) in maps.items():
            out[name] = expected(c, group, num_out)
            set_groups(apm, group, num_out)
            assert_counts(counter.counts(True), out[name], f"counter {name}")
            assert_counts(alignment_counts(apm, grp_wise=True), out[name], f"one-shot {name}")
    return out


@pytest.mark.parametrize("H", [1, 16, 32])
def test_counts_haplotype_counts(H):
    """H = 32 uses all five haplotype bits of the key."""
    c = cases.counts_hap_case(H)
    out = check_case(c)
    assert out["isoforms"][0][H - 1].sum() > 0 and out["genes"][0].sum() < out["isoforms"][0].sum()


@pytest.mark.parametrize("R", [1, 2, 4096, 4097])
def test_counts_row_counts(R):
    """R = 4096: row R - 1 sets every row bit that the sort compares, next to the all-ones keys of dropped entries."""
    c = cases.counts_row_case(R)
    out = check_case(c)
    assert out["genes"][0].sum() > 0


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257])
def test_counts_entry_counts(N):
    """One wavefront, one block, and one entry more or less; empty columns at both ends of every haplotype."""
    check_case(cases.counts_entry_case(N))


def test_counts_hand_checkable_rows():
    c, isoforms, genes = cases.counts_hand_case()
    out = check_case(c)
    assert_counts(out["isoforms"], isoforms, "written out, isoforms")
    assert_counts(out["genes"], genes, "written out, genes")


def test_counts_group_maps():
    c = cases.counts_map_case()
    out = check_case(c, cases.group_maps(c.L))
    for v in out["all_ungrouped"]:
        assert not v.any()
    np.testing.assert_array_equal(out["one_gene"][2], [c.count[np.unique(cases.triplets_of(c)[0])].sum()])
    assert out["fifty_genes"][0].shape == (c.H, 50) and (out["fifty_genes"][0].sum(axis=0) == 0).sum() >= 30


def test_counts_one_handle_several_queries():
    """The workspace and the zeroed outputs of one handle over queries with different numbers of output loci."""
    from gbrs_amd.counts import AlignmentCounter
    c = cases.counts_map_case()
    maps = cases.group_maps(c.L)
    apm = make_apm(c)
    with AlignmentCounter(apm) as counter:
        for name in ("isoforms", "three_genes", "fifty_genes", "isoforms", "three_genes"):
            if name == "isoforms":
                assert_counts(counter.counts(False), expected(c), name)
            else:
                set_groups(apm, *maps[name])
                assert_counts(counter.counts(True), expected(c, *maps[name]), name)


def test_counts_argument_errors_leave_the_handle_usable():
    from gbrs_amd import _lib
    lib = _lib.load()
    c = cases.counts_map_case()
    handle = C.c_void_p()
    _lib.check(lib.gbrs_counts_create(c.R, c.L, c.H, _lib.ptr_table(c.indptr), _lib.ptr_table(c.indices), _lib.ptr(c.count),
                                      0, C.byref(handle)))
    try:
        good = np.asarray(cases.group_maps(c.L)["three_genes"][0], dtype=np.int32)
        exp = expected(c, good, 3)

        def query(group, num_out):
            aln, uniq, lu = np.full((c.H, 64), -1.0), np.full((c.H, 64), -1.0), np.full(64, -1.0)
            st = lib.gbrs_counts_get(handle, _lib.ptr(group), num_out, _lib.ptr(aln), _lib.ptr(uniq), _lib.ptr(lu))
            return st, aln, uniq, lu

        too_big, too_small = good.copy(), good.copy()
        too_big[7] = 3
        too_small[11] = -2
        for group, num_out in ((good, 0), (good, 1 << 27), (too_big, 3), (too_small, 3)):
            st, aln, uniq, lu = query(group, num_out)
            assert st == _lib.GBRS_ERR_INVALID
            assert (aln == -1.0).all() and (uniq == -1.0).all() and (lu == -1.0).all()      # nothing written
            st, aln, uniq, lu = query(good, 3)
            assert st == _lib.GBRS_OK
            got = (aln.reshape(-1)[:c.H * 3].reshape(c.H, 3), uniq.reshape(-1)[:c.H * 3].reshape(c.H, 3), lu[:3])
            assert_counts(got, exp, "after an error")
    finally:
        lib.gbrs_counts_destroy(handle)
