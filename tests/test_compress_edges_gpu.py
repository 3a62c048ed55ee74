"""`gbrs compress` on the device where its row key collides, at rows and locus counts the fixtures do not reach, against
the CPU restatement: class count, structure, first-seen order and counts, all exact (needs an MI355X)."""
import time

import numpy as np
import pytest

import small_ops_cases as cases

pytestmark = pytest.mark.gpu


def make_apm(c):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    return AlignmentPropertyMatrix(shape=(c.L, c.H, c.R), indptr=c.indptr, indices=c.indices, count=c.count,
                                   haplotype_names=[f"h{h:02d}" for h in range(c.H)],
                                   locus_names=None if c.L > 100_000 else [f"T{l:05d}" for l in range(c.L)])


def check_case(c, what):
    """Device classes == the restatement's; returns (input matrix, class matrix, number of classes)."""
    from gbrs_amd.compress import compress_matrix
    from oracle.compress_oracle import compress as ref_compress
    apm = make_apm(c)
    t0 = time.perf_counter()
    ec = compress_matrix(apm)
    print(f"[{what}] R={c.R} L={c.L} H={c.H} N={c.N}: compress_matrix {time.perf_counter() - t0:.3f} s")
    n, ip, ix, counts = ref_compress(c.R, c.L, c.H, c.indptr, c.indices, c.count)
    assert ec.num_reads == n
    np.testing.assert_array_equal(ec.count, counts)
    for h in range(c.H):
        np.testing.assert_array_equal(ec.indptr[h], ip[h], err_msg=f"indptr of haplotype {h}")
        np.testing.assert_array_equal(ec.indices[h], ix[h], err_msg=f"indices of haplotype {h}")
    return apm, ec, n


def check_em_on_classes(apm, ec):
    """Five EM steps on the classes == five EM steps on the reads.  Single steps, not run(): the stopping rule looks at
    the loci's totals, and with every read on one locus those do not move, so its error is rounding noise around 0."""
    from gbrs_amd.em import EMfactory
    out = []
    for m in (apm, ec):
        em = EMfactory(m)
        em.target_lengths = np.ones((m.num_haplotypes, m.num_loci))
        em.prepare(0.0)
        for _ in range(5):
            em.update_allelic_expression(4)
        out.append(em.allelic_expression.copy())
        em.close()
    np.testing.assert_allclose(out[1], out[0], rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("with_count", [False, True], ids=["reads", "counted"])
def test_compress_h16_masks_that_share_a_key(with_count):
    """12,000 one-locus rows' masks under a 16-bit mask hash: copies of different rows interleave in the sorted order."""
    c = cases.h16_collision_case(with_count)
    apm, ec, n = check_case(c, "h16 collisions")
    assert n == 12_000
    check_em_on_classes(apm, ec)


def test_compress_h8_pairs_that_share_a_key():
    """10,200 two-locus rows under one (first locus, locus hash); the empty class takes its rank among them."""
    c = cases.h8_collision_case()
    apm, ec, n = check_case(c, "h8 collisions")
    assert n == 255 * 40 + 1
    empty_rank = int(np.setdiff1d(np.arange(n), np.concatenate(ec.indices))[0])
    assert 0 < empty_rank < 2000 and ec.count[empty_rank] == 300
    check_em_on_classes(apm, ec)


def test_compress_interleaved_rows_of_one_key():
    a, b, c3 = cases.three_rows_one_key()
    c = cases.interleaved_case()
    apm, ec, n = check_case(c, "A B C A B C")
    assert n == 3
    np.testing.assert_array_equal(ec.count, [4.0, 4.0, 4.0])
    for rank, mask in enumerate((a, b, c3)):                            # classes in the order A, B, C
        haps = [h for h in range(16) if rank in ec.indices[h][ec.indptr[h][1]:ec.indptr[h][2]]]
        assert sum(1 << h for h in haps) == mask


def test_compress_long_row():
    c = cases.long_row_case()
    apm, ec, n = check_case(c, "long row")
    assert n == 4
    np.testing.assert_array_equal(ec.count, [2.0, 1.0, 1.0, 1.0])        # rows 0 and 3 join, row 2 does not


def test_compress_more_than_2_pow_24_loci():
    """The key's first-locus field is shifted (rows that start at 2k and 2k + 1 share it, so do rows that start at a locus
    >= 2^24 and at locus 0), and the entry keys carry loci >= 2^24."""
    c = cases.large_l_case()
    apm, ec, n = check_case(c, "large L")
    assert n < c.R
    assert sum(int(ec.indptr[h][-1] - ec.indptr[h][1 << 24]) for h in range(c.H)) > 0


def test_compress_one_row():
    c = cases.csc_from_rows(4, 3, [[(0, 5), (3, 2)]], count=[7])
    apm, ec, n = check_case(c, "R = 1")
    assert n == 1
    np.testing.assert_array_equal(ec.count, [7.0])


def test_compress_all_rows_empty():
    c = cases.csc_from_rows(5, 2, [[] for _ in range(300)], count=np.arange(300) % 3 + 1)
    apm, ec, n = check_case(c, "all rows empty")
    assert n == 1 and ec.count[0] == c.count.sum()


def test_compress_no_entries_without_counts():
    c = cases.csc_from_rows(1, 1, [[] for _ in range(7)])
    assert c.N == 0
    apm, ec, n = check_case(c, "N = 0")
    assert n == 1 and ec.count[0] == 7.0


def test_compress_all_rows_identical():
    c = cases.csc_from_rows(6, 4, [[(1, 9), (2, 15), (5, 1)]] * 1000)
    apm, ec, n = check_case(c, "all rows identical")
    assert n == 1 and ec.count[0] == 1000.0
