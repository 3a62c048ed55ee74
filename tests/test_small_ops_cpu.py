"""The oracles of the four small device operations against brute force, scipy and hand rules, and the preconditions of
the generated edge cases (tests/small_ops_cases.py).  No GPU."""
import numpy as np
import pytest

import small_ops_cases as cases


def _tiny_case(seed, with_count, R=12, L=6, H=3):
    rng = np.random.default_rng(seed)
    flat = rng.choice(R * L, size=25, replace=False)
    rows, loci = flat // L, flat % L
    keep = rows != 4                                                   # row 4 stays empty
    rows, loci = rows[keep], loci[keep]
    # rows 7 and 9 repeat row 1, so that classes join and gene-level entries collapse
    for twin in (7, 9):
        sel = rows != twin
        rows, loci = rows[sel], loci[sel]
    masks = rng.integers(1, 1 << H, size=len(rows))
    for twin in (7, 9):
        sel = rows == 1
        rows = np.concatenate((rows, np.full(int(sel.sum()), twin)))
        loci = np.concatenate((loci, loci[sel]))
        masks = np.concatenate((masks, masks[sel]))
    count = rng.integers(1, 5, size=R).astype(np.float64) if with_count else None
    return cases.csc_from_masks(R, L, H, rows, loci, masks, count)


@pytest.mark.parametrize("with_count", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_counts_oracle_matches_brute_force(seed, with_count):
    from oracle.counts_oracle import alignment_counts
    c = _tiny_case(seed, with_count).with_groups([1, 1, -1, 0, 2, 0], 4)       # locus 2 in no gene, gene 3 without a locus
    for got, exp in zip(alignment_counts(c.R, c.L, c.H, c.indptr, c.indices, c.count), cases.brute_counts(c, False)):
        np.testing.assert_array_equal(got, exp)
    got = alignment_counts(c.R, c.L, c.H, c.indptr, c.indices, c.count, c.locus_group, c.num_out)
    for g, e in zip(got, cases.brute_counts(c, True)):
        np.testing.assert_array_equal(g, e)
    assert got[0].shape == (c.H, 4) and not got[0][:, 3].any()


def test_counts_hand_case_matches_both():
    from oracle.counts_oracle import alignment_counts
    c, isoforms, genes = cases.counts_hand_case()
    for got, exp, brute in zip(alignment_counts(c.R, c.L, c.H, c.indptr, c.indices, c.count), isoforms,
                               cases.brute_counts(c, False)):
        np.testing.assert_array_equal(got, exp)
        np.testing.assert_array_equal(brute, exp)
    for got, exp, brute in zip(alignment_counts(c.R, c.L, c.H, c.indptr, c.indices, c.count, c.locus_group, c.num_out),
                               genes, cases.brute_counts(c, True)):
        np.testing.assert_array_equal(got, exp)
        np.testing.assert_array_equal(brute, exp)


@pytest.mark.parametrize("with_count", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_compress_oracle_matches_brute_force(seed, with_count):
    from oracle.compress_oracle import compress
    c = _tiny_case(seed, with_count)
    n, ip, ix, cnt = compress(c.R, c.L, c.H, c.indptr, c.indices, c.count)
    bn, bip, bix, bcnt = cases.brute_compress(c)
    assert n == bn and n <= c.R - 2                                     # rows 1, 7 and 9 are one class
    np.testing.assert_array_equal(cnt, bcnt)
    for h in range(c.H):
        np.testing.assert_array_equal(ip[h], bip[h])
        np.testing.assert_array_equal(ix[h], bix[h])


INTERP = [(name, S) for name in cases.interp_positions() for S in cases.STATE_COUNTS
          if S in (3, 136) or name in ("on_knots", "one_gene")]


@pytest.mark.parametrize("name,S", INTERP)
def test_interpolate_oracle_matches_scipy(name, S):
    """scipy's interp1d on the knots the reference builds (gbrs_utils.interpolate: 0.0 in front, the last grid point + 1
    behind, the first and the last column repeated), bit for bit."""
    interp1d = pytest.importorskip("scipy.interpolate").interp1d
    from oracle import postproc_oracle
    x_gene, gamma, x_grid = cases.interp_case(name, S)
    x = np.append([0.0], [float(v) for v in x_gene])
    x = np.append(x, [x_grid[-1] + 1.0])
    y = np.hstack((gamma[:, 0][:, np.newaxis], gamma))
    y = np.hstack((y, y[:, -1][:, np.newaxis]))
    assert (np.diff(x) >= 0).all()                # the oracle's assumption; scipy would sort the knots otherwise
    expected = interp1d(x, y, axis=1)(x_grid)
    got = postproc_oracle.interpolate(x_gene, gamma, x_grid)
    assert got.shape == (S, len(x_grid)) and np.isfinite(expected).all()
    np.testing.assert_array_equal(got, expected)


def test_interpolate_edge_values():
    """What the edge cases are there for, on the oracle: a query on a repeated position gets the segment that ends at
    the first of the genes there, queries outside the genes get the first or the last column."""
    from oracle import postproc_oracle
    err = 4 * 2.0 ** -53          # four roundings (subtract, divide, multiply, add) of values within [-1, 1]
    x_gene, gamma, x_grid = cases.interp_case("two_at_one_position", 36)
    out = postproc_oracle.interpolate(x_gene, gamma, x_grid)
    np.testing.assert_allclose(out[:, 1], gamma[:, 1], rtol=0, atol=err)
    assert np.abs(gamma[:, 1] - gamma[:, 2]).max() > 1e-3
    x_gene, gamma, x_grid = cases.interp_case("three_at_one_position", 36)
    out = postproc_oracle.interpolate(x_gene, gamma, x_grid)
    np.testing.assert_allclose(out[:, 1], gamma[:, 1], rtol=0, atol=err)
    x_gene, gamma, x_grid = cases.interp_case("before_first_gene", 36)
    np.testing.assert_array_equal(postproc_oracle.interpolate(x_gene, gamma, x_grid), np.repeat(gamma[:, :1], 3, axis=1))
    x_gene, gamma, x_grid = cases.interp_case("after_last_gene", 36)
    np.testing.assert_array_equal(postproc_oracle.interpolate(x_gene, gamma, x_grid), np.repeat(gamma[:, -1:], 3, axis=1))
    x_gene, gamma, x_grid = cases.interp_case("on_knots", 36)
    out = postproc_oracle.interpolate(x_gene, gamma, x_grid)
    on = np.isin(x_grid, x_gene)
    assert on.sum() >= 10
    np.testing.assert_allclose(out[:, on], gamma[:, np.searchsorted(x_gene, x_grid[on])], rtol=0, atol=err)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_dosage_oracle_on_one_hot_rows(H):
    from oracle import postproc_oracle
    rows, expected = cases.dosage_one_hot(H)
    assert rows.shape == (H * (H + 1) // 2, H * (H + 1) // 2)
    np.testing.assert_array_equal(expected.sum(axis=1), 1.0)
    np.testing.assert_array_equal(postproc_oracle.dosage(rows, H), expected)


@pytest.mark.parametrize("H", [1, 3, 16])
def test_dosage_fsum_reference(H):
    from oracle import postproc_oracle
    rows, expected = cases.dosage_random(H, 33)
    np.testing.assert_allclose(postproc_oracle.dosage(rows, H), expected, rtol=cases.dosage_rtol(H), atol=0)
    np.testing.assert_allclose(expected.sum(axis=1), 1.0, rtol=1e-13)


def test_mix32_matches_the_scalar_definition():
    def scalar(h, v):
        h ^= (v + 0x9e3779b9 + (h << 6) + (h >> 2)) & 0xFFFFFFFF
        h = (h * 0x85ebca6b) & 0xFFFFFFFF
        return h ^ (h >> 13)
    vals = [0, 1, 0xFFFF, 0xFFFFFFFF, 0x12345678]
    got = cases.mix32(np.full(len(vals), cases.KEY_MASK_SEED), vals)
    assert [int(x) for x in got] == [scalar(cases.KEY_MASK_SEED, v) for v in vals]


def test_h16_collision_precondition():
    """The case reaches the kernels that join segments only if many different masks share a row key."""
    masks = cases.h16_collision_masks()
    assert len(np.unique(masks)) == 12_000
    keys = cases.row_keys(3, np.ones(len(masks), dtype=np.int64), masks)
    assert cases.shared_key_count(keys) >= 1000
    c = cases.h16_collision_case(True)
    assert 20_000 < c.R < 28_000 and c.H == 16 and c.L == 3
    assert c.indptr[0][1] == 0 and c.indptr[0][3] == c.indptr[0][2]     # every entry on locus 1


def test_h8_collision_precondition():
    pairs = cases.h8_collision_pairs()
    assert len(np.unique(pairs, axis=0)) == 255 * 40
    keys = cases.row_keys(2, np.tile([0, 1], (len(pairs), 1)), pairs)
    assert cases.shared_key_count(keys) >= 500
    c = cases.h8_collision_case()
    touched = np.zeros(c.R, dtype=bool)
    for h in range(c.H):
        touched[c.indices[h]] = True
    assert (~touched).sum() == 300 and touched[0] and not touched[:2000].all()    # the first empty row comes early, not first


def test_interleaved_precondition():
    a, b, c = cases.three_rows_one_key()
    assert len({a, b, c}) == 3
    assert len(set(cases.row_keys(3, [1, 1, 1], [a, b, c]).tolist())) == 1
    from oracle.compress_oracle import compress
    case = cases.interleaved_case()
    n, ip, ix, cnt = compress(case.R, case.L, case.H, case.indptr, case.indices)
    assert n == 3
    np.testing.assert_array_equal(cnt, [4.0, 4.0, 4.0])


def test_large_l_precondition():
    """Checked on a cheap stand-in for the shape logic, and on the loci of the real case."""
    c = cases.large_l_case()
    rows, loci, haps = cases.triplets_of(c)
    assert c.L == (1 << 24) + 3 and cases.bits_for(c.L - 1) == 25
    assert 2 * (loci >= 1 << 24).sum() >= len(loci)
    first = np.full(c.R, c.L)
    np.minimum.at(first, rows, loci)
    first = first[first < c.L]
    low = np.unique(first[first < 1 << 24])
    assert np.isin(low[low % 2 == 0] + 1, low).sum() >= 20              # rows that start at 2k and rows that start at 2k + 1
    assert (first >= 1 << 24).sum() >= 100                              # rows whose shifted first-locus field wraps to 0 or 1


def test_counts_cases_have_the_advertised_edges():
    for R in (1, 2, 4096, 4097):
        c = cases.counts_row_case(R)
        rows, loci, haps = cases.triplets_of(c)
        last = rows == R - 1
        assert len(set(zip(loci[last].tolist(), haps[last].tolist()))) >= 5
        assert 10 * (c.locus_group[loci] < 0).sum() >= len(loci)
    for N in (1, 63, 64, 65, 255, 256, 257):
        c = cases.counts_entry_case(N)
        assert c.N == N
        for h in range(c.H):
            assert c.indptr[h][3] == 0 and c.indptr[h][9] == c.indptr[h][12]
        assert c.indptr[0][5] == 0 and c.indptr[0][6] == len(c.indices[0]) > 0
    for H in (1, 16, 32):
        c = cases.counts_hap_case(H)
        assert 25_000 <= c.N <= 35_000 and (c.locus_group < 0).sum() == 10
        assert len(c.indices[H - 1]) > 0
