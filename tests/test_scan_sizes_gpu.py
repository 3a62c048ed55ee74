"""The genome scan on the device at size (needs an MI355X): what only a cohort past the
256-thread stride of scan_prepare_kernel's per-sample solve, a permutation pass of more than eight 512-column chunks or
the covariate limit reaches, beside the comparisons of scan_cases.LARGE_CASES with both host routes in test_scan_gpu.py
and test_scan_perm_gpu.py.  Everything here is bit equality, except the maxima of the event ring's pass."""
import numpy as np
import pytest

import scan_cases as cases
import scan_perm_restate as restate
from test_scan_gpu import scan_of

pytestmark = pytest.mark.gpu

SIZE = (8, 257, 2, 65, cases.POINTS)       # one sample past the solve's stride and past the rank kernel's tile; 9 K chunks
LIMIT = (8, 130, 64, 64, cases.POINTS)     # c = SC_MAX_C


def test_the_same_bits_at_size():
    """257 samples: a phenotype alone and among 65; the cohort appended as 256 + 1, as 100 + 157 and at once; three
    permutations and the first three of five."""
    assert SIZE in cases.LARGE_CASES
    _, _, Y, _ = cases.build(SIZE)
    whole = scan_of(SIZE)
    full = whole.run(Y)
    rank = whole.info()["rank"]
    for p in (0, 5, 63, 64):
        alone = whole.run(Y[:, p])
        for key in full:
            np.testing.assert_array_equal(alone[key][0], full[key][p], err_msg=f"{key}, phenotype {p} alone")
    five = whole.permute(Y, 5, seed=restate.SEED, want_index=True)
    three = whole.permute(Y, 3, seed=restate.SEED, want_index=True)
    np.testing.assert_array_equal(three["perm_max"], five["perm_max"][:, :3])
    np.testing.assert_array_equal(three["perm_index"], five["perm_index"][:3])
    np.testing.assert_array_equal(whole.permute(Y[:, 64], 5, seed=restate.SEED)["perm_max"][0], five["perm_max"][64])
    whole.close()
    for pieces in ([256, 1], [100, 157]):
        cut = scan_of(SIZE, pieces)
        got = cut.run(Y)
        np.testing.assert_array_equal(cut.info()["rank"], rank, err_msg=f"rank, pieces {pieces}")
        for key in full:
            np.testing.assert_array_equal(got[key], full[key], err_msg=f"{key}, pieces {pieces}")
        np.testing.assert_array_equal(cut.permute(Y, 3, seed=restate.SEED)["perm_max"], three["perm_max"], err_msg=f"pieces {pieces}")
        cut.close()


def test_a_pass_that_wraps_the_event_ring():
    """Nine phenotypes under 512 permutations are 4,608 columns in nine chunks of 512: from the ninth on, a chunk waits for
    the pair of events its slot held eight chunks before and reads it.  The permutations are the restatement's, every
    maximum is held against both host routes at the device factor of what the two differ by on these very columns
    (scan_perm_restate.MEASURED_RING), the first seven permutations have the bits of a pass of seven, the product time is
    that of all nine chunks, and run() returns the same bits before and after."""
    case, P, B = restate.RING, restate.RING_PHENO, restate.RING_PERM
    assert P * B > 8 * 512
    _, _, Y, _ = cases.build(case)
    perm, rule, lstsq = restate.expected_ring()
    by_rule, by_lstsq = (restate.masked_max(lod, case[4]).reshape(P, B) for lod in (rule, lstsq))
    scan = scan_of(case)
    before = scan.run(Y)
    got = scan.permute(Y[:, :P], B, seed=restate.SEED, want_index=True)
    timing = scan.perm_info()
    after = scan.run(Y)
    seven = scan.permute(Y[:, :P], 7, seed=restate.SEED)["perm_max"]
    short = scan.perm_info()
    scan.close()
    np.testing.assert_array_equal(got["perm_index"], perm)
    assert got["perm_max"].shape == (P, B)
    np.testing.assert_array_equal(got["perm_max"][:, :7], seven)
    tol = cases.DEVICE_FACTOR * restate.MEASURED_RING
    worst, worst_ls = cases.deviation(got["perm_max"], by_rule), cases.deviation(got["perm_max"], by_lstsq)
    print(f"DEVIATION device perm_max of the event ring's pass against scan_rule {worst:.3g}, against scan_lstsq {worst_ls:.3g}, "
          f"tolerance {tol:.3g}; product {timing['product_ms']:.3g} ms of {timing['permute_ms']:.3g} ms, a pass of 7: "
          f"{short['product_ms']:.3g} ms")
    assert worst <= tol and worst_ls <= tol
    assert (timing["P"], timing["B"]) == (P, B) and (short["P"], short["B"]) == (P, 7)
    assert timing["product_ms"] > 0 and timing["permute_ms"] >= timing["product_ms"]
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)


def test_the_covariate_limit_through_the_abi():
    """130 samples: gbrs_scan_prepare takes 64 covariate columns and refuses 65, and the preparation of 64 survives the
    refusal - gbrs_scan_run returns the same bits before and after it, those held against the restatement."""
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan, covariate_basis
    lib = _lib.load()
    H, n, c, P, points = LIMIT
    assert LIMIT in cases.LARGE_CASES
    D, Z, Y, _ = cases.build(LIMIT)
    q64 = covariate_basis(Z)
    q65 = covariate_basis(np.column_stack([Z, np.random.default_rng(65).normal(size=n)]))
    assert q64.shape == (n, 64) and q65.shape == (n, 65)
    Yc = np.ascontiguousarray(Y)
    scan = GenomeScan(H, points)
    scan.append(D)

    def run():
        lod, peak, index = np.full((P, sum(points)), -1.0), np.full((P, len(points)), -1.0), np.full((P, len(points)), -7, dtype=np.int64)
        assert lib.gbrs_scan_run(scan._h, P, _lib.ptr(Yc), _lib.ptr(lod), _lib.ptr(peak), _lib.ptr(index)) == _lib.GBRS_OK
        return lod, peak, index

    assert lib.gbrs_scan_prepare(scan._h, 65, _lib.ptr(q65)) == _lib.GBRS_ERR_INVALID
    assert b"covariate columns must be 1..64" in lib.gbrs_last_error() and b"got 65" in lib.gbrs_last_error()
    assert scan.info()["c"] == 0
    assert lib.gbrs_scan_prepare(scan._h, 64, _lib.ptr(q64)) == _lib.GBRS_OK
    before, rank = run(), scan.info()["rank"]
    assert lib.gbrs_scan_prepare(scan._h, 65, _lib.ptr(q65)) == _lib.GBRS_ERR_INVALID
    assert b"covariate columns must be 1..64" in lib.gbrs_last_error()
    assert scan.info()["c"] == 64
    np.testing.assert_array_equal(scan.info()["rank"], rank)
    after = run()
    scan.close()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    want, want_rank = cases.expected(LIMIT)[:2]
    np.testing.assert_array_equal(rank, want_rank)
    assert cases.deviation(before[0], want) <= cases.device_tol(LIMIT)
