"""The scan with interactive covariates on the device (gbrs_scan_int_*, GenomeScan.prepare_int / run_int; DESIGN.md §35;
needs an MI355X).  Cohorts and the two host computations: tests/scan_int_cases.py.

The device is held against both host routes - the numpy restatement of the rule and np.linalg.lstsq - to ten times the
difference the two have between themselves on the CPU, per output (scan_int_cases.device_tol); the ranks, the peaks of the
device's own matrices and every statement about bits are held with ==."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as base
import scan_int_cases as cases

pytestmark = pytest.mark.gpu

PEAK_KEYS = ("peak_full", "peak_full_index", "peak_full_add", "peak_int", "peak_int_index")


def scan_of(case, pieces=None):
    """A GenomeScan of a case after prepare_int, the cohort appended in pieces of the given sizes (default: all at once)."""
    from gbrs_amd.scan import GenomeScan
    H, n, c, k, P, points = case
    D, Z, _, _, _ = cases.build(case)
    scan = GenomeScan(H, points)
    lo = 0
    for size in pieces or [n]:
        scan.append(D[lo:lo + size])
        lo += size
    assert lo == n == scan.n
    scan.prepare_int(Z, list(range(1, 1 + k)))
    return scan


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_device_against_both_host_routes(case):
    """The three LOD matrices against the restatement and against lstsq within the case's tolerance per output; rank_full
    and rank_add equal; lod_int never negative or NaN and lod_full >= lod_add wherever both are finite; the five peak
    arrays are scan_cases.peaks of the device's own matrices and peak_full_add is lod_add at the index; the twin grid
    points carry the same bits."""
    H, n, c, k, P, points = case
    _, _, Y, _, special = cases.build(case)
    (rule, rank_full, rank_add, _), (lstsq, _, _) = cases.expected(case)
    scan = scan_of(case)
    got = scan.run_int(Y)
    info = scan.int_info()
    scan.close()
    M = sum(points)
    assert (info["n"], info["M"], info["H"], info["c"], info["k"], info["HPI"]) == (n, M, H, c, k, cases.hpi_of(case))
    n_ld = (n + 31) // 32 * 32
    assert info["prepare_ms"] > 0 and info["run_ms"] >= info["product_ms"] > 0 and info["device_bytes"] >= 8 * M * info["HPI"] * n_ld
    np.testing.assert_array_equal(info["rank_full"], rank_full)
    np.testing.assert_array_equal(info["rank_add"], rank_add)
    for key in cases.KEYS:
        assert got[key].shape == (P, M)
        worst, worst_ls = cases.deviation(got[key], rule[key]), cases.deviation(got[key], lstsq[key])
        print(f"DEVIATION {key} device against int_rule {worst:.3g}, against int_lstsq {worst_ls:.3g}, tolerance "
              f"{cases.device_tol(case, key):.3g}, {cases.case_id(case)}")
        assert worst <= cases.device_tol(case, key) and worst_ls <= cases.device_tol(case, key), key
    assert (got["lod_int"] >= 0.0).all() and (got["lod_add"] >= 0.0).all()
    fin = np.isfinite(got["lod_full"]) & np.isfinite(got["lod_add"])
    assert (got["lod_full"][fin] >= got["lod_add"][fin]).all() and not (np.isinf(got["lod_add"]) & fin).any()
    twin = special["twin"]
    for key in cases.KEYS:
        np.testing.assert_array_equal(got[key][:, twin], got[key][:, twin - 1])
    peak, index = base.peaks(got["lod_full"], points)
    np.testing.assert_array_equal(got["peak_full"], peak)
    np.testing.assert_array_equal(got["peak_full_index"], index)
    np.testing.assert_array_equal(got["peak_full_add"], got["lod_add"][np.arange(P)[:, None], index])
    peak, index = base.peaks(got["lod_int"], points)
    np.testing.assert_array_equal(got["peak_int"], peak)
    np.testing.assert_array_equal(got["peak_int_index"], index)


@pytest.mark.parametrize("case", cases.PLAIN, ids=cases.case_id)
def test_the_additive_rows_are_the_plain_scans(case):
    """lod_add == GenomeScan.run()['lod'] after prepare with the same covariates, rank_add == info()'s rank; plain run
    gives the same bits before and after prepare_int, and run_int the same before and after prepare."""
    from gbrs_amd.scan import GenomeScan
    H, n, c, k, P, points = case
    D, Z, Y, _, _ = cases.build(case)
    scan = GenomeScan(H, points)
    scan.append(D)
    scan.prepare(Z)
    before = scan.run(Y)
    rank = scan.info()["rank"]
    scan.prepare_int(Z, list(range(1, 1 + k)))
    after = scan.run(Y)
    assert_same(after, before, "plain run after prepare_int")
    got = scan.run_int(Y)
    np.testing.assert_array_equal(got["lod_add"], before["lod"])
    np.testing.assert_array_equal(scan.int_info()["rank_add"], rank)
    np.testing.assert_array_equal(scan.info()["rank"], rank)
    scan.prepare(Z[:, :1])                                                          # another plain preparation: the other one stays
    assert_same(scan.run_int(Y), got, "run_int after another prepare")
    scan.close()


@pytest.mark.parametrize("case", [cases.CASES[5], cases.CASES[11], cases.CASES[15]], ids=cases.case_id)
def test_a_phenotype_has_the_same_bits_wherever_it_stands(case):
    """Alone, at another column, a second run, and with any subset of the output pointers NULL (HPI 32 at Hp 8, 32 at Hp 16
    and 64)."""
    from gbrs_amd import _lib
    H, n, c, k, P, points = case
    _, _, Y, _, _ = cases.build(case)
    M, nc = sum(points), len(points)
    scan = scan_of(case)
    full = scan.run_int(Y)
    assert_same(scan.run_int(Y), full, "again")
    lean = scan.run_int(Y, want_lod=False)
    assert sorted(lean) == sorted(PEAK_KEYS)
    for key in PEAK_KEYS:
        np.testing.assert_array_equal(lean[key], full[key], err_msg=key)
    for p in (0, P - 1):
        alone = scan.run_int(Y[:, p])
        for key in full:
            np.testing.assert_array_equal(alone[key][0], full[key][p], err_msg=f"{key}, phenotype {p} alone")
    shift = P // 2
    moved = scan.run_int(np.roll(Y, shift, axis=1))
    for key in full:
        np.testing.assert_array_equal(moved[key], np.roll(full[key], shift, axis=0), err_msg=key)
    order = cases.KEYS + PEAK_KEYS
    Yc = np.ascontiguousarray(Y)
    for mask in range(1, 255, 7):                                                   # subsets of the eight outputs, each alone among them
        asked = [key for b, key in enumerate(order) if mask >> b & 1]
        out = {key: np.full_like(full[key], -3) for key in asked}
        assert _lib.load().gbrs_scan_int_run(scan._h, P, _lib.ptr(Yc), *[_lib.ptr(out.get(key)) for key in order]) == 0
        for key in asked:
            np.testing.assert_array_equal(out[key], full[key], err_msg=f"{key} among {asked}")
    for b, key in enumerate(order):
        out = np.full_like(full[key], -3)
        assert _lib.load().gbrs_scan_int_run(scan._h, P, _lib.ptr(Yc), *[_lib.ptr(out) if a == b else None for a in range(8)]) == 0
        np.testing.assert_array_equal(out, full[key], err_msg=f"{key} alone")
    scan.close()


def test_chunks_of_phenotypes_and_the_cut_of_the_appends_do_not_show():
    """513 phenotypes cross the 512-column chunk: each has the bits it has in the case's own run; the cohort appended one
    sample at a time gives the same bits and ranks as at once."""
    case = cases.SMALL
    H, n, c, k, P, points = case
    _, _, Y, _, _ = cases.build(case)
    wide = np.tile(Y, (1, 9))[:, :513]
    scan = scan_of(case)
    own = scan.run_int(Y)
    got = scan.run_int(wide)
    ranks = scan.int_info()
    scan.close()
    for key in own:
        np.testing.assert_array_equal(got[key], np.tile(own[key], (9, 1))[:513], err_msg=key)
    single = scan_of(case, [1] * n)
    assert_same(single.run_int(Y), own, "one sample at a time")
    for key in ("rank_full", "rank_add"):
        np.testing.assert_array_equal(single.int_info()[key], ranks[key])
    single.close()


def test_constant_and_exact_columns():
    """A constant column goes as zeros: rss0 == 0 and 0.0 in all three matrices.  A column in the span of the covariates
    and the additive columns at a point has rss_add at rounding there: lod_add is +inf or large, lod_int 0.0 where it is
    +inf, never NaN; a column in the span of the full model alone has lod_full +inf or large and lod_int with it."""
    case = cases.CASES[3]                                                           # H8-n33-c2-k1
    H, n, c, k, P, points = case
    D, Z, Y, zint, _ = cases.build(case)
    X = cases.columns(D, zint, 2)
    additive = 3.0 * X[:, 0] - 2.0 * X[:, 3] + 1.5 * Z[:, 1]
    full = additive + 2.0 * X[:, H - 1 + 2]
    y = np.column_stack([np.full(n, 3.7), Y[:, 0], additive, full, Y[:, 1]])
    scan = scan_of(case)
    got = scan.run_int(y)
    want = scan.run_int(Y[:, :2])
    scan.close()
    for key in cases.KEYS:
        assert not np.isnan(got[key]).any() and (got[key] >= 0.0).all()
        assert (got[key][0] == 0.0).all()
        np.testing.assert_array_equal(got[key][[1, 4]], want[key])
    np.testing.assert_array_equal(got["peak_full_index"][0], [0, 1, 8])             # ties: each chromosome's first point
    assert got["lod_add"][2, 2] >= 5.0 * n and got["lod_full"][2, 2] >= 5.0 * n     # rss1 below 1e-10 rss0, or +inf
    if np.isinf(got["lod_add"][2, 2]):
        assert np.isinf(got["lod_full"][2, 2]) and got["lod_int"][2, 2] == 0.0
    assert got["lod_full"][3, 2] >= 5.0 * n and np.isfinite(got["lod_add"][3, 2])
    assert got["lod_int"][3, 2] >= 5.0 * n - got["lod_add"][3, 2] - 1.0
    assert np.isinf(got["lod_int"][3, 2]) == np.isinf(got["lod_full"][3, 2])


def test_refusals_leave_the_handle_and_the_outputs_as_they_were():
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan, covariate_basis
    lib = _lib.load()
    case = cases.SMALL
    H, n, c, k, P, points = case
    D, Z, Y, zint, _ = cases.build(case)
    M, nc = sum(points), len(points)
    Yc, qz, zi = np.ascontiguousarray(Y), covariate_basis(Z), np.ascontiguousarray(zint)
    scan = GenomeScan(H, points)
    scan.append(D[:4])
    outs = [np.full((P, M), -1.0) for _ in range(3)] + [np.full((P, nc), -1.0), np.full((P, nc), -7, dtype=np.int64),
                                                        np.full((P, nc), -1.0), np.full((P, nc), -1.0), np.full((P, nc), -7, dtype=np.int64)]
    run = lambda y, cols=P: lib.gbrs_scan_int_run(scan._h, cols, _lib.ptr(y), *[_lib.ptr(a) for a in outs])
    untouched = lambda: all((a == (-7 if a.dtype == np.int64 else -1.0)).all() for a in outs)
    prepare = lambda cc, q, kk, z: lib.gbrs_scan_int_prepare(scan._h, cc, _lib.ptr(q), kk, _lib.ptr(z))
    assert run(Yc) == _lib.GBRS_ERR_INVALID and b"call gbrs_scan_int_prepare first" in lib.gbrs_last_error() and untouched()
    assert prepare(c, qz, k, zi) == _lib.GBRS_ERR_INVALID and b"4 samples are too few" in lib.gbrs_last_error()     # n <= c + Hx (1 + k)
    scan.append(D[4:])
    assert prepare(c, qz, 0, zi) == _lib.GBRS_ERR_INVALID and b"at least 1" in lib.gbrs_last_error()
    assert prepare(0, qz, k, zi) == _lib.GBRS_ERR_INVALID and prepare(65, qz, k, zi) == _lib.GBRS_ERR_INVALID
    bad = qz.copy()
    bad[20, 1] = np.inf
    assert prepare(c, bad, k, zi) == _lib.GBRS_ERR_INVALID and b"sample 20, column 1" in lib.gbrs_last_error()
    bad = zi.copy()
    bad[7, 0] = np.nan
    assert prepare(c, qz, k, bad) == _lib.GBRS_ERR_INVALID and b"interactive covariate 0 holds a value that is not finite (sample 7)" in lib.gbrs_last_error()
    assert scan.int_info()["c"] == 0 and scan.int_info()["rank_full"] is None and scan.int_info()["device_bytes"] == 0
    wide = GenomeScan(17, points)                                                   # 16 + 4 x 16 rows: more than 64
    assert lib.gbrs_scan_int_prepare(wide._h, c, _lib.ptr(qz), 4, _lib.ptr(np.ones((n, 4)))) == _lib.GBRS_ERR_UNSUPPORTED
    wide.close()
    for interactive, message in (([0], "intercept"), ([1, 1], "twice"), ([2], "not a column"), ([], "no interactive")):
        with pytest.raises(ValueError, match=message):
            scan.prepare_int(Z, interactive)
    scan.prepare_int(Z, [1])
    want = scan.run_int(Y)
    for cc, q, kk, z in ((65, qz, k, zi), (c, qz, 0, zi), (c, qz, k, bad)):         # refused prepares keep the preparation
        assert prepare(cc, q, kk, z) == _lib.GBRS_ERR_INVALID
    assert scan.int_info()["c"] == c and scan.int_info()["k"] == k
    y = Yc.copy()
    y[30, 2] = -np.inf
    assert run(y) == _lib.GBRS_ERR_INVALID and b"phenotype 2 holds a value that is not finite (sample 30)" in lib.gbrs_last_error()
    assert untouched() and run(Yc, 0) == _lib.GBRS_ERR_INVALID and untouched()
    assert lib.gbrs_scan_int_run(None, P, _lib.ptr(Yc), *[None] * 8) == _lib.GBRS_ERR_INVALID
    assert run(Yc) == _lib.GBRS_OK and not untouched()
    for a, key in zip(outs, cases.KEYS + PEAK_KEYS):
        np.testing.assert_array_equal(a, want[key], err_msg=key)
    scan.append(D[:1])                                                              # an append drops the preparation
    for a in outs:
        a[...] = -7 if a.dtype == np.int64 else -1.0
    assert not scan.int_prepared and scan.int_info()["c"] == 0 and scan.int_info()["device_bytes"] == 0
    assert run(np.ascontiguousarray(np.vstack([Y, Y[:1]]))) == _lib.GBRS_ERR_INVALID and untouched()
    scan.close()
