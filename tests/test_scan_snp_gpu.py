"""The SNP association scan on the device (gbrs_scan_set_snps / gbrs_scan_snp_dosage / gbrs_scan_snps,
GenomeScan.set_snps / snp_dosage / run_snps; needs an MI355X).  Cohorts: tests/scan_cases.py; SNP sets and
the three host computations: tests/scan_snp_cases.py.

The dosages are the restatement's bit for bit.  The LODs are held against both host routes - the numpy restatement of the
rule and np.linalg.lstsq - to ten times the difference the two have between themselves on the CPU
(scan_snp_cases.device_tol), and nothing is excluded: no SNP of the fixtures has a ratio that rounding could flip
(tests/test_scan_snp_cpu.py)."""
import numpy as np
import pytest

import scan_cases as base
import scan_snp_cases as cases

pytestmark = pytest.mark.gpu


def scan_of(case, snps=None, pieces=None, prepare=True):
    """A GenomeScan of a case with the given SNP set (default: the main set), the cohort appended in pieces."""
    from gbrs_amd.scan import GenomeScan
    D, Z, _, _ = base.build(case)
    scan = GenomeScan(case[0], case[4])
    lo = 0
    for size in pieces or [len(D)]:
        scan.append(D[lo:lo + size])
        lo += size
    assert lo == len(D) == scan.n
    grid, pos, masks, _ = snps if snps is not None else cases.main_set(case)
    scan.set_snps(grid, pos, masks)
    if prepare:
        scan.prepare(Z)
    return scan


def assert_peaks(got, lod, used, counts, tol):
    """The device's peaks against a host route's LODs: peak_lod within tol of the route's; the SNP the device names is a
    used SNP of the chromosome whose LOD by the route is the route's maximum within 2 tol (the rounding of both); and it is
    the route's own first maximum wherever the route's runner-up is more than 2 tol below.  A pattern and its complement
    at one position have equal LODs up to rounding, so which of the two leads is not the host's to say; exact ties and
    their lowest index are asserted on the device's own LODs."""
    peak, index = cases.snp_peaks(lod, used, counts)
    np.testing.assert_array_equal(got["peak_index"] < 0, index < 0)
    np.testing.assert_array_equal(np.isnan(got["peak_lod"]), np.isnan(peak))
    assert cases.deviation(np.nan_to_num(got["peak_lod"]), np.nan_to_num(peak)) <= tol
    off = np.concatenate(([0], np.cumsum(counts)))
    rows = np.arange(len(lod))
    for ci, (a, b) in enumerate(zip(off[:-1], off[1:])):
        on = a + np.flatnonzero(used[a:b])
        if len(on) == 0:
            continue
        at = got["peak_index"][:, ci]
        assert np.isin(at, on).all()
        scale = np.maximum(1.0, np.abs(peak[:, ci]))
        assert (np.abs(lod[rows, at] - peak[:, ci]) <= 2 * tol * scale).all()
        rest = lod[:, on].copy()
        rest[rows, rest.argmax(axis=1)] = -np.inf
        clear = peak[:, ci] - rest.max(axis=1) > 2 * tol * scale
        np.testing.assert_array_equal(at[clear], index[clear, ci])


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_the_device_against_the_three_host_routes(case):
    """Dosages bit for bit the restatement's, also in descending order; LODs against the rule and against lstsq within the
    case's tolerance; `used` equal to both; peaks and their indices the restatement's and, exactly, those of the device's
    own LODs; unused SNPs score exactly 0.0.  Past 256 samples the first 256 alone give other LODs."""
    H, n, c, P, points = case
    D, Z, Y, _ = base.build(case)
    grid, pos, masks, labels = cases.main_set(case)
    X, lod, used, _, lod_ls, rank = cases.expected(case)
    counts = [len(x) for x in pos]
    scan = scan_of(case, prepare=False)
    np.testing.assert_array_equal(scan.snp_dosage(), X)                           # needs no preparation
    np.testing.assert_array_equal(scan.snp_dosage(3, 11), X[:, 3:14])
    scan.prepare(Z)
    got = scan.run_snps(Y)
    info = scan.snp_info()
    scan.close()
    M_snp = sum(counts)
    assert got["lod"].shape == (P, M_snp) and got["used"].shape == (M_snp,)
    assert got["peak_lod"].shape == got["peak_index"].shape == (P, len(points))
    assert (info["M_snp"], info["P"]) == (M_snp, P) and info["chunk"] >= 64 and info["chunk"] % 64 == 0
    assert info["pass_ms"] >= info["row_ms"] > 0 and info["pass_ms"] >= info["product_ms"] > 0
    assert info["device_bytes"] >= 16 * M_snp and info["peak_device_bytes"] > info["device_bytes"]
    worst, worst_ls = cases.deviation(got["lod"], lod), cases.deviation(got["lod"], lod_ls)
    print(f"DEVIATION device SNP LODs against snp_rule {worst:.3g}, against snp_lstsq {worst_ls:.3g}, tolerance "
          f"{cases.device_tol(case):.3g}, {cases.case_id(case)}")
    np.testing.assert_array_equal(got["used"], used)
    np.testing.assert_array_equal(got["used"], rank == 1)
    assert worst <= cases.device_tol(case) and worst_ls <= cases.device_tol(case)
    assert (got["lod"] >= 0.0).all() and (got["lod"][:, ~used] == 0.0).all()
    flat = cases.flat_snps(case)
    assert len(flat) >= 3 and not got["used"][flat].any()
    for a, b in cases.complement_pairs(case):
        assert got["used"][a] == got["used"][b]
        assert cases.deviation(got["lod"][:, a], got["lod"][:, b]) <= 2 * cases.device_tol(case)
    for route in (lod, lod_ls):
        assert_peaks(got, route, used, counts, cases.device_tol(case))
    own_peak, own_index = cases.snp_peaks(got["lod"], got["used"], counts)
    np.testing.assert_array_equal(got["peak_lod"], own_peak)
    np.testing.assert_array_equal(got["peak_index"], own_index)
    flipped = cases.descending_set(case)
    back = scan_of(case, snps=flipped)
    np.testing.assert_array_equal(back.snp_dosage(), cases.snp_dosage_rule(D, points, *flipped[:3]))
    order = [flipped[3].index(label) if labels.count(label) == 1 else None for label in labels]
    turned = back.run_snps(Y)["lod"]
    back.close()
    for j, k in enumerate(order):                                                 # the same SNP, another place: the same bits
        if k is not None:
            assert np.array_equal(turned[:, k], got["lod"][:, j]), labels[j]
    if n > 256:
        from gbrs_amd.scan import GenomeScan
        head = GenomeScan(H, points)
        head.append(D[:256])
        head.set_snps(grid, pos, masks)
        head.prepare(Z[:256])
        first = head.run_snps(Y[:256])["lod"]
        head.close()
        assert first.shape == got["lod"].shape and (first != got["lod"]).any()


def test_the_row_kernel_without_lds_staging():
    """1,300 samples of 8 founders: the two grid points of a SNP are 166,400 bytes, more than a workgroup's LDS, so every
    SNP reads the cohort itself (snp_info says which way the pass went).  Dosages bit for bit, LODs within the cohort's own
    tolerance of both routes; the first 256 samples alone take the staged way, and a SNP's bits there are those of the
    cohort of 256 whichever SNPs stand beside it."""
    case = cases.DIRECT
    D, Z, Y, _ = base.build(case)
    X, lod, used, _, lod_ls, rank = cases.expected(case)
    scan = scan_of(case)
    np.testing.assert_array_equal(scan.snp_dosage(), X)
    got = scan.run_snps(Y)
    info = scan.snp_info()
    scan.close()
    assert not info["staged"]
    worst, worst_ls = cases.deviation(got["lod"], lod), cases.deviation(got["lod"], lod_ls)
    print(f"DEVIATION device SNP LODs without staging against snp_rule {worst:.3g}, against snp_lstsq {worst_ls:.3g}, tolerance "
          f"{cases.device_tol(case):.3g}, {cases.case_id(case)}")
    np.testing.assert_array_equal(got["used"], used)
    assert worst <= cases.device_tol(case) and worst_ls <= cases.device_tol(case)
    for route in (lod, lod_ls):
        assert_peaks(got, route, used, [len(x) for x in cases.main_set(case)[1]], cases.device_tol(case))
    from gbrs_amd.scan import GenomeScan
    head = GenomeScan(case[0], case[4])
    head.append(D[:256])
    head.set_snps(*cases.main_set(case)[:3])
    head.prepare(Z[:256])
    first = head.run_snps(Y[:256])
    assert head.snp_info()["staged"]
    head.close()
    assert (first["lod"] != got["lod"]).any()


TILE = (8, 70, 4, 130, (1, 65, 9))


def test_snp_sets_around_the_row_tile():
    """63, 64, 65 and 130 SNPs on one chromosome, the others without SNPs: dosages bit for bit, LODs within the case's
    tolerance of the rule, NaN and -1 peaks on the chromosomes without SNPs."""
    D, Z, Y, _ = base.build(TILE)
    for count in (63, 64, 65, 130):
        snps = cases.sized_set(TILE, count)
        X = cases.snp_dosage_rule(D, TILE[4], *snps[:3])
        lod, used, _ = cases.snp_rule(X, Z, Y)
        scan = scan_of(TILE, snps=snps)
        np.testing.assert_array_equal(scan.snp_dosage(), X)
        got = scan.run_snps(Y)
        scan.close()
        np.testing.assert_array_equal(got["used"], used)
        assert cases.deviation(got["lod"], lod) <= cases.device_tol(TILE), count
        peak, index = cases.snp_peaks(got["lod"], got["used"], [0, count, 0])
        np.testing.assert_array_equal(got["peak_index"], index)
        np.testing.assert_array_equal(got["peak_lod"], peak)
        assert (got["peak_index"][:, [0, 2]] == -1).all() and np.isnan(got["peak_lod"][:, [0, 2]]).all()


def test_a_snp_has_the_same_bits_wherever_it_stands():
    """A SNP alone, at row 0, at row 63, at row 64 and among 130; a phenotype alone and among 65; 513 phenotypes across
    the phenotype chunk; the cohort appended as 1 + rest and at once; a second run; without the LOD matrix."""
    D, Z, Y, _ = base.build(TILE)
    n = TILE[1]
    snps = cases.sized_set(TILE, 130)
    grid, pos, masks, _ = snps
    scan = scan_of(TILE, snps=snps)
    full = scan.run_snps(Y)
    again = scan.run_snps(Y)
    for key in full:
        np.testing.assert_array_equal(again[key], full[key], err_msg=key)
    lean = scan.run_snps(Y, want_lod=False)
    assert "lod" not in lean
    np.testing.assert_array_equal(lean["peak_lod"], full["peak_lod"])
    np.testing.assert_array_equal(lean["peak_index"], full["peak_index"])
    for p in (0, 5, 64):                                                          # a phenotype alone and among 65
        alone = scan.run_snps(Y[:, p])
        among = scan.run_snps(Y[:, :65])
        assert np.array_equal(alone["lod"][0], full["lod"][p]) and np.array_equal(among["lod"][p], full["lod"][p])
        assert np.array_equal(alone["peak_index"][0], full["peak_index"][p])
    wide = np.tile(Y, (1, 4))[:, :513]                                            # across the 512-column chunk
    got = scan.run_snps(wide)
    for k in range(513):
        assert np.array_equal(got["lod"][k], full["lod"][k % 130]), k
    assert np.array_equal(got["peak_index"][512], full["peak_index"][512 % 130])
    chosen = 77
    for place, total in ((0, 1), (0, 70), (63, 70), (64, 70)):                    # SNP 77 of the 130 at another row
        x, m = pos[1][:total].copy(), masks[1][:total].copy()
        x[place], m[place] = pos[1][chosen], masks[1][chosen]
        scan.set_snps(grid, [None, x, None], [None, m, None])                      # set_snps keeps the preparation
        moved = scan.run_snps(Y)
        assert np.array_equal(moved["lod"][:, place], full["lod"][:, chosen]), (place, total)
    scan.close()
    cut = scan_of(TILE, snps=snps, pieces=[1, n - 1])
    pieces = cut.run_snps(Y)
    cut.close()
    for key in full:
        np.testing.assert_array_equal(pieces[key], full[key], err_msg=f"{key}, appended as 1 + {n - 1}")


def test_the_one_hot_snp_on_a_grid_point_is_the_founder_scan():
    """H = 2: the pattern 01 on a grid point is the founder scan's only column there, so the LOD is GenomeScan.run's own
    at that point within the case's tolerance."""
    case = (2, 32, 2, 64, base.POINTS)
    _, _, Y, _ = base.build(case)
    grid = cases.grid_of(case)
    keep = [np.flatnonzero(np.concatenate(([True], g[1:] > g[:-1])) & np.concatenate((g[:-1] < g[1:], [True]))) for g in grid]
    pos = [g[k] for g, k in zip(grid, keep)]                                      # every grid point that is not duplicated
    scan = scan_of(case, snps=(grid, pos, [np.ones(len(x), dtype=np.uint32) for x in pos], None))
    by_point = scan.run(Y)["lod"]
    got = scan.run_snps(Y)
    rank = scan.info()["rank"]
    scan.close()
    off = np.concatenate(([0], np.cumsum(case[4])))
    points = np.concatenate([o + k for o, k in zip(off, keep)])
    np.testing.assert_array_equal(got["used"], rank[points] == 1)                # founder 0 is constant at two special points
    assert got["used"].sum() >= len(points) - 2
    worst = cases.deviation(got["lod"], by_point[:, points])
    print(f"DEVIATION one-hot SNPs against the founder scan at their grid points {worst:.3g}, tolerance {cases.device_tol(case):.3g}")
    assert worst <= cases.device_tol(case)


def test_the_snp_chunk_boundary():
    """L + 1 SNPs at n = 9, P = 2, L the chunk length from snp_info: the 200 SNPs around L have the bits they have when set
    alone, and their dosages are the restatement's; the chromosome that straddles L carries a planted tie across the
    boundary - the same SNP at L - 1 and at L, the best of the chromosome - and its peak is the lower index."""
    case = (8, 9, 1, 64, base.POINTS)
    D, Z, Y, _ = base.build(case)
    Y = Y[:, :2].copy()
    grid = cases.grid_of(case)
    scan = scan_of(case)
    L = scan.snp_info()["chunk"]
    rng = np.random.default_rng(29)
    x = np.sort(rng.uniform(grid[2][0], grid[2][-1], size=L + 1))
    m = rng.integers(1, 127, size=L + 1).astype(np.uint32)                        # founders 0 .. 6, never all seven of them
    a, b = L - 199, L + 1
    x[L - 1:] = x[L - 1]
    m[L - 1:] = 128                                                               # founder 7 alone: no other SNP has it
    none, no_mask = np.zeros(0), np.zeros(0, dtype=np.uint32)
    around = (grid, [none, none, x[a:b]], [no_mask, no_mask, m[a:b]], None)
    want = cases.snp_dosage_rule(D, case[4], *around[:3])
    Y[:, 0] = want[:, -1] + 0.01 * rng.normal(size=len(D))                        # phenotype 0 follows the planted SNP
    scan.set_snps(grid, [None, None, x], [None, None, m])
    full = scan.run_snps(Y)
    np.testing.assert_array_equal(scan.snp_dosage(a, b - a), want)
    scan.set_snps(*around[:3])
    alone = scan.run_snps(Y)
    scan.close()
    np.testing.assert_array_equal(full["lod"][:, a:b], alone["lod"])
    np.testing.assert_array_equal(full["used"][a:b], alone["used"])
    rule = cases.snp_rule(want, Z, Y)[0]
    assert cases.deviation(alone["lod"], rule) <= cases.device_tol(case)
    assert full["lod"][0, L - 1] == full["lod"][0, L] == full["lod"][0].max()
    assert full["peak_index"][0, 2] == L - 1 and full["peak_lod"][0, 2] == full["lod"][0, L]
    assert alone["peak_index"][0, 2] == L - 1 - a
    peak, index = cases.snp_peaks(full["lod"], full["used"], [0, 0, L + 1])
    np.testing.assert_array_equal(full["peak_index"], index)
    np.testing.assert_array_equal(full["peak_lod"], peak)


def test_every_refusal_through_the_abi():
    """Before prepare, without SNPs, a bad pattern bit, a descending grid, a SNP on a pointless chromosome, a value that is
    not finite and P = 0: GBRS_ERR_INVALID with untouched outputs and an intact handle; gbrs_scan_run and gbrs_scan_snps
    give the same bits before and after."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan, covariate_basis
    lib = _lib.load()
    case = (3, 33, 1, 65, (0, 7, 9))                                              # the first chromosome has no points
    H, n, c, P, points = case
    full = base.build((3, 33, 1, 65, base.POINTS))
    D, Z, Y = np.ascontiguousarray(full[0][:, 1:]), full[1], np.ascontiguousarray(full[2])
    rng = np.random.default_rng(3)
    grid = [np.zeros(0), np.sort(rng.uniform(0, 50, 7)), np.sort(rng.uniform(0, 50, 9))]
    pos = [np.zeros(0), rng.uniform(0, 50, 20), rng.uniform(0, 50, 20)]
    masks = [np.zeros(0, dtype=np.uint32), rng.integers(1, 7, 20).astype(np.uint32), rng.integers(1, 7, 20).astype(np.uint32)]
    scan = GenomeScan(H, points)
    scan.append(D)

    def set_snps(g, x, m):
        counts = np.array([len(a) for a in x], dtype=np.int64)
        return lib.gbrs_scan_set_snps(scan._h, _lib.ptr_table(g), _lib.ptr(counts), _lib.ptr_table(x), _lib.ptr_table(m))

    def run_snps(y, p):
        out = (np.full((max(p, 1), 40), -1.0), np.full(40, 7, dtype=np.uint8), np.full((max(p, 1), 3), -1.0),
               np.full((max(p, 1), 3), -7, dtype=np.int64))
        return lib.gbrs_scan_snps(scan._h, p, _lib.ptr(y), *[_lib.ptr(a) for a in out]), out

    def untouched(out):
        return (out[0] == -1.0).all() and (out[1] == 7).all() and (out[2] == -1.0).all() and (out[3] == -7).all()

    dosage = np.full((n, 5), -1.0)
    assert lib.gbrs_scan_snp_dosage(scan._h, 0, 5, _lib.ptr(dosage)) == _lib.GBRS_ERR_INVALID and (dosage == -1.0).all()
    assert set_snps(grid, pos, masks) == _lib.GBRS_OK
    status, out = run_snps(Y, P)
    assert status == _lib.GBRS_ERR_INVALID and b"gbrs_scan_prepare" in lib.gbrs_last_error() and untouched(out)
    scan.prepare(Z)
    status, before = run_snps(Y, P)
    assert status == _lib.GBRS_OK
    founder = scan.run(Y)
    bad = [m.copy() for m in masks]
    bad[2][4] |= np.uint32(1 << H)
    assert set_snps(grid, pos, bad) == _lib.GBRS_ERR_INVALID
    assert b"chromosome 2" in lib.gbrs_last_error() and b"SNP 4" in lib.gbrs_last_error()
    down = [g.copy() for g in grid]
    down[1][3] = down[1][2] - 1.0
    assert set_snps(down, pos, masks) == _lib.GBRS_ERR_INVALID
    assert b"chromosome 1" in lib.gbrs_last_error() and b"index 3" in lib.gbrs_last_error()
    assert set_snps(grid, [np.array([1.0])] + pos[1:], [np.array([1], dtype=np.uint32)] + masks[1:]) == _lib.GBRS_ERR_INVALID
    assert b"chromosome 0" in lib.gbrs_last_error() and b"no grid point" in lib.gbrs_last_error()
    nowhere = [x.copy() for x in pos]
    nowhere[1][0] = np.inf
    assert set_snps(grid, nowhere, masks) == _lib.GBRS_ERR_INVALID and b"not finite" in lib.gbrs_last_error()
    assert scan.snp_info()["M_snp"] == 40                                         # the handle kept what it had
    holed = Y.copy()
    holed[5, 2] = np.nan
    status, out = run_snps(holed, P)
    assert status == _lib.GBRS_ERR_INVALID and b"phenotype 2" in lib.gbrs_last_error() and untouched(out)
    status, out = run_snps(Y, 0)
    assert status == _lib.GBRS_ERR_INVALID and untouched(out)
    status, after = run_snps(Y, P)
    assert status == _lib.GBRS_OK
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    again = scan.run(Y)
    for key in founder:
        np.testing.assert_array_equal(again[key], founder[key], err_msg=key)
    assert scan.info()["c"] == c
    empty = [np.zeros(0)] * 3
    assert set_snps(grid, empty, [np.zeros(0, dtype=np.uint32)] * 3) == _lib.GBRS_OK and scan.snp_info()["M_snp"] == 0
    status, out = run_snps(Y, P)
    assert status == _lib.GBRS_ERR_INVALID and b"gbrs_scan_set_snps" in lib.gbrs_last_error() and untouched(out)
    scan.close()
