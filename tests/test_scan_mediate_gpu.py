"""The mediation pass on the device (gbrs_scan_mediate, GenomeScan.mediate; needs an MI355X).  Cohorts:
tests/scan_cases.py; targets, mediators and the two host computations: tests/scan_mediate_cases.py.

The mediated LODs are held against both host routes - the numpy restatement of the rule and np.linalg.lstsq - to ten
times the difference the two have between themselves on the CPU (scan_mediate_cases.device_tol), and nothing is excluded:
no pair of the fixtures has a guard ratio that rounding could flip (tests/test_scan_mediate_cpu.py)."""
import numpy as np
import pytest

import grid_cases
import scan_cases as base
import scan_mediate_cases as cases

pytestmark = pytest.mark.gpu


def scan_of(case, pieces=None):
    """A prepared GenomeScan of a mediation case's cohort, appended in pieces of the given sizes (default: at once)."""
    from gbrs_amd.scan import GenomeScan
    D, Z = cases.build(case)[:2]
    scan = GenomeScan(case[0], base.POINTS)
    lo = 0
    for size in pieces or [len(D)]:
        scan.append(D[lo:lo + size])
        lo += size
    assert lo == len(D) == scan.n
    scan.prepare(Z)
    return scan


def same(a, b):
    """Equal bits, NaNs included."""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_device_against_both_host_routes(case):
    """lod_med, lod0, mean and sd within the case's tolerance of the rule and of lstsq; used, n_used and best_index equal
    to the restatement's exactly; best_lod the matrix's own entries; lod0 within the scan's tolerance of run()'s LOD at the
    point.  Past 256 samples the first 256 alone give other values."""
    H, n, c, T, Q, K = case
    D, Z, tgt, pts, med, _ = cases.build(case)
    lod0, lod, used, _, lod0_ls, lod_ls, used_ls = cases.expected(case)
    tol = cases.device_tol(case)
    scan = scan_of(case)
    got = scan.mediate(tgt, pts, med, top=K, want_lod=True)
    info = scan.mediate_info()
    by_point = scan.run(tgt)["lod"][np.arange(T), pts]
    scan.close()
    assert got["lod_med"].shape == got["used"].shape == (T, Q) and got["best_index"].shape == got["best_lod"].shape == (T, K)
    assert (info["T"], info["Q"]) == (T, Q) and info["pass_ms"] >= info["product_ms"] > 0
    assert info["peak_device_bytes"] > 8 * Q * 32
    np.testing.assert_array_equal(got["used"], used)
    np.testing.assert_array_equal(got["used"], used_ls)
    assert np.isnan(got["lod_med"][~used]).all()
    worst = (cases.deviation(got["lod_med"], lod), cases.deviation(got["lod_med"], lod_ls),
             cases.deviation(got["lod0"], lod0), cases.deviation(got["lod0"], lod0_ls))
    count, mean, sd, index, best = cases.select(lod, used, K)
    own = cases.select(got["lod_med"], got["used"], K)
    moments = max(cases.deviation(got["mean"], m) for m in (mean, own[1])), max(cases.deviation(got["sd"], s) for s in (sd, own[2]))
    scan_tol = base.device_tol(cases.cohort_case(case))                           # run()'s LOD at the point: the scan's own tolerance
    against_run = cases.deviation(got["lod0"], by_point)
    print(f"DEVIATION device lod_med against mediate_rule {worst[0]:.3g}, against mediate_lstsq {worst[1]:.3g}; lod0 {worst[2]:.3g}, "
          f"{worst[3]:.3g}; mean {moments[0]:.3g}, sd {moments[1]:.3g}; lod0 against run() {against_run:.3g}; tolerance {tol:.3g}, "
          f"{cases.case_id(case)}")
    assert max(worst) <= tol and max(moments) <= tol
    assert against_run <= scan_tol
    np.testing.assert_array_equal(got["n_used"], count)
    np.testing.assert_array_equal(got["best_index"], index)
    np.testing.assert_array_equal(got["best_index"], own[3])
    assert same(got["best_lod"], own[4])
    if n > 256:
        from gbrs_amd.scan import GenomeScan
        head = GenomeScan(H, base.POINTS)
        head.append(D[:256])
        head.prepare(Z[:256])
        first = head.mediate(tgt[:256], pts, med[:256], top=K, want_lod=True)
        head.close()
        assert first["lod_med"].shape == got["lod_med"].shape
        assert (first["lod_med"][used] != got["lod_med"][used]).any() and (first["lod0"] != got["lod0"]).any()


def test_a_pair_has_the_same_bits_wherever_it_stands():
    """On the 65 x 130 case: a pair alone; the target at position 0, 8 and 64; the mediator at 0, 63 and 64; K = 1 against
    K = 5; the cohort appended as 1 + rest; the duplicated target's two rows; without the matrix; a second call."""
    case = cases.TILE
    H, n, c, T, Q, K = case
    D, Z, tgt, pts, med, planted = cases.build(case)
    scan = scan_of(case)
    full = scan.mediate(tgt, pts, med, top=5, want_lod=True)
    again = scan.mediate(tgt, pts, med, top=5, want_lod=True)
    for key in full:
        assert same(again[key], full[key]), key
    lean = scan.mediate(tgt, pts, med, top=5)
    assert "lod_med" not in lean and "used" not in lean
    for key in lean:
        assert same(lean[key], full[key]), key
    one = scan.mediate(tgt, pts, med, top=1, want_lod=True)
    assert same(one["lod_med"], full["lod_med"]) and same(one["best_lod"], full["best_lod"][:, :1])
    assert same(one["best_index"], full["best_index"][:, :1]) and same(one["mean"], full["mean"]) and same(one["sd"], full["sd"])
    assert same(full["lod_med"][5], full["lod_med"][0]) and full["lod0"][5] == full["lod0"][0]       # the same target twice
    assert same(full["best_lod"][5], full["best_lod"][0]) and same(full["best_index"][5], full["best_index"][0])
    assert full["mean"][5] == full["mean"][0] and full["sd"][5] == full["sd"][0]
    for t, q in ((0, planted["true"]), (9, 100), (64, 129)):                      # a pair alone
        alone = scan.mediate(tgt[:, t], pts[t:t + 1], med[:, q], top=1, want_lod=True)
        assert alone["lod_med"][0, 0] == full["lod_med"][t, q] and alone["lod0"][0] == full["lod0"][t]
        assert alone["used"][0, 0] and full["used"][t, q]
    chosen = 17                                                                   # target 17 at position 0, 8 and 64
    for place in (0, 8, 64):
        order = np.arange(T)
        order[place], order[chosen] = chosen, place
        moved = scan.mediate(tgt[:, order], pts[order], med, top=5, want_lod=True)
        assert same(moved["lod_med"][place], full["lod_med"][chosen]) and moved["lod0"][place] == full["lod0"][chosen], place
        assert same(moved["best_index"][place], full["best_index"][chosen]) and same(moved["best_lod"][place], full["best_lod"][chosen])
        assert moved["mean"][place] == full["mean"][chosen] and moved["sd"][place] == full["sd"][chosen], place
    chosen = 77                                                                   # mediator 77 at position 0, 63 and 64
    for place in (0, 63, 64):
        order = np.arange(Q)
        order[place], order[chosen] = chosen, place
        moved = scan.mediate(tgt, pts, med[:, order], top=0, want_lod=True)
        assert same(moved["lod_med"][:, place], full["lod_med"][:, chosen]), place
        assert same(moved["lod_med"][:, chosen], full["lod_med"][:, place]), place
    scan.close()
    cut = scan_of(case, pieces=[1, n - 1])
    pieces = cut.mediate(tgt, pts, med, top=5, want_lod=True)
    cut.close()
    for key in full:
        assert same(pieces[key], full[key]), f"{key}, appended as 1 + {n - 1}"


def test_the_target_chunk_boundary():
    """513 targets at n = 10, Q = 64: the targets pass in chunks of 512, so target 512 is a chunk of its own.  Target k is
    target k % 9 of the case, and its rows are those of the nine on their own, on either side of the boundary."""
    case = (8, 10, 1, 9, 64, 0)
    D, Z, tgt, pts, med, _ = cases.build(case)
    scan = scan_of(case)
    nine = scan.mediate(tgt, pts, med, top=3, want_lod=True)
    wide = np.arange(513) % 9
    got = scan.mediate(tgt[:, wide], pts[wide], med, top=3, want_lod=True)
    assert scan.mediate_info()["T"] == 513
    scan.close()
    for key in nine:
        assert same(got[key], nine[key][wide]), key
    assert cases.deviation(nine["lod_med"], cases.expected(case)[1]) <= cases.device_tol(case)


def test_a_mediation_leaves_the_handle_as_it_was():
    case = cases.TILE
    D, Z, tgt, pts, med, _ = cases.build(case)
    scan = scan_of(case)
    before, info = scan.run(med), scan.info()
    scan.mediate(tgt, pts, med)
    after, info_after = scan.run(med), scan.info()
    scan.close()
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    for key in ("n", "M", "H", "c", "device_bytes", "prepare_ms"):
        assert info_after[key] == info[key], key
    np.testing.assert_array_equal(info_after["rank"], info["rank"])


def test_every_refusal_through_the_abi():
    """Before prepare, T < 1, Q < 1, K < 0, K > 64, a point outside the grid, n = c + H and a value that is not finite:
    GBRS_ERR_INVALID with a message that names the entry and untouched outputs; the same call goes through afterwards."""
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    lib = _lib.load()
    case = (3, 32, 2, 8, 63, 1)
    H, n, c, T, Q, K = case
    D, Z, tgt, pts, med, _ = cases.build(case)
    tgt, pts, med = np.ascontiguousarray(tgt), np.array(pts), np.ascontiguousarray(med)
    scan = GenomeScan(H, base.POINTS)
    scan.append(D)

    def call(handle=None, t=T, q=Q, k=5, y=tgt, at=pts, z=med):
        out = (np.full(T, -1.0), np.full((T, Q), -1.0), np.full((T, Q), 7, dtype=np.uint8), np.full((T, 5), -1.0),
               np.full((T, 5), -7, dtype=np.int64), np.full(T, -1.0), np.full(T, -1.0), np.full(T, -7, dtype=np.int64))
        status = lib.gbrs_scan_mediate((handle or scan)._h, t, _lib.ptr(y), _lib.ptr(at), q, _lib.ptr(z), k,
                                       *[_lib.ptr(a) for a in out])
        kept = all((a == (-1.0 if a.dtype == np.float64 else 7 if a.dtype == np.uint8 else -7)).all() for a in out)
        return status, kept, lib.gbrs_last_error()

    def refused(needle, **how):
        status, kept, message = call(**how)
        assert status == _lib.GBRS_ERR_INVALID and kept and needle in message, (how.keys(), message)

    refused(b"call gbrs_scan_prepare first")
    scan.prepare(Z)
    refused(b"at least 1 target, got 0", t=0)
    refused(b"at least 1 mediator, got 0", q=0)
    refused(b"0..64 places, got -1", k=-1)
    refused(b"0..64 places, got 65", k=65)
    outside = pts.copy()
    outside[3] = sum(base.POINTS)
    refused(b"target 3 is at grid point 17", at=outside)
    outside[3] = -1
    refused(b"target 3 is at grid point -1", at=outside)
    holed = tgt.copy()
    holed[30, 2] = np.nan
    refused(b"target 2 holds a value that is not finite (sample 30)", y=holed)
    holed = med.copy()
    holed[4, 62] = np.inf
    refused(b"mediator 62 holds a value that is not finite (sample 4)", z=holed)
    few = GenomeScan(H, base.POINTS)
    few.append(D[:c + H])
    few.prepare(Z[:c + H])                                                        # the scan itself takes n = c + H
    refused(b"5 samples are too few to mediate with 2 covariate columns and 3 founders", handle=few, y=np.ascontiguousarray(tgt[:5]),
            z=np.ascontiguousarray(med[:5]))
    few.close()
    assert lib.gbrs_scan_mediate(None, T, _lib.ptr(tgt), _lib.ptr(pts), Q, _lib.ptr(med), 0, *[None] * 8) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_scan_mediate_info(scan._h, None) == _lib.GBRS_ERR_INVALID
    assert scan.mediate_info()["T"] == 0                                          # nothing has run yet
    with pytest.raises(ValueError, match="grid points for 8 targets"):
        scan.mediate(tgt, pts[:3], med)
    with pytest.raises(ValueError, match="mediators have shape"):
        scan.mediate(tgt, pts, med[:-1])
    status, kept, _ = call()
    assert status == _lib.GBRS_OK and not kept
    got = scan.mediate(tgt, pts, med, top=K, want_lod=True)
    scan.close()
    assert cases.deviation(got["lod_med"], cases.expected(case)[1]) <= cases.device_tol(case)


def test_mediation_on_hmm_posteriors():
    """28 samples of 8 founders on grid "a" (193 points), the dosages of the HMM's grid pass: 40 phenotypes, one of them
    planted on a founder through another; the targets are the scan's own peaks, the mediators the phenotypes.  No guard
    ratio lies in the undecided band, `used` is the restatement's, and the LODs are within ten times the restatement's own
    distance from lstsq on these pairs."""
    from gbrs_amd.scan import GenomeScan
    from test_grid_gpu import run_samples
    H = 8
    grid = grid_cases.grids()["a"]
    big, _ = run_samples(H, "do", range(25))
    small, _ = run_samples(H, "do", range(25, 28))
    for hmm in (big, small):
        hmm.set_grid(grid.positions, grid.points)
    points = big.grid_points
    assert sum(points) == 193
    D = np.concatenate([big.grid()["dosage"], small.grid()["dosage"]])
    rng = np.random.default_rng(30)
    Y = rng.normal(size=(28, 40))
    Z = np.column_stack([np.ones(28), rng.integers(0, 2, size=28)])
    Z[:2, 1] = (0.0, 1.0)
    Y[:, 3] = 4.0 * D[:, 100, 2] + 0.3 * rng.normal(size=28)                      # the mediator
    Y[:, 0] = 2.0 * Y[:, 3] + 0.2 * rng.normal(size=28)                           # what it mediates
    scan = GenomeScan(H, points)
    scan.append_from(big)
    scan.append_from(small)
    scan.prepare(Z)
    found = scan.run(Y)
    on = np.flatnonzero(np.asarray(points) > 0)
    top = on[np.argmax(found["peak_lod"][:, on], axis=1)]                         # every phenotype's best chromosome
    pts = found["peak_index"][np.arange(40), top]
    got = scan.mediate(Y, pts, Y, top=5, want_lod=True)
    scan.close()
    big.close()
    small.close()
    lod0, lod, used, ratios = cases.mediate_rule(D, Z, Y, pts, Y)
    lod0_ls, lod_ls, used_ls = cases.mediate_lstsq(D, Z, Y, pts, Y)
    assert not cases.undecided(ratios).any()
    np.testing.assert_array_equal(got["used"], used)
    np.testing.assert_array_equal(used, used_ls)
    np.testing.assert_array_equal(~used, np.eye(40, dtype=bool))                  # a target cannot mediate itself
    floor = max(cases.deviation(lod, lod_ls), cases.deviation(lod0, lod0_ls))
    worst = max(cases.deviation(got["lod_med"], lod), cases.deviation(got["lod_med"], lod_ls), cases.deviation(got["lod0"], lod0))
    print(f"DEVIATION device lod_med on HMM dosages against the host routes {worst:.3g}; the routes between themselves {floor:.3g}")
    assert worst <= cases.DEVICE_FACTOR * floor
    assert cases.deviation(got["lod0"], found["peak_lod"][np.arange(40), top]) <= base.DEVICE_FACTOR * base.MEASURED_FLOOR
    assert got["best_index"][0, 0] == 3 and got["lod0"][0] - got["best_lod"][0, 0] > 0.5 * got["lod0"][0]
    own = cases.select(got["lod_med"], got["used"], 5)
    np.testing.assert_array_equal(got["n_used"], own[0])
    np.testing.assert_array_equal(got["best_index"], own[3])
    assert same(got["best_lod"], own[4])
