"""Founder effects and LOD support intervals on the device (gbrs_scan_effects, gbrs_scan_run_support, GenomeScan.effects,
GenomeScan.run(lod_drop=...); needs an MI355X).  Cohorts: tests/scan_cases.py; targets and the host
computations: tests/scan_effects_cases.py.

The effects are held against both host routes - the numpy restatement of the rule and the SVD route - to ten times the
difference the two have between themselves on the CPU (scan_effects_cases.device_tol).  The intervals are held against
the numpy restatement applied to the device's own LODs, which needs no tolerance."""
import numpy as np
import pytest

import scan_cases as base
import scan_effects_cases as cases

pytestmark = pytest.mark.gpu


def scan_of(case, pieces=None):
    """A prepared GenomeScan of an effects case's cohort, appended in pieces of the given sizes (default: at once)."""
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
    """Equal bits."""
    return np.array_equal(a, b, equal_nan=True)


KEYS = ("effect", "se", "lod", "sigma2", "rank")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_device_against_both_host_routes(case):
    """effect, se, lod and sigma2 within the case's tolerance of the rule and of the SVD route; rank equal to info()'s at the
    target's point; lod within the scan's own tolerance of run()'s LOD at (column, point); and what the planted targets
    are there to show, exactly."""
    H, n, c, T = case
    D, Z, pheno, columns, points, planted = cases.build(case)
    rule, svd, _ = cases.expected(case)
    scan = scan_of(case)
    got = scan.effects(pheno, columns, points)
    info = scan.effects_info()
    by_point = scan.run(pheno)["lod"][columns, points]
    ranks = scan.info()["rank"]
    scan.close()
    assert got["effect"].shape == got["se"].shape == (T, H) and got["lod"].shape == got["sigma2"].shape == got["rank"].shape == (T,)
    assert (info["T"], info["P"]) == (T, pheno.shape[1]) and info["pass_ms"] > 0 and info["peak_device_bytes"] > 8 * D.size
    np.testing.assert_array_equal(got["rank"], ranks[points])
    np.testing.assert_array_equal(got["rank"], rule["rank"])
    assert np.isfinite(got["effect"]).all() and np.isfinite(got["se"]).all() and (got["se"] >= 0).all() and (got["sigma2"] >= 0).all()
    worst = {}
    for key in cases.KEYS:
        on = cases.judged(case, key)
        worst[key] = max(cases.deviation(got[key][on], rule[key][on]), cases.deviation(got[key][on], svd[key][on]))
    on = cases.judged(case, "lod")
    against_run = cases.deviation(got["lod"][on], by_point[on])
    print("DEVIATION device against the host routes " + ", ".join(f"{k} {v:.3g} (tolerance {cases.device_tol(case, k):.3g})"
                                                                  for k, v in worst.items()) +
          f"; lod against run() {against_run:.3g}; {cases.case_id(case)}")
    for key, value in worst.items():
        assert value <= cases.device_tol(case, key), key
    assert against_run <= cases.run_tol(case)
    full = got["rank"] == H - 1
    total = np.abs(got["effect"][full].sum(axis=1)) / np.maximum(1.0, np.abs(got["effect"][full]).max(axis=1))
    assert total.max() <= H * cases.device_tol(case, "effect")
    if planted:
        t = planted["zero"]
        assert got["effect"][t, 0] == 0.0 and got["se"][t, 0] == 0.0                # no dosage: exactly nothing
        if H >= 3:
            t = planted["equal"]
            assert got["effect"][t, 0] == got["effect"][t, 1] and got["se"][t, 0] == got["se"][t, 1]
        else:
            assert got["rank"][t] == 0 and not got["effect"][t].any() and not got["se"][t].any()
        t = planted["constant"]
        assert not got["effect"][t].any() and not got["se"][t].any() and got["lod"][t] == 0.0 and got["sigma2"][t] == 0.0
        for key in KEYS:
            assert same(got[key][planted["twice"]], got[key][0]), key
        t = planted["exact"]
        assert got["lod"][t] >= cases.exact_lod_bound(n) and got["sigma2"][t] <= cases.EXACT_SHARE * (pheno[:, columns[t]] ** 2).sum()
    if n > 256:                                                                     # past 256 samples the first 256 alone give other values
        from gbrs_amd.scan import GenomeScan
        head = GenomeScan(H, base.POINTS)
        head.append(D[:256])
        head.prepare(Z[:256])
        first = head.effects(pheno[:256], columns, points)
        head.close()
        assert cases.deviation(first["effect"], rule["effect"]) > cases.device_tol(case, "effect")
        assert cases.deviation(first["sigma2"], rule["sigma2"]) > cases.device_tol(case, "sigma2")


def test_a_target_has_the_same_bits_wherever_it_stands():
    """On the 65-target case: a target alone; first and last in the list; its column at position 0 and 64 of P = 130; the
    cohort appended as 1 + rest, as 3 pieces and at once; the same target twice; a second call."""
    case = cases.TILE
    H, n, c, T = case
    D, Z, pheno, columns, points, planted = cases.build(case)
    scan = scan_of(case)
    full = scan.effects(pheno, columns, points)
    again = scan.effects(pheno, columns, points)
    for key in KEYS:
        assert same(again[key], full[key]), key
        assert same(full[key][planted["twice"]], full[key][0]), key
    for t in (0, planted["zero"], 17, 64):                                          # alone
        alone = scan.effects(pheno, columns[t:t + 1], points[t:t + 1])
        for key in KEYS:
            assert same(alone[key][0], full[key][t]), (key, t)
    chosen = 17                                                                     # first and last in the list
    for place in (0, 64):
        order = np.arange(T)
        order[place], order[chosen] = chosen, place
        moved = scan.effects(pheno, columns[order], points[order])
        for key in KEYS:
            assert same(moved[key][place], full[key][chosen]), (key, place)
            assert same(moved[key], full[key][order]), (key, place)
    wide = np.tile(pheno[:, :13], (1, 10))                                          # P = 130: column 3 at positions 0 and 64
    ordinary = columns < 13
    for place in (0, 64):
        table = wide.copy()
        table[:, [place, 3]] = table[:, [3, place]]
        where = np.where(columns == 3, place, np.where(columns == place, 3, columns))
        moved = scan.effects(table, where[ordinary], points[ordinary])
        assert scan.effects_info()["P"] == 130
        for key in KEYS:
            assert same(moved[key], full[key][ordinary]), (key, place)
    scan.close()
    for pieces in ([1, n - 1], [20, 30, n - 50]):
        cut = scan_of(case, pieces=pieces)
        got = cut.effects(pheno, columns, points)
        cut.close()
        for key in KEYS:
            assert same(got[key], full[key]), f"{key}, appended as {pieces}"


def test_the_target_chunk_boundary():
    """513 targets: the targets pass in chunks of 512, so target 512 is a chunk of its own.  It is given again as target 3
    and as target 511, and alone: the same bits on either side of the boundary."""
    case = cases.CHUNK
    D, Z, pheno, columns, points, _ = cases.build(case)
    columns, points = columns.copy(), points.copy()
    columns[[3, 511]], points[[3, 511]] = columns[512], points[512]
    scan = scan_of(case)
    got = scan.effects(pheno, columns, points)
    assert scan.effects_info()["T"] == 513
    alone = scan.effects(pheno, columns[512:], points[512:])
    head = scan.effects(pheno, columns[:512], points[:512])
    scan.close()
    for key in KEYS:
        assert same(got[key][512], got[key][3]) and same(got[key][512], got[key][511]) and same(got[key][512], alone[key][0]), key
        assert same(got[key][:512], head[key]), key


def test_the_effects_leave_the_handle_as_it_was():
    case = cases.TILE
    D, Z, pheno, columns, points, _ = cases.build(case)
    scan = scan_of(case)
    before, info = scan.run(pheno), scan.info()
    scan.effects(pheno, columns, points)
    after, info_after = scan.run(pheno), scan.info()
    scan.close()
    for key in before:
        assert same(after[key], before[key]), key
    for key in ("n", "M", "H", "c", "device_bytes", "prepare_ms"):
        assert info_after[key] == info[key], key
    np.testing.assert_array_equal(info_after["rank"], info["rank"])


# ---- intervals -------------------------------------------------------------------------------------------------------------------

DROPS = (0.0, 1.5, 1e6)


@pytest.mark.parametrize("case", base.CASES, ids=base.case_id)
def test_the_intervals_against_the_rule_on_the_devices_own_lods(case):
    """Every scan case with every drop: lod, peak_lod and peak_index the bits of the plain run, support_lo and support_hi the
    restatement's on the device's LODs.  Phenotype 0 peaks on the `twin` tie; chromosome 0 has one point; one case has a
    chromosome of 65 points."""
    from gbrs_amd.scan import GenomeScan
    H, n, c, P, points = case
    D, Z, Y, special = base.build(case)
    scan = GenomeScan(H, points)
    scan.append(D)
    scan.prepare(Z)
    plain = scan.run(Y)
    assert sorted(plain) == ["lod", "peak_index", "peak_lod"]
    off = np.concatenate(([0], np.cumsum(points)))
    for drop in DROPS:
        got = scan.run(Y, lod_drop=drop)
        for key in plain:
            assert same(got[key], plain[key]), (key, drop)
        peak, lo, hi = cases.support_rule(plain["lod"], points, drop)
        np.testing.assert_array_equal(peak, plain["peak_index"])
        np.testing.assert_array_equal(got["support_lo"], lo, err_msg=f"drop {drop}")
        np.testing.assert_array_equal(got["support_hi"], hi, err_msg=f"drop {drop}")
        assert (got["support_lo"][:, 0] == 0).all() and (got["support_hi"][:, 0] == 0).all()       # the one-point chromosome
        assert (got["support_lo"] >= off[:-1]).all() and (got["support_hi"] < off[1:]).all()
        assert (got["support_lo"] <= plain["peak_index"]).all() and (got["support_hi"] >= plain["peak_index"]).all()
        lean = scan.run(Y, want_lod=False, lod_drop=drop)
        assert "lod" not in lean and same(lean["support_lo"], lo) and same(lean["support_hi"], hi)
    if n > c + H:                                                                   # phenotype 0 peaks on the tie
        tie = plain["peak_index"][0, -1]
        assert tie == special["twin"] - 1 and plain["lod"][0, tie] == plain["lod"][0, tie + 1]
        assert scan.run(Y, lod_drop=1.5)["support_hi"][0, -1] > tie + 1             # the twin has not fallen: it is the peak's equal
        assert scan.run(Y, lod_drop=0.0)["support_hi"][0, -1] == tie + 1            # without a drop it has
    scan.close()


def test_the_intervals_past_the_phenotype_chunk():
    """P = 513 on the 65-point chromosome's cohort: phenotype 512 is a chunk of its own."""
    from gbrs_amd.scan import GenomeScan
    case = (8, 70, 4, 130, (1, 65, 9))
    H, n, c, P, points = case
    D, Z, Y, _ = base.build(case)
    wide = Y[:, np.arange(513) % P]
    scan = GenomeScan(H, points)
    scan.append(D)
    scan.prepare(Z)
    plain = scan.run(wide)
    got = scan.run(wide, lod_drop=1.5)
    scan.close()
    for key in plain:
        assert same(got[key], plain[key]), key
    peak, lo, hi = cases.support_rule(plain["lod"], points, 1.5)
    np.testing.assert_array_equal(got["support_lo"], lo)
    np.testing.assert_array_equal(got["support_hi"], hi)
    assert same(got["support_lo"][512], got["support_lo"][512 % P]) and same(got["support_hi"][512], got["support_hi"][512 % P])


@pytest.mark.parametrize("side", ["lo", "hi"])
def test_an_interval_end_more_than_one_step_from_the_peak(side):
    """The plateau fixture: the LOD has fallen 73 points from the peak and nowhere nearer, so the walk takes two 64-point
    steps on that side, and the point it finds is not the chromosome's end, which a walk that gave up after one step would
    report; on the other side the peak is the chromosome's end."""
    from gbrs_amd.scan import GenomeScan
    D, Z, Y = cases.plateau(side)
    scan = GenomeScan(D.shape[2], cases.PLATEAU_POINTS)
    scan.append(D)
    scan.prepare(Z)
    got = scan.run(Y, lod_drop=cases.PLATEAU_DROP)
    scan.close()
    peak, lo, hi = cases.support_rule(got["lod"], cases.PLATEAU_POINTS, cases.PLATEAU_DROP)
    k, want_lo, want_hi = cases.PLATEAU_WANT[side]
    assert (peak.tolist(), lo.tolist(), hi.tolist()) == ([[k]], [[want_lo]], [[want_hi]])      # what the fixture is built to give
    assert got["peak_index"].tolist() == [[k]]
    assert got["support_lo"].tolist() == [[want_lo]] and got["support_hi"].tolist() == [[want_hi]]
    assert max(k - want_lo, want_hi - k) == 73 and 0 < (want_lo if side == "lo" else want_hi) < 74


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_every_refusal_through_the_abi():
    """Before prepare, P < 1, T < 1, a column or a point out of range, a value that is not finite, a negative or NaN drop:
    GBRS_ERR_INVALID with a message that names the entry, untouched outputs and an unchanged handle; the same calls go
    through afterwards."""
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    lib = _lib.load()
    case = (3, 32, 2, 9)
    H, n, c, T = case
    D, Z, pheno, columns, points, _ = cases.build(case)
    pheno, columns, points = np.ascontiguousarray(pheno), np.array(columns), np.array(points)
    P, M, nc = pheno.shape[1], sum(base.POINTS), len(base.POINTS)
    scan = GenomeScan(H, base.POINTS)
    scan.append(D)

    def effects(p=P, t=T, y=pheno, col=columns, at=points):
        out = (np.full((T, H), -1.0), np.full((T, H), -1.0), np.full(T, -1.0), np.full(T, -1.0), np.full(T, -7, dtype=np.int32))
        status = lib.gbrs_scan_effects(scan._h, p, _lib.ptr(y), t, _lib.ptr(col), _lib.ptr(at), *[_lib.ptr(a) for a in out])
        kept = all((a == (-1.0 if a.dtype == np.float64 else -7)).all() for a in out)
        return status, kept, lib.gbrs_last_error()

    def support(drop=1.5, p=P, y=pheno):
        out = (np.full((P, M), -1.0), np.full((P, nc), -1.0), np.full((P, nc), -7, dtype=np.int64), np.full((P, nc), -7, dtype=np.int64),
               np.full((P, nc), -7, dtype=np.int64))
        status = lib.gbrs_scan_run_support(scan._h, p, _lib.ptr(y), drop, *[_lib.ptr(a) for a in out])
        kept = all((a == (-1.0 if a.dtype == np.float64 else -7)).all() for a in out)
        return status, kept, lib.gbrs_last_error()

    def refused(call, needle, **how):
        status, kept, message = call(**how)
        assert status == _lib.GBRS_ERR_INVALID and kept and needle in message, (how.keys(), message)

    refused(effects, b"call gbrs_scan_prepare first")
    refused(support, b"call gbrs_scan_prepare first")
    scan.prepare(Z)
    before, info = scan.run(pheno), scan.info()
    refused(effects, b"at least 1 phenotype, got 0", p=0)
    refused(effects, b"at least 1 target, got 0", t=0)
    outside = columns.copy()
    outside[4] = P
    refused(effects, b"target 4 is phenotype column 18: the table has the columns 0 .. 17", col=outside)
    outside[4] = -1
    refused(effects, b"target 4 is phenotype column -1", col=outside)
    outside = points.copy()
    outside[3] = M
    refused(effects, b"target 3 is at grid point 17: the handle has the points 0 .. 16", at=outside)
    outside[3] = -2
    refused(effects, b"target 3 is at grid point -2", at=outside)
    holed = pheno.copy()
    holed[30, 2] = np.nan
    refused(effects, b"phenotype 2 holds a value that is not finite (sample 30)", y=holed)
    refused(support, b"phenotype 2 holds a value that is not finite (sample 30)", y=holed)
    holed[30, 2] = -np.inf
    refused(effects, b"phenotype 2 holds a value that is not finite (sample 30)", y=holed)
    refused(support, b"finite number that is not negative, got -0.5", drop=-0.5)
    refused(support, b"finite number that is not negative, got nan", drop=float("nan"))
    refused(support, b"finite number that is not negative, got inf", drop=float("inf"))
    refused(support, b"bad argument", p=0)
    assert lib.gbrs_scan_effects(None, P, _lib.ptr(pheno), T, _lib.ptr(columns), _lib.ptr(points), *[None] * 5) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_scan_effects_info(scan._h, None) == _lib.GBRS_ERR_INVALID
    assert scan.effects_info()["T"] == 0                                            # nothing has run yet
    with pytest.raises(ValueError, match="phenotype columns and"):
        scan.effects(pheno, columns, points[:3])
    with pytest.raises(ValueError, match="phenotypes have shape"):
        scan.effects(pheno[:-1], columns, points)
    after, info_after = scan.run(pheno), scan.info()                                # the refusals left the handle as it was
    for key in before:
        assert same(after[key], before[key]), key
    for key in ("n", "M", "H", "c", "device_bytes", "prepare_ms"):
        assert info_after[key] == info[key], key
    status, kept, _ = effects()
    assert status == _lib.GBRS_OK and not kept
    status, kept, _ = support()
    assert status == _lib.GBRS_OK and not kept
    assert lib.gbrs_scan_effects(scan._h, P, _lib.ptr(pheno), T, _lib.ptr(columns), _lib.ptr(points), *[None] * 5) == _lib.GBRS_OK
    got = scan.effects(pheno, columns, points)
    scan.close()
    assert cases.deviation(got["effect"], cases.expected(case)[0]["effect"]) <= cases.device_tol(case, "effect")
