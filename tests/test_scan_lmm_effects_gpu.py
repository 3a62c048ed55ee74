"""Founder effects and LOD support intervals under the mixed model on the device (gbrs_scan_lmm_effects,
gbrs_scan_lmm_run_support, GenomeScan.effects_lmm / run_lmm(lod_drop=...); needs an MI355X) against the two
host routes of tests/scan_lmm_effects_cases.py, each fed the device's own heritabilities, at ten times each case's recorded
floor; the LOD and the heritability of a target against run_lmm's with ==; the bit equalities, the intervals against
scan_effects_cases.support_rule on the device's own LODs, the refusals and the files of the two commands."""
import functools
import os

import numpy as np
import pytest

import grid_cases
import scan_effects_cases as plain
import scan_lmm_cases as lmm
import scan_lmm_effects_cases as cases
import scan_lmm_snp_cases as snp_cases
from test_scan_gpu import H_FILES, N_FILES, GRID_FILES, STYLE_FILES, cohort_files, tables, write_table  # noqa: F401
from test_scan_lmm_gpu import kinship_argument, open_scan, write_cohort

pytestmark = pytest.mark.gpu

BITS = lmm.CASES[1]                        # H8-n70-c2-P65: the case of the bit equalities
OUT = ("effect", "se", "lod", "sigma2", "hsq", "rank")
RUN = ("lod", "peak_lod", "peak_index", "hsq", "sigma2", "rank_min", "rank_max")


def scan_of(case, split=None):
    scan = open_scan(case, split)
    scan.prepare_lmm(lmm.build(case)[1], kinship_argument(case))
    return scan


@functools.lru_cache(maxsize=None)
def device(case):
    """(run_lmm fitted, run_lmm given, effects_lmm fitted, effects_lmm given) of a case's table (its P phenotypes and the
    exact column) and targets, computed once; `given` hands the fitted heritabilities back."""
    pheno, columns, at, _ = cases.build(case)
    scan = scan_of(case)
    run = scan.run_lmm(pheno)
    fitted = scan.effects_lmm(pheno, columns, at)
    info = scan.lmm_effects_info()
    run_given = scan.run_lmm(pheno, hsq=run["hsq"])
    given = scan.effects_lmm(pheno, columns, at, hsq=run["hsq"])
    scan.close()
    assert (info["T"], info["P"], info["columns"]) == (len(columns), pheno.shape[1], len(set(columns.tolist())))
    assert info["pass_ms"] >= info["null_ms"] > 0 and info["target_ms"] > 0 and info["peak_device_bytes"] > 0
    out = (run, run_given, fitted, given)
    for d in out:
        for a in d.values():
            a.setflags(write=False)
    return out


def same(a, b, rows=slice(None), note=""):
    for key in OUT:
        np.testing.assert_array_equal(a[key], b[key][rows], err_msg=f"{key} {note}")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_effects_against_both_host_routes_at_the_devices_heritabilities(case):
    H, n, cz, P, points, _ = case
    pheno, columns, at, planted = cases.build(case)
    run, run_given, fitted, given = device(case)
    kin_of_chrom = lmm.build(case)[4]
    chrom = np.array([cases.chrom_of(points, m) for m in at])
    first = [list(kin_of_chrom).index(e) for e in range(max(kin_of_chrom) + 1)]
    rule, gls, shares = cases.both_routes(case, run["hsq"][:, first])
    assert not ((shares > cases.SVD_UNDECIDED[0]) & (shares < cases.SVD_UNDECIDED[1])).any()
    np.testing.assert_array_equal(rule["rank"], gls["rank"])
    for name, got, scan in (("fitted", fitted, run), ("given", given, run_given)):
        for route, want in (("rule", rule), ("gls", gls)):
            for key in cases.KEYS:
                on = cases.judged(case, key)
                measured = cases.deviation(got[key][on], want[key][on])
                print(f"{cases.case_id(case)} {name} {key} vs {route}: {measured:.3g}, tolerance {cases.device_tol(case, key):.3g}")
                assert measured <= cases.device_tol(case, key), (name, route, key)
        np.testing.assert_array_equal(got["rank"], rule["rank"])
        # the same wavefront sums as the scan's: its bits
        np.testing.assert_array_equal(got["lod"], scan["lod"][columns, at], err_msg=name)
        np.testing.assert_array_equal(got["hsq"], scan["hsq"][columns, chrom], err_msg=name)
        assert ((got["rank"] >= scan["rank_min"][columns]) & (got["rank"] <= scan["rank_max"][columns])).all()
        t = planted["zero"]
        assert got["effect"][t, 0] == 0.0 and got["se"][t, 0] == 0.0
        if "equal" in planted:
            t = planted["equal"]
            assert got["effect"][t, 0] == got["effect"][t, 1] and got["se"][t, 0] == got["se"][t, 1]
        else:                                                                       # H = 2: the one kept column is zeros
            assert got["rank"][t] == 0 and not got["effect"][t].any() and not got["se"][t].any() and got["lod"][t] == 0.0
        full = got["rank"] == H - 1
        assert np.abs(got["effect"][full].sum(axis=1)).max() <= 1e-9 * max(1.0, np.abs(got["effect"][full]).max())
        t = planted["exact"]
        assert np.isfinite(got["se"][t]).all() and got["lod"][t] >= cases.exact_lod_bound(n)
        assert got["sigma2"][t] <= cases.EXACT_SHARE * cases.whitened_size(case)
    same(given, fitted, note="given the fitted heritabilities")
    for key in RUN:
        np.testing.assert_array_equal(run_given[key], run[key], err_msg=key)


def test_a_constant_column_gives_zeros():
    case = lmm.CASES[8]
    pheno, columns, at, _ = cases.build(case)
    table = np.column_stack([pheno, np.full(len(pheno), 2.5)])
    scan = scan_of(case)
    got = scan.effects_lmm(table, [table.shape[1] - 1, 0], [3, 3])
    scan.close()
    assert got["hsq"][0] == 0.0 and got["lod"][0] == 0.0 and got["sigma2"][0] == 0.0
    assert not got["effect"][0].any() and not got["se"][0].any() and got["effect"][1].any()


def test_a_target_has_the_same_bits_alone_among_others_twice_and_at_any_place():
    pheno, columns, at, planted = cases.build(BITS)
    _, _, fitted, given = device(BITS)
    hsq = device(BITS)[0]["hsq"]
    scan = scan_of(BITS)
    T = len(columns)
    for t in (planted["alone"], planted["zero"], T - 1):
        same(scan.effects_lmm(pheno, columns[t], at[t]), fitted, [t], "alone")
        same(scan.effects_lmm(pheno, columns[t], at[t], hsq=hsq), given, [t], "alone, given")
    back = np.arange(T)[::-1]
    same(scan.effects_lmm(pheno, columns[back], at[back]), fitted, back, "reversed")
    twice = np.concatenate([np.arange(T), [planted["alone"], 5, planted["alone"]]])
    same(scan.effects_lmm(pheno, columns[twice], at[twice], hsq=hsq), given, twice, "given twice")
    # with P = 1, and the column at 0, 17 and 64 of 65
    Y = pheno[:, :65]
    m = int(at[planted["alone"]])
    wide = scan.effects_lmm(Y, [0, 17, 64], [m, m, m])
    for k, p in enumerate((0, 17, 64)):
        same(scan.effects_lmm(Y[:, p], [0], [m]), wide, [k], f"column {p} as the only one")
        shifted = np.roll(Y, -p, axis=1)                                            # column p now stands at 0
        same(scan.effects_lmm(shifted, [0], [m]), wide, [k], f"column {p} moved to 0")
    scan.close()


def test_the_target_chunk_boundary():
    """T = 513: the targets on either side of the 512-target chunk alone, and the list with one target put in front."""
    case = cases.CHUNK
    pheno, columns, at, _ = cases.build(case)
    assert len(columns) == cases.CHUNK_T
    _, _, fitted, _ = device(case)
    scan = scan_of(case)
    for t in (510, 511, 512):
        same(scan.effects_lmm(pheno, columns[t], at[t]), fitted, [t], f"target {t} alone")
    order = np.concatenate([[512], np.arange(512)])
    same(scan.effects_lmm(pheno, columns[order], at[order]), fitted, order, "rotated by one")
    scan.close()


def test_the_cohorts_appends_do_not_change_a_bit():
    pheno, columns, at, _ = cases.build(BITS)
    _, _, fitted, _ = device(BITS)
    rows = np.arange(0, len(columns), 7)
    for split in (lambda d: [d[:1], d[1:]], lambda d: [d[k:k + 3] for k in range(0, len(d), 3)]):
        scan = scan_of(BITS, split)
        same(scan.effects_lmm(pheno, columns[rows], at[rows]), fitted, rows, "appended in parts")
        scan.close()


def test_overall_mode_is_loco_mode_handed_the_same_matrix():
    case = lmm.CASES[10]
    pheno, columns, at, _ = cases.build(case)
    _, _, fitted, _ = device(case)
    scan = open_scan(case)
    scan.prepare_lmm(lmm.build(case)[1], [scan.kinship()] * len(case[4]))
    same(scan.effects_lmm(pheno, columns, at), fitted, note="three decompositions of one matrix")
    scan.close()


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_support_intervals_are_the_rule_on_the_devices_own_lods(case):
    pheno = cases.build(case)[0]
    run = device(case)[0]
    scan = scan_of(case)
    for drop in (0.0, 1.5, 1e6):
        got = scan.run_lmm(pheno, lod_drop=drop)
        peak, lo, hi = plain.support_rule(got["lod"], case[4], drop)
        np.testing.assert_array_equal(got["peak_index"], peak)
        np.testing.assert_array_equal(got["support_lo"], lo)
        np.testing.assert_array_equal(got["support_hi"], hi)
        assert sorted(got) == sorted(list(run) + ["support_lo", "support_hi"])
        for key in run:
            np.testing.assert_array_equal(got[key], run[key], err_msg=f"{key} with a drop of {drop}")
    quiet = scan.run_lmm(pheno, want_lod=False, lod_drop=1.5)
    np.testing.assert_array_equal(quiet["support_lo"], plain.support_rule(run["lod"], case[4], 1.5)[1])
    assert "lod" not in quiet
    scan.close()


def test_support_intervals_across_the_phenotype_chunk():
    case = cases.CHUNK
    pheno = cases.build(case)[0]
    wide = np.tile(pheno, (1, 171))[:, :513]
    scan = scan_of(case)
    plain_run = scan.run_lmm(wide)
    got = scan.run_lmm(wide, lod_drop=1.5)
    scan.close()
    peak, lo, hi = plain.support_rule(got["lod"], case[4], 1.5)
    np.testing.assert_array_equal(got["support_lo"], lo)
    np.testing.assert_array_equal(got["support_hi"], hi)
    assert (lo <= peak).all() and (peak <= hi).all() and (lo < hi).any()
    for key in plain_run:
        np.testing.assert_array_equal(got[key], plain_run[key], err_msg=key)


def test_the_other_entry_points_give_the_same_bits_before_and_after():
    case = lmm.CASES[0]
    D, Z, Y, _, _, _ = lmm.build(case)
    pheno, columns, at, _ = cases.build(case)
    grid, pos, masks, _ = snp_cases.snp_set(case)
    scan = scan_of(case)
    scan.prepare(Z)
    scan.set_snps(grid, pos, masks)
    passes = lambda: (scan.run(Y), scan.run_lmm(Y), scan.run_snps_lmm(Y), scan.run_lmm(Y, lod_drop=1.5))
    before = passes()
    info = (scan.info()["device_bytes"], scan.lmm_info()["device_bytes"])
    got = scan.effects_lmm(pheno, columns, at)
    after = passes()
    assert (scan.info()["device_bytes"], scan.lmm_info()["device_bytes"]) == info
    again = scan.effects_lmm(pheno, columns, at)
    scan.close()
    for a, b in zip(before, after):
        assert sorted(a) == sorted(b)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    same(got, device(case)[2], note="beside the other passes")
    same(again, device(case)[2], note="after the other passes")


def test_refusals_leave_the_outputs_and_the_handle():
    from gbrs_amd import _lib
    case = lmm.CASES[8]
    H, n, cz, P, points, _ = case
    D, Z, _, _, _, _ = lmm.build(case)
    pheno, columns, at, _ = cases.build(case)
    M, P1 = sum(points), pheno.shape[1]
    lib = _lib.load()
    scan = open_scan(case)
    with pytest.raises(_lib.GbrsHipError, match="call prepare_lmm first"):
        scan.effects_lmm(pheno, columns, at)
    y = np.ascontiguousarray(lmm.centred(pheno))
    col, pt = np.array([0, 1], dtype=np.int64), np.array([2, 3], dtype=np.int64)
    outs = lambda: (np.full((2, H), 7.0), np.full((2, H), 7.0), np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7, dtype=np.int32), np.full(2, 7.0))

    def call(P_=P1, y_=y, hsq=None, T=2, col_=col, pt_=pt):
        o = outs()
        status = lib.gbrs_scan_lmm_effects(scan._h, P_, _lib.ptr(y_), _lib.ptr(hsq), T, _lib.ptr(col_), _lib.ptr(pt_),
                                           *[_lib.ptr(a) for a in o])
        assert all((a == 7).all() for a in o) or status == _lib.GBRS_OK
        return status, lib.gbrs_last_error().decode()

    status, text = call()
    assert status == _lib.GBRS_ERR_INVALID and "gbrs_scan_lmm_prepare first" in text
    assert lib.gbrs_scan_lmm_run_support(scan._h, P1, _lib.ptr(y), None, 1.5, None, None, None, None, None, None, None) == _lib.GBRS_ERR_INVALID
    assert b"gbrs_scan_lmm_prepare first" in lib.gbrs_last_error()
    scan.prepare_lmm(Z)
    want = scan.effects_lmm(pheno, col, pt)
    run = scan.run_lmm(pheno)
    bad = np.array(y)
    bad[4, 2] = np.inf
    for kwargs, message in ((dict(P_=0), "at least 1 phenotype"), (dict(T=-1), "cannot be negative"),
                            (dict(col_=np.array([0, P1], dtype=np.int64)), f"target 1 is phenotype column {P1}"),
                            (dict(col_=np.array([-1, 0], dtype=np.int64)), "target 0 is phenotype column -1"),
                            (dict(pt_=np.array([2, M], dtype=np.int64)), f"target 1 is at grid point {M}"),
                            (dict(pt_=np.array([-1, 2], dtype=np.int64)), "target 0 is at grid point -1"),
                            (dict(y_=bad), "phenotype 2 holds a value that is not finite (sample 4)"),
                            (dict(hsq=np.full((P1, 3), 1.5)), "outside [0, 1]"),
                            (dict(hsq=np.where(np.arange(3 * P1).reshape(P1, 3) == 4, np.nan, 0.5)), "phenotype 1 and decomposition 1")):
        status, text = call(**kwargs)
        assert status == _lib.GBRS_ERR_INVALID and message in text, (message, text)
    assert call(T=0)[0] == _lib.GBRS_OK                                             # nothing to do, nothing written
    empty = scan.effects_lmm(pheno, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert empty["effect"].shape == (0, H) and empty["rank"].shape == (0,)
    for drop in (-1.0, np.nan, np.inf):
        with pytest.raises(_lib.GbrsHipError, match="LOD drop of a support interval must be a finite number that is not negative"):
            scan.run_lmm(pheno, lod_drop=drop)
    with pytest.raises(ValueError, match="phenotype columns and"):
        scan.effects_lmm(pheno, [0, 1], [2])
    same(scan.effects_lmm(pheno, col, pt), want, note="after the refusals")
    after = scan.run_lmm(pheno)
    for key in RUN:
        np.testing.assert_array_equal(after[key], run[key], err_msg=key)
    info = scan.lmm_info()
    scan.append(D[:2])                                                              # an append drops the preparation, as before
    assert scan.lmm_info()["cz"] == 0 and scan.lmm_info()["device_bytes"] < info["device_bytes"]
    with pytest.raises(_lib.GbrsHipError, match="prepare_lmm first"):
        scan.effects_lmm(np.ones((n + 2, 1)), [0], [0])
    with pytest.raises(_lib.GbrsHipError, match="prepare_lmm first"):
        scan.run_lmm(np.ones((n + 2, 1)), lod_drop=1.5)
    scan.close()


# ---- the commands ----------------------------------------------------------------------------------------------------------

def effects_lines(names, chrom_names, pos, targets, points, got):
    return ["\t".join([names[p], chrom_names[c], repr(float(pos[points[t]])), repr(float(got["lod"][t])), str(int(got["rank"][t])),
                       repr(float(got["hsq"][t]))] + [repr(float(v)) for pair in zip(got["effect"][t], got["se"][t]) for v in pair])
            for t, (p, c) in enumerate(targets)]


def test_gbrs_scan_with_kinship_effects_and_intervals(tmp_path, caplog):
    """`gbrs scan --scan-kinship loco --scan-kinship-effects --scan-kinship-lod-drop 1.5`: the two effects files hold
    effects_lmm at the scan's peaks and heritabilities, the scan's files the intervals of run_lmm(lod_drop=1.5); without the
    new options every file is byte for byte write_scan's of run_lmm; the old refusal stands."""
    from gbrs_amd import cli
    from gbrs_amd.scan import mediation_targets, write_scan
    case = lmm.CASES[8]
    H, n, cz, P, points, _ = case
    D, Z, Y, _, _, _ = lmm.build(case)
    command, ids, names, chrom_names, pos = write_cohort(tmp_path, case)
    founders = [chr(ord("A") + h) for h in range(H)]
    scan = scan_of(case)
    run = scan.run_lmm(Y)
    with_drop = scan.run_lmm(Y, lod_drop=1.5)
    min_lod = float(np.sort(run["peak_lod"].ravel())[3])                             # all but three peaks reach it
    targets = mediation_targets(run["peak_lod"], run["peak_index"], min_lod)
    at = run["peak_index"][targets[:, 0], targets[:, 1]]
    want = scan.effects_lmm(Y, targets[:, 0], at, hsq=run["hsq"])
    scan.close()
    assert len(targets) == 3 * P - 3
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(command + ["--scan-out", str(tmp_path / "mixed"), "--scan-kinship", "loco", "--scan-kinship-effects",
                                   "--scan-kinship-effects-min-lod", repr(min_lod), "--scan-kinship-lod-drop", "1.5"]) == 0
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("mixed.")) == ["mixed.scan.effects.npz", "mixed.scan.effects.tsv",
                                                                                 "mixed.scan.npz", "mixed.scan.peaks.tsv"]
    z = np.load(tmp_path / "mixed.scan.effects.npz")
    assert sorted(z.files) == sorted(["phenotypes", "founders", "samples", "covariates", "targets", "target_phenotype", "target_chromosome",
                                      "points", "position", "min_lod", "effect", "se", "lod", "sigma2", "rank", "hsq", "kinship_mode"])
    assert str(z["kinship_mode"]) == "loco" and z["founders"].tolist() == founders and float(z["min_lod"]) == min_lod
    np.testing.assert_array_equal(z["points"], at)
    np.testing.assert_array_equal(z["target_phenotype"], targets[:, 0])
    for key in OUT:
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    np.testing.assert_array_equal(z["hsq"], run["hsq"][targets[:, 0], targets[:, 1]])
    np.testing.assert_array_equal(z["lod"], run["peak_lod"][targets[:, 0], targets[:, 1]])
    lines = open(tmp_path / "mixed.scan.effects.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\trank\thsq" + "".join(f"\teffect_{f}\tse_{f}" for f in founders)
    assert lines[1:] == effects_lines(names, chrom_names, pos, targets, at, want)
    s = np.load(tmp_path / "mixed.scan.npz")
    assert sorted(s.files) == sorted(["phenotypes", "samples", "covariates", "chrom", "pos", "peak_lod", "peak_index", "hsq", "sigma2",
                                      "rank_min", "rank_max", "kinship_mode", "lod", "support_lo", "support_hi", "lod_drop"])
    assert float(s["lod_drop"]) == 1.5
    for key in with_drop:
        np.testing.assert_array_equal(s[key], with_drop[key], err_msg=key)
    peaks = open(tmp_path / "mixed.scan.peaks.tsv").read().splitlines()
    assert peaks[0] == "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\thsq\tsupport_lo\tsupport_hi"
    expected = []
    for p, name in enumerate(names):
        top = max(range(3), key=lambda c: (run["peak_lod"][p, c], -c))
        for c in range(3):
            expected.append("\t".join([name, chrom_names[c], repr(float(pos[run["peak_index"][p, c]])), repr(float(run["peak_lod"][p, c])),
                                       str(int(c == top)), repr(float(run["hsq"][p, c])), repr(float(pos[with_drop["support_lo"][p, c]])),
                                       repr(float(pos[with_drop["support_hi"][p, c]]))]))
    assert peaks[1:] == expected
    # a minimum above every peak: both files, headers only
    assert cli.main(command + ["--scan-out", str(tmp_path / "none"), "--scan-kinship", "loco", "--scan-kinship-effects",
                               "--scan-kinship-effects-min-lod", "1e9"]) == 0
    assert open(tmp_path / "none.scan.effects.tsv").read().splitlines() == lines[:1]
    e = np.load(tmp_path / "none.scan.effects.npz")
    assert e["effect"].shape == (0, H) and e["hsq"].shape == (0,) and "support_lo" not in np.load(tmp_path / "none.scan.npz").files
    # without the new options: the mixed model's files as they were
    assert cli.main(command + ["--scan-out", str(tmp_path / "old"), "--scan-kinship", "loco"]) == 0
    chrom = np.repeat(chrom_names, points)
    write_scan(str(tmp_path / "hand"), names, ids, ["intercept", "sex"], chrom, pos, chrom_names, run, None, kinship_mode="loco")
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("old.")) == ["old.scan.npz", "old.scan.peaks.tsv"]
    assert open(tmp_path / "old.scan.peaks.tsv", "rb").read() == open(tmp_path / "hand.scan.peaks.tsv", "rb").read()
    a, b = np.load(tmp_path / "old.scan.npz"), np.load(tmp_path / "hand.scan.npz")
    assert a.files == b.files == ["phenotypes", "samples", "covariates", "chrom", "pos", "peak_lod", "peak_index", "hsq", "sigma2",
                                  "rank_min", "rank_max", "kinship_mode", "lod"]
    for key in b.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    # the passes of the unweighted W are still refused next to the kinship, before the device runs
    caplog.clear()
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(command + ["--scan-out", str(tmp_path / "refused"), "--scan-kinship", "overall", "--scan-effects"])
        cli.main(command + ["--scan-out", str(tmp_path / "refused"), "--scan-kinship-effects"])
    assert any("--scan-effects cannot be combined with --scan-kinship" in r.getMessage() for r in caplog.records)
    assert any("--scan-kinship-effects needs --scan-kinship" in r.getMessage() for r in caplog.records)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused.")]


def test_gbrs_reconstruct_with_kinship_effects_and_intervals(tmp_path, tables, caplog, monkeypatch):
    """`gbrs reconstruct --scan-pheno --scan-kinship overall --scan-kinship-effects --scan-kinship-lod-drop 1.5` on six
    samples: the effects files and the interval columns are effects_lmm and run_lmm(lod_drop=1.5) driven by hand on the
    dosages that went through the handle; without the options every file of the run is what it was."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import DiplotypeHMM
    from gbrs_amd.scan import GenomeScan, mediation_targets
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self.grid_points, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    rng = np.random.default_rng(34)
    names = [f"gene{p}" for p in range(4)]
    values = rng.normal(size=(N_FILES, 4))
    ids = lambda stem: [str(tmp_path / f"{stem}{s}") for s in range(N_FILES)]
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]

    def reconstruct(stem, extra):
        sample_file = cohort_files(tmp_path, stem)
        pheno = write_table(tmp_path / f"{stem}.pheno.tsv", ids(stem), names, values)
        return cli.main(["reconstruct", "--sample-file", sample_file] + common +
                        ["--scan-pheno", pheno, "--scan-out", str(tmp_path / stem), "--scan-kinship", "overall", "--scan-lod-matrix"] + extra)

    with caplog.at_level("ERROR", logger="gbrs"):
        assert reconstruct("with", ["--scan-kinship-effects", "--scan-kinship-effects-min-lod", "0", "--scan-kinship-lod-drop", "1.5"]) == 0
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    first = len(seen)
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])
    assert reconstruct("plain", []) == 0
    assert len(seen) == 2 * first
    assert not [f for f in os.listdir(tmp_path) if f.startswith("plain.scan.effects")]
    made = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain") and not f.startswith("plain.pheno") and f != "plain.txt")
    assert made == sorted(f[len("with"):] for f in os.listdir(tmp_path)
                          if f.startswith("with") and not f.startswith(("with.pheno", "with.scan.effects")) and f != "with.txt")
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare_lmm(None, "overall")
    run = scan.run_lmm(values)
    with_drop = scan.run_lmm(values, lod_drop=1.5)
    targets = mediation_targets(run["peak_lod"], run["peak_index"], 0.0)
    at = run["peak_index"][targets[:, 0], targets[:, 1]]
    want = scan.effects_lmm(values, targets[:, 0], at, hsq=run["hsq"])
    scan.close()
    a, b = np.load(tmp_path / "with.scan.npz"), np.load(tmp_path / "plain.scan.npz")
    assert [k for k in a.files if k not in ("support_lo", "support_hi", "lod_drop")] == b.files
    for key in b.files:
        if key != "samples":                                                        # the outbases carry the stem
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    for key in with_drop:
        np.testing.assert_array_equal(a[key], with_drop[key], err_msg=key)
    pos = a["pos"]
    old, new = (open(tmp_path / f"{stem}.scan.peaks.tsv").read().splitlines() for stem in ("plain", "with"))
    assert new[0] == old[0] + "\tsupport_lo\tsupport_hi" and len(new) == len(old)
    rows = [(p, c) for p in range(4) for c in range(len(points)) if run["peak_index"][p, c] >= 0]
    assert new[1:] == [line + f"\t{repr(float(pos[with_drop['support_lo'][p, c]]))}\t{repr(float(pos[with_drop['support_hi'][p, c]]))}"
                       for line, (p, c) in zip(old[1:], rows)]
    z = np.load(tmp_path / "with.scan.effects.npz")
    assert len(targets) == len(rows) > 0 and str(z["kinship_mode"]) == "overall" and z["samples"].tolist() == ids("with")
    for key in OUT:
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    np.testing.assert_array_equal(z["points"], at)
    lines = open(tmp_path / "with.scan.effects.tsv").read().splitlines()
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    assert lines[1:] == effects_lines(names, [str(c) for c in p0.chroms], pos, targets, at, want)
    assert lines[0].startswith("#phenotype\tchromosome\tposition\tlod\trank\thsq\teffect_")
    caplog.clear()
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(["reconstruct", "--sample-file", cohort_files(tmp_path, "refused")] + common +
                 ["--scan-pheno", str(tmp_path / "with.pheno.tsv"), "--scan-kinship-lod-drop", "1.5"])
    assert any("--scan-kinship-lod-drop needs --scan-kinship" in r.getMessage() for r in caplog.records)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused0.")]
