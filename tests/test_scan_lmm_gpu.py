"""The mixed-model genome scan on the device (gbrs_scan_kinship, gbrs_scan_lmm_*, GenomeScan.kinship / prepare_lmm /
run_lmm; needs an MI355X) against the two host routes of tests/scan_lmm_cases.py, each fed the device's own
heritabilities, at ten times each case's recorded floor; the fitted heritabilities within MEASURED_HSQ of the
restatement's; the kinships against numpy at ten times numpy's own distance from the long double sums; and the bit
equalities, refusals and files."""
import functools
import os

import numpy as np
import pytest

import scan_cases as base
import scan_lmm_cases as cases

pytestmark = pytest.mark.gpu

ALL = cases.CASES + cases.LARGE_CASES
BITS = cases.CASES[1]                      # H8-n70-c2-P65: the case of the bit equalities
KEYS = ("lod", "peak_lod", "peak_index", "hsq", "sigma2", "rank_min", "rank_max")


def open_scan(case, split=None):
    from gbrs_amd.scan import GenomeScan
    H, n, cz, P, points, mode = case
    D = cases.build(case)[0]
    scan = GenomeScan(H, points)
    for part in ([D] if split is None else split(D)):
        scan.append(part)
    return scan


def kinship_argument(case):
    mode = case[5]
    if mode == "scaled":
        return list(cases.build(case)[3])                 # the caller's own matrix per chromosome
    return cases.build(case)[3][0] if mode == "given" else mode


@functools.lru_cache(maxsize=None)
def device(case):
    """(run_lmm's dict, the matrices prepare_lmm used) of a case, computed once."""
    D, Z, Y, _, _, _ = cases.build(case)
    scan = open_scan(case)
    used = scan.prepare_lmm(Z, kinship_argument(case))
    got = scan.run_lmm(Y)
    info = scan.lmm_info()
    scan.close()
    assert info["cz"] == case[2] and info["n_eig"] == len(used) and info["P"] == case[3]
    assert info["rotate_ms"] > 0 and info["null_ms"] > 0 and info["point_ms"] > 0 and info["peak_device_bytes"] > info["device_bytes"] > 0
    for a in list(got.values()) + used:
        a.setflags(write=False)
    return got, used


def per_decomposition(case, by_chrom):
    kin_of_chrom = cases.build(case)[4]
    return by_chrom[:, [list(kin_of_chrom).index(e) for e in range(max(kin_of_chrom) + 1)]]


@pytest.mark.parametrize("case", ALL, ids=cases.case_id)
def test_lods_against_both_host_routes_at_the_devices_heritabilities(case):
    D, Z, Y, kinships, kin_of_chrom, _ = cases.build(case)
    got, _ = device(case)
    hsq = per_decomposition(case, got["hsq"])
    np.testing.assert_array_equal(got["hsq"], hsq[:, list(kin_of_chrom)])           # chromosomes of one decomposition share it
    rule = cases.lmm_rule(D, Z, Y, case[4], cases.decompositions(case), kin_of_chrom, hsq=hsq)
    gls = cases.lmm_gls(D, Z, Y, case[4], kinships, kin_of_chrom, hsq)
    for name, want in (("rule", rule["lod"]), ("gls", gls)):
        measured = cases.deviation(got["lod"], want)
        print(f"{cases.case_id(case)} vs {name}: {measured:.3g}, tolerance {cases.device_tol(case):.3g}")
        assert measured <= cases.device_tol(case), name
    np.testing.assert_array_equal(got["rank_min"], rule["rank_min"])
    np.testing.assert_array_equal(got["rank_max"], rule["rank_max"])
    sigma2 = per_decomposition(case, got["sigma2"])
    # rss is the difference of two sums of n terms of centred numbers: n rounding steps on either side of a cancellation
    # that loses less than a factor of 4
    np.testing.assert_allclose(sigma2, rule["sigma2"], rtol=8 * case[1] * np.finfo(float).eps, atol=0)
    peak, index = base.peaks(got["lod"], case[4])
    np.testing.assert_array_equal(got["peak_index"], index)
    np.testing.assert_array_equal(got["peak_lod"], peak)


@pytest.mark.parametrize("case", ALL, ids=cases.case_id)
def test_fitted_heritabilities(case):
    """Every pair within MEASURED_HSQ of the restatement's; a boundary optimum whose margin exceeds ENDPOINT_MARGIN equal
    with == (at the usual scale of the kinship no margin does, in the `scaled` case 10 of 14 do: test_scan_lmm_cpu.py
    prints them)."""
    got, _ = device(case)
    rule, _ = cases.expected(case)
    hsq = per_decomposition(case, got["hsq"])
    assert ((hsq >= 0.0) & (hsq <= 1.0)).all()
    print(f"{cases.case_id(case)}: worst {np.abs(hsq - rule['hsq']).max():.3g}, bound {cases.MEASURED_HSQ:.3g}")
    assert np.abs(hsq - rule["hsq"]).max() <= cases.MEASURED_HSQ
    boundary = (rule["hsq"] == 0.0) | (rule["hsq"] == 1.0)
    with np.errstate(invalid="ignore"):
        sure = boundary & (rule["margin"] > cases.ENDPOINT_MARGIN)
    np.testing.assert_array_equal(hsq[sure], rule["hsq"][sure])
    assert case[5] != "scaled" or sure.sum() >= 5
    print(f"{int(sure.sum())} of {int(boundary.sum())} boundary pairs compared with ==, "
          f"{int((hsq[boundary] == rule['hsq'][boundary]).sum())} equal")


@pytest.mark.parametrize("case", [cases.CASES[0], cases.CASES[3], cases.CASES[5], cases.CASES[6], cases.CASES[8], cases.LARGE_CASES[0]], ids=cases.case_id)
def test_kinship(case):
    """Per left-out chromosome and overall, against numpy's A A' at ten times numpy's distance from the long double sums
    (at least one unit in the last place of the largest entry); symmetric bit for bit; the scale is the caller's."""
    D, points = cases.build(case)[0], case[4]
    scan = open_scan(case)
    for leave_out in [None] + list(range(len(points))):
        K = scan.kinship(leave_out)
        assert (K == K.T).all()
        want, exact = cases.kinship(D, points, leave_out), cases.kinship_longdouble(D, points, leave_out)
        floor = max(np.abs(want - exact).max(), np.spacing(np.abs(exact).max()))
        assert np.abs(K - want).max() <= base.DEVICE_FACTOR * floor, leave_out
    np.testing.assert_array_equal(scan.kinship(1, scale=8.0), 4.0 * scan.kinship(1))      # the default is 2 / t^2 = 2 for rows that add up to 1
    assert scan.lmm_info()["kinship_ms"] > 0
    scan.close()


def test_heritabilities_given_are_honoured_and_zero_is_the_plain_scan():
    case = cases.CASES[4]
    D, Z, Y, kinships, kin_of_chrom, _ = cases.build(case)
    P, nc = Y.shape[1], len(case[4])
    scan = open_scan(case)
    scan.prepare_lmm(Z)
    given = np.random.default_rng(5).uniform(0.0, 1.0, size=(P, nc))
    got = scan.run_lmm(Y, hsq=given)
    np.testing.assert_array_equal(got["hsq"], given)
    for route in (cases.lmm_rule(D, Z, Y, case[4], cases.decompositions(case), kin_of_chrom, hsq=given)["lod"],
                  cases.lmm_gls(D, Z, Y, case[4], kinships, kin_of_chrom, given)):
        assert cases.deviation(got["lod"], route) <= cases.device_tol(case)
    zero = scan.run_lmm(Y, hsq=np.zeros((P, nc)))
    scan.prepare(Z)
    plain = scan.run(Y)
    scan.close()
    # two device passes, each within ten times its restatement's floor of the same least squares
    assert cases.deviation(zero["lod"], plain["lod"]) <= base.DEVICE_FACTOR * (cases.measured_floor(case) + base.MEASURED_FLOOR)
    np.testing.assert_array_equal(zero["peak_index"], plain["peak_index"])
    assert (zero["hsq"] == 0.0).all()


def test_a_phenotype_has_the_same_bits_alone_at_any_column_and_in_any_chunk():
    D, Z, Y, _, _, _ = cases.build(BITS)
    got, _ = device(BITS)
    scan = open_scan(BITS)
    scan.prepare_lmm(Z)
    for p in (0, 64, 17):
        alone = scan.run_lmm(Y[:, p])
        for key in KEYS:
            np.testing.assert_array_equal(alone[key][0], got[key][p], err_msg=f"{key} of column {p}")
    wide = np.tile(Y, (1, 8))[:, :515]                                              # column 512 + k is column (512 + k) % 65
    far = scan.run_lmm(wide)
    scan.close()
    for key in KEYS:
        np.testing.assert_array_equal(far[key][:65], got[key], err_msg=key)
        np.testing.assert_array_equal(far[key][511:515], got[key][[511 % 65, 512 % 65, 513 % 65, 514 % 65]], err_msg=key)


def test_the_cohorts_appends_do_not_change_a_bit():
    D, Z, Y, _, _, _ = cases.build(BITS)
    got, used = device(BITS)
    for split in (lambda d: [d[:1], d[1:]], lambda d: [d[k:k + 3] for k in range(0, len(d), 3)]):
        scan = open_scan(BITS, split)
        again = scan.prepare_lmm(Z)
        for a, b in zip(again, used):
            np.testing.assert_array_equal(a, b)
        out = scan.run_lmm(Y[:, :9])
        scan.close()
        for key in KEYS:
            np.testing.assert_array_equal(out[key], got[key][:9], err_msg=key)


def test_overall_mode_is_loco_mode_handed_the_same_matrix():
    case = cases.CASES[10]
    D, Z, Y, _, _, _ = cases.build(case)
    got, used = device(case)
    scan = open_scan(case)
    K = scan.kinship()
    np.testing.assert_array_equal(K, used[0])
    scan.prepare_lmm(Z, [K] * len(case[4]))
    assert scan.lmm_info()["n_eig"] == len(case[4])
    out = scan.run_lmm(Y)
    scan.close()
    for key in KEYS:
        np.testing.assert_array_equal(out[key], got[key], err_msg=key)


def test_refusals_leave_the_preparation_and_its_bits():
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    case = cases.CASES[8]
    H, n, cz, P, points, _ = case
    D, Z, Y, kinships, _, _ = cases.build(case)
    got, _ = device(case)
    lib = _lib.load()
    scan = open_scan(case)
    with pytest.raises(_lib.GbrsHipError, match="call prepare_lmm first"):
        scan.run_lmm(Y)
    y = np.ascontiguousarray(cases.centred(Y))
    assert lib.gbrs_scan_lmm_run(scan._h, P, _lib.ptr(y), None, None, None, None, None, None) == _lib.GBRS_ERR_INVALID
    assert b"gbrs_scan_lmm_prepare first" in lib.gbrs_last_error()
    scan.prepare_lmm(Z)
    eigs = cases.decompositions(case)
    U, lam = [u for u, _ in eigs], [np.ascontiguousarray(v) for _, v in eigs]
    mapping = np.arange(3, dtype=np.int32)

    def prepare(cz_, z, n_eig=3, vectors=U, values=lam, chrom=mapping):
        status = lib.gbrs_scan_lmm_prepare(scan._h, cz_, _lib.ptr(z), n_eig, _lib.ptr_table(vectors), _lib.ptr_table(values), _lib.ptr(chrom))
        return status, lib.gbrs_last_error().decode()

    z17 = np.ones((n, 17))
    bad_z = np.array(Z)
    bad_z[5, 1] = np.nan
    bad_u = [U[0], np.where(np.arange(n * n).reshape(n, n) == 7, np.inf, U[1]), U[2]]
    small = [lam[0], lam[1] * np.where(np.arange(n) == 0, 1e-12, 1.0), lam[2]]
    inf_lam = [np.where(np.arange(n) == 3, np.inf, lam[0]), lam[1], lam[2]]
    for args, message in (((0, Z), "must be 1..16"), ((17, z17), "must be 1..16"), ((cz, bad_z), "sample 5, column 1"),
                          ((cz, Z, 3, bad_u), "decomposition 1: the eigenvectors hold a value that is not finite (row 0, column 7)"),
                          ((cz, Z, 3, U, small), "decomposition 1: eigenvalue 0"),
                          ((cz, Z, 3, U, inf_lam), "decomposition 0: eigenvalue 3 is not finite"),
                          ((cz, Z, 0), "decompositions must number"), ((cz, Z, 3, U, lam, np.array([0, 1, 3], dtype=np.int32)), "mapped to decomposition 3")):
        status, text = prepare(*args)
        assert status == _lib.GBRS_ERR_INVALID and message in text, (message, text)
    assert "fewer independent dosage columns than samples" in prepare(cz, Z, 3, U, small)[1]
    singular = kinships[0] - np.outer(eigs[0][0][:, 0], eigs[0][0][:, 0]) * eigs[0][1][0]        # its smallest eigenvalue taken out
    with pytest.raises(_lib.GbrsHipError, match="fewer independent dosage columns than samples"):
        scan.prepare_lmm(Z, [singular] + kinships[1:])
    with pytest.raises(ValueError, match="at most 16 covariate columns"):
        scan.prepare_lmm(z17)
    with pytest.raises(_lib.GbrsHipError, match="outside \\[0, 1\\]"):
        scan.run_lmm(Y, hsq=np.full((P, 3), 1.5))
    with pytest.raises(_lib.GbrsHipError, match="phenotype 2 holds a value that is not finite \\(sample 4\\)"):
        scan.run_lmm(np.where((np.arange(n)[:, None] == 4) & (np.arange(P) == 2), np.nan, Y))
    with pytest.raises(_lib.GbrsHipError, match="to leave out"):
        scan.kinship(3)
    after = scan.run_lmm(Y)
    for key in KEYS:
        np.testing.assert_array_equal(after[key], got[key], err_msg=key)
    scan.append(D[:2])                                                              # an append drops the preparation
    assert scan.lmm_info()["cz"] == 0
    with pytest.raises(_lib.GbrsHipError, match="prepare_lmm first"):
        scan.run_lmm(np.ones((n + 2, 1)))
    scan.close()
    few = GenomeScan(H, points)                                                     # n = cz + H - 1: one sample short
    few.append(D[:cz + H - 1])
    with pytest.raises(_lib.GbrsHipError, match="too few"):
        few.prepare_lmm(Z[:cz + H - 1], np.eye(cz + H - 1))
    few.close()
    one = GenomeScan(2, [5, 0])                                                     # chromosome 0 holds every grid point
    one.append(np.full((4, 5, 2), 0.5))
    with pytest.raises(_lib.GbrsHipError, match="holds every grid point"):
        one.kinship(0)
    assert one.kinship(1).shape == (4, 4)
    one.close()
    many = GenomeScan(2, [1])                                                       # past the cap of 4096 samples
    many.append(np.full((4097, 1, 2), 0.5))
    dummy = np.ones((4097, 1))
    status = lib.gbrs_scan_lmm_prepare(many._h, 1, _lib.ptr(dummy), 1, _lib.ptr_table([dummy]), _lib.ptr_table([dummy]),
                                       _lib.ptr(np.zeros(1, dtype=np.int32)))
    assert status == _lib.GBRS_ERR_INVALID and b"at most 4096 samples" in lib.gbrs_last_error()
    with pytest.raises(_lib.GbrsHipError, match="at most 4096 samples"):
        many.kinship()
    many.close()


def test_the_plain_scan_and_the_mixed_model_do_not_touch_each_other():
    case = cases.CASES[0]
    D, Z, Y, _, _, _ = cases.build(case)
    got, _ = device(case)
    scan = open_scan(case)
    scan.prepare(Z)
    before, rank = scan.run(Y), scan.info()["rank"]
    scan.prepare_lmm(Z)
    mixed = scan.run_lmm(Y)
    after = scan.run(Y)
    scan.prepare(Z)
    again = scan.run(Y)
    np.testing.assert_array_equal(scan.info()["rank"], rank)
    mixed_again = scan.run_lmm(Y)
    scan.close()
    for key in ("lod", "peak_lod", "peak_index"):
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
        np.testing.assert_array_equal(again[key], before[key], err_msg=key)
    for key in KEYS:
        np.testing.assert_array_equal(mixed[key], got[key], err_msg=key)
        np.testing.assert_array_equal(mixed_again[key], got[key], err_msg=key)


def write_cohort(folder, case):
    """The files `gbrs scan` reads for a case: dosage tables in `gbrs export` format, their list, the grid file, the
    phenotypes and one covariate.  Returns (command arguments, ids, names, chromosome names, positions)."""
    H, n, cz, P, points, _ = case
    D, Z, Y, _, _, _ = cases.build(case)
    founders = [chr(ord("A") + h) for h in range(H)]
    ids = [f"s{k}" for k in range(n)]
    chrom_names = [str(c + 1) for c in range(len(points))]
    pos = np.concatenate([np.linspace(1.0, 90.0, m) for m in points])
    with open(folder / "grid.tsv", "w") as fh:
        fh.write("marker\tchr\tbp\tcM\n")
        k = 0
        for c, m in zip(chrom_names, points):
            for _ in range(m):
                fh.write(f"m{k}\t{c}\t{k}\t{repr(float(pos[k]))}\n")
                k += 1
    with open(folder / "list.tsv", "w") as fh:
        for k, i in enumerate(ids):
            with open(folder / f"{i}.tsv", "w") as out:
                out.write("# " + "\t".join(founders) + "\n")
                for row in D[k]:
                    out.write("\t".join(repr(float(v)) for v in row) + "\n")
            fh.write(f"{i}\t{folder / (i + '.tsv')}\n")
    names = [f"trait{p}" for p in range(P)]
    with open(folder / "pheno.tsv", "w") as fh:
        fh.write("id\t" + "\t".join(names) + "\n")
        for i, row in zip(ids, Y):
            fh.write(i + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    with open(folder / "covar.tsv", "w") as fh:
        fh.write("id\tsex\n")
        for i, row in zip(ids, Z):
            fh.write(f"{i}\t{repr(float(row[1]))}\n")
    command = ["scan", "--dosage-list", str(folder / "list.tsv"), "--grid-file", str(folder / "grid.tsv"), "--pheno",
               str(folder / "pheno.tsv"), "--covar", str(folder / "covar.tsv")]
    return command, ids, names, chrom_names, pos


def test_gbrs_scan_with_a_kinship(tmp_path, caplog):
    """`gbrs scan --scan-kinship loco --scan-kinship-out` writes what run_lmm returns, the new arrays and the new column;
    without the option the two files are, byte for byte, what write_scan makes of GenomeScan.run - the scan as it was."""
    from gbrs_amd import cli
    from gbrs_amd.scan import write_scan
    case = cases.CASES[8]
    D, Z, Y, _, _, _ = cases.build(case)
    got, used = device(case)
    command, ids, names, chrom_names, pos = write_cohort(tmp_path, case)
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(command + ["--scan-out", str(tmp_path / "mixed"), "--scan-kinship", "loco", "--scan-kinship-out"]) == 0
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("mixed.")) == ["mixed.scan.kinship.npz", "mixed.scan.npz", "mixed.scan.peaks.tsv"]
    z = np.load(tmp_path / "mixed.scan.npz")
    assert sorted(z.files) == sorted(["phenotypes", "samples", "covariates", "chrom", "pos", "peak_lod", "peak_index", "hsq", "sigma2",
                                      "rank_min", "rank_max", "kinship_mode", "lod"])
    assert str(z["kinship_mode"]) == "loco" and z["samples"].tolist() == ids and z["covariates"].tolist() == ["intercept", "sex"]
    for key in KEYS:
        np.testing.assert_array_equal(z[key], got[key], err_msg=key)
    lines = open(tmp_path / "mixed.scan.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\thsq"
    expected = []
    for p, name in enumerate(names):
        top = max(range(3), key=lambda c: (got["peak_lod"][p, c], -c))
        for c in range(3):
            expected.append("\t".join([name, chrom_names[c], repr(float(pos[got["peak_index"][p, c]])), repr(float(got["peak_lod"][p, c])),
                                       str(int(c == top)), repr(float(got["hsq"][p, c]))]))
    assert lines[1:] == expected
    k = np.load(tmp_path / "mixed.scan.kinship.npz")
    assert k["samples"].tolist() == ids and k["chromosomes"].tolist() == chrom_names and str(k["kinship_mode"]) == "loco"
    np.testing.assert_array_equal(k["kinship"], np.stack(used))
    np.testing.assert_array_equal(k["kinship_of_chromosome"], [0, 1, 2])
    # without the option: no new code runs, the files are the plain scan's
    assert cli.main(command + ["--scan-out", str(tmp_path / "plain")]) == 0
    scan = open_scan(case)
    scan.prepare(Z)
    result, rank = scan.run(Y), scan.info()["rank"]
    scan.close()
    chrom = np.repeat(chrom_names, case[4])
    write_scan(str(tmp_path / "hand"), names, ids, ["intercept", "sex"], chrom, pos, chrom_names, result, rank)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("plain.")) == ["plain.scan.npz", "plain.scan.peaks.tsv"]
    assert open(tmp_path / "plain.scan.peaks.tsv", "rb").read() == open(tmp_path / "hand.scan.peaks.tsv", "rb").read()
    a, b = np.load(tmp_path / "plain.scan.npz"), np.load(tmp_path / "hand.scan.npz")
    assert a.files == b.files == ["phenotypes", "samples", "covariates", "chrom", "pos", "rank", "peak_lod", "peak_index", "lod"]
    for key in b.files:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    # and the passes of the unweighted W are refused next to the kinship, before the device runs
    caplog.clear()
    with caplog.at_level("ERROR", logger="gbrs"):
        cli.main(command + ["--scan-out", str(tmp_path / "refused"), "--scan-kinship", "overall", "--scan-effects"])
    assert any("--scan-effects cannot be combined with --scan-kinship" in r.getMessage() for r in caplog.records)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("refused.")]
