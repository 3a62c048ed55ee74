"""The genome scan on the device (gbrs_scan_*, gbrs_amd.scan.GenomeScan), `gbrs reconstruct --scan-pheno` and `gbrs scan`
over it (needs an MI355X).  Cohorts, phenotypes and the two host computations: tests/scan_cases.py.

The device is held against both host routes - the numpy restatement of the rule and np.linalg.lstsq - to ten times the
difference the two have between themselves on the CPU (scan_cases.device_tol), and nothing is excluded: the fixtures
hold no grid point whose rank rounding could flip (tests/test_scan_cpu.py)."""
import os

import numpy as np
import pytest

import grid_cases
import scan_cases as cases

pytestmark = pytest.mark.gpu


def scan_of(case, pieces=None):
    """A prepared GenomeScan of a case, the cohort appended in pieces of the given sizes (default: all at once)."""
    from gbrs_amd.scan import GenomeScan
    D, Z, _, _ = cases.build(case)
    scan = GenomeScan(case[0], case[4])
    lo = 0
    for size in pieces or [len(D)]:
        scan.append(D[lo:lo + size])
        lo += size
    assert lo == len(D) == scan.n
    scan.prepare(Z)
    return scan


@pytest.mark.parametrize("case", cases.CASES + cases.LARGE_CASES, ids=cases.case_id)
def test_the_device_against_both_host_routes(case):
    """LODs against the restatement and against lstsq within the case's tolerance; rank and peak_index equal the
    restatement's, peak_lod within the tolerance; the twin grid points carry the same bits and the tie goes to the first.
    Past 256 samples the first 256 alone give other LODs: the samples behind the solve's stride are in what is compared."""
    H, n, c, P, points = case
    _, _, Y, special = cases.build(case)
    lod, rank, _, lod_ls, _ = cases.expected(case)
    scan = scan_of(case)
    got = scan.run(Y)
    info = scan.info()
    scan.close()
    assert got["lod"].shape == (P, sum(points)) and got["peak_lod"].shape == got["peak_index"].shape == (P, len(points))
    assert (info["n"], info["M"], info["H"], info["c"]) == (n, sum(points), H, c)
    assert info["prepare_ms"] > 0 and info["run_ms"] >= info["product_ms"] > 0 and info["device_bytes"] > 8 * n * sum(points) * H
    worst, worst_ls = cases.deviation(got["lod"], lod), cases.deviation(got["lod"], lod_ls)
    print(f"DEVIATION device against scan_rule {worst:.3g}, against scan_lstsq {worst_ls:.3g}, tolerance "
          f"{cases.device_tol(case):.3g}, {cases.case_id(case)}")
    np.testing.assert_array_equal(info["rank"], rank)
    assert worst <= cases.device_tol(case) and worst_ls <= cases.device_tol(case)
    assert (got["lod"] >= 0.0).all()
    twin = special["twin"]
    np.testing.assert_array_equal(got["lod"][:, twin], got["lod"][:, twin - 1])
    peak, index = cases.peaks(lod, points)
    np.testing.assert_array_equal(got["peak_index"], index)
    assert cases.deviation(got["peak_lod"], peak) <= cases.device_tol(case)
    own_peak, own_index = cases.peaks(got["lod"], points)                        # and of the device's own LODs, exactly
    np.testing.assert_array_equal(got["peak_lod"], own_peak)
    np.testing.assert_array_equal(got["peak_index"], own_index)
    if n > c + H:
        assert got["peak_index"][0, -1] == twin - 1
    if n > 256:
        from gbrs_amd.scan import GenomeScan
        D, Z, _, _ = cases.build(case)
        head = GenomeScan(H, points)
        head.append(D[:256])
        head.prepare(Z[:256])
        first = head.run(Y[:256])["lod"]
        head.close()
        assert first.shape == got["lod"].shape and (first != got["lod"]).any()


BITS = (8, 70, 4, 130, (1, 65, 9))
BITS16 = (16, 18, 2, 130, cases.POINTS)


@pytest.mark.parametrize("case", [BITS, BITS16], ids=cases.case_id)
def test_a_phenotype_has_the_same_bits_wherever_it_stands(case):
    """Alone, at column 0, at column 64 and among 130; a second run; without the LOD matrix."""
    _, _, Y, _ = cases.build(case)
    scan = scan_of(case)
    full = scan.run(Y)
    again = scan.run(Y)
    for key in full:
        np.testing.assert_array_equal(again[key], full[key], err_msg=key)
    lean = scan.run(Y, want_lod=False)
    assert "lod" not in lean
    np.testing.assert_array_equal(lean["peak_lod"], full["peak_lod"])
    np.testing.assert_array_equal(lean["peak_index"], full["peak_index"])
    for p in (0, 5, 64, 129):
        alone = scan.run(Y[:, p])
        np.testing.assert_array_equal(alone["lod"][0], full["lod"][p], err_msg=f"phenotype {p} alone")
        np.testing.assert_array_equal(alone["peak_lod"][0], full["peak_lod"][p])
        np.testing.assert_array_equal(alone["peak_index"][0], full["peak_index"][p])
    moved = np.roll(Y, 64, axis=1)                                                # column p -> column p + 64
    got = scan.run(moved)
    np.testing.assert_array_equal(got["lod"], np.roll(full["lod"], 64, axis=0))
    scan.close()


def test_chunks_of_phenotypes_do_not_show():
    """600 phenotypes cross the 512-column chunk: every one has the bits it has alone in a run of 88 from column 512 on."""
    case = (4, 31, 2, 130, cases.POINTS)
    _, _, Y, _ = cases.build(case)
    wide = np.tile(Y, (1, 5))[:, :600]
    scan = scan_of(case)
    got = scan.run(wide)
    tail = scan.run(wide[:, 512:])
    base = scan.run(Y)
    scan.close()
    np.testing.assert_array_equal(got["lod"][512:], tail["lod"])
    np.testing.assert_array_equal(got["peak_index"][512:], tail["peak_index"])
    for k in range(600):
        assert np.array_equal(got["lod"][k], base["lod"][k % 130]), k


@pytest.mark.parametrize("case", [BITS, (9, 33, 1, 63, cases.POINTS)], ids=cases.case_id)
def test_the_cut_of_the_appends_does_not_show(case):
    """The cohort in pieces of 1, of 3 and all at once: the same bits."""
    n = case[1]
    _, _, Y, _ = cases.build(case)
    whole = scan_of(case)
    want = whole.run(Y)
    want_rank = whole.info()["rank"]
    whole.close()
    for size in (1, 3):
        pieces = [size] * (n // size) + ([n % size] if n % size else [])
        scan = scan_of(case, pieces)
        got = scan.run(Y)
        np.testing.assert_array_equal(scan.info()["rank"], want_rank)
        scan.close()
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key}, pieces of {size}")


def test_a_constant_phenotype_scores_zero_everywhere():
    """rss0 == 0: 0.0 at every grid point, whatever the constant, next to ordinary phenotypes that keep their bits."""
    case = (8, 70, 4, 130, (1, 65, 9))
    _, _, Y, _ = cases.build(case)
    scan = scan_of(case)
    want = scan.run(Y[:, :3])
    y = np.column_stack([np.zeros(70), Y[:, 0], np.full(70, 3.7), Y[:, 1], np.full(70, -1e6), Y[:, 2]])
    got = scan.run(y)
    scan.close()
    for p in (0, 2, 4):
        assert (got["lod"][p] == 0.0).all() and (got["peak_lod"][p] == 0.0).all()
        np.testing.assert_array_equal(got["peak_index"][p], [0, 1, 66])              # ties: each chromosome's first point
    np.testing.assert_array_equal(got["lod"][[1, 3, 5]], want["lod"])


def test_append_from_the_hmm_handle():
    """Runs of 25 and of 3 samples on grid "a" (its chromosome X is off the grid): append_from, whole runs or sample by
    sample, leaves what append(hmm.grid()['dosage']) leaves - the same LODs, ranks and peaks bit for bit - whether the
    grid pass ran before it or not.  A chromosome without grid points has no peak: NaN and -1."""
    from gbrs_amd.scan import GenomeScan
    from test_grid_gpu import run_samples
    H = 8
    grid = grid_cases.grids()["a"]
    big, p0 = run_samples(H, "do", range(25))
    small, _ = run_samples(H, "do", range(25, 28))
    for hmm in (big, small):
        hmm.set_grid(grid.positions, grid.points)
    points = big.grid_points
    assert points[-1] == 0 and sum(points) == 193
    rng = np.random.default_rng(5)
    Y = rng.normal(size=(28, 65))
    Z = np.column_stack([np.ones(28), rng.integers(0, 2, size=28)])
    Z[:2, 1] = (0.0, 1.0)
    by_device = GenomeScan(H, points)
    by_device.append_from(big)                                                    # launches the grid kernel itself
    by_device.append_from(small)
    host = [big.grid()["dosage"], small.grid()["dosage"]]
    Y[:, 0] += 4.0 * np.concatenate(host)[:, 100, 2]
    by_host = GenomeScan(H, points)
    for d in host:
        by_host.append(d)
    one_by_one = GenomeScan(H, points)
    for hmm in (big, small):
        for s in range(hmm.n_samples):
            one_by_one.append_from(hmm, sample=s)
    assert by_device.n == by_host.n == one_by_one.n == 28
    results = []
    for scan in (by_device, by_host, one_by_one):
        scan.prepare(Z)
        results.append((scan.run(Y), scan.info()["rank"]))
        scan.close()
    for got, rank in results[1:]:
        np.testing.assert_array_equal(rank, results[0][1])
        for key in got:
            np.testing.assert_array_equal(got[key], results[0][0][key], err_msg=key)
    got = results[0][0]
    assert np.isnan(got["peak_lod"][:, -1]).all() and (got["peak_index"][:, -1] == -1).all()
    assert np.isfinite(got["peak_lod"][:, :-1]).all()
    lod, rank, ratios = cases.scan_rule(np.concatenate(host), Z, Y)
    with np.errstate(invalid="ignore"):
        undecided = int(((ratios >= cases.UNDECIDED[0]) & (ratios <= cases.UNDECIDED[1])).any(axis=1).sum())
    print(f"DEVIATION device against scan_rule on HMM dosages: {cases.deviation(got['lod'], lod):.3g}; ranks differ at "
          f"{int((rank != results[0][1]).sum())} of {len(rank)} grid points, {undecided} with an undecided pivot")
    assert undecided == 0                 # these posteriors put no pivot where rounding could flip a rank, so:
    np.testing.assert_array_equal(results[0][1], rank)
    assert cases.deviation(got["lod"], lod) <= cases.DEVICE_FACTOR * cases.MEASURED_FLOOR
    big.close()
    small.close()


def test_refusals_leave_the_handle_usable():
    """H = 1, too few samples, values that are not finite, a run before prepare, a handle on another grid: GBRS_ERR_INVALID
    with a message that names the trouble, outputs untouched, and the scan goes on as if nothing had been asked."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.scan import GenomeScan
    from test_grid_gpu import run_samples
    lib = _lib.load()
    case = (3, 33, 1, 65, cases.POINTS)
    D, Z, Y, _ = cases.build(case)
    pts = np.asarray(case[4], dtype=np.int32)
    h = C.c_void_p()
    assert lib.gbrs_scan_create(0, 3, _lib.ptr(pts), 1, C.byref(h)) == _lib.GBRS_ERR_INVALID and b"at least 2 founders" in lib.gbrs_last_error()
    assert lib.gbrs_scan_create(0, 3, _lib.ptr(pts), 18, C.byref(h)) == _lib.GBRS_ERR_INVALID and b"at most 17" in lib.gbrs_last_error()
    assert lib.gbrs_scan_create(0, 3, _lib.ptr(np.zeros(3, dtype=np.int32)), 3, C.byref(h)) == _lib.GBRS_ERR_INVALID
    assert not h.value
    with pytest.raises(_lib.GbrsHipError, match="at least 2 founders"):
        GenomeScan(1, case[4])
    scan = GenomeScan(3, case[4])
    lod, peak, index = np.full((65, 17), -1.0), np.full((65, 3), -1.0), np.full((65, 3), -7, dtype=np.int64)
    run = lambda y: lib.gbrs_scan_run(scan._h, y.shape[1], _lib.ptr(y), _lib.ptr(lod), _lib.ptr(peak), _lib.ptr(index))
    untouched = lambda: (lod == -1.0).all() and (peak == -1.0).all() and (index == -7).all()
    Yc = np.ascontiguousarray(Y)
    assert run(Yc) == _lib.GBRS_ERR_INVALID and b"call gbrs_scan_prepare first" in lib.gbrs_last_error() and untouched()
    scan.append(D[:3])
    with pytest.raises(_lib.GbrsHipError, match="3 samples are too few for 1 covariate columns and 3 founders"):
        scan.prepare(Z[:3])
    bad = D[3:].copy()
    bad[4, 9, 1] = np.nan
    with pytest.raises(_lib.GbrsHipError, match=r"dosage of sample 7 holds a value that is not finite \(grid point 9, founder 1\)"):
        scan.append(bad)
    assert scan.info()["n"] == 3 and scan.n == 3
    with pytest.raises(ValueError, match="shape"):
        scan.append(D[3:, :-1])
    scan.append(D[3:])
    q = np.full((33, 1), 1.0 / np.sqrt(33.0))
    q[20, 0] = np.inf
    assert lib.gbrs_scan_prepare(scan._h, 1, _lib.ptr(q)) == _lib.GBRS_ERR_INVALID and b"sample 20, column 0" in lib.gbrs_last_error()
    assert lib.gbrs_scan_prepare(scan._h, 0, _lib.ptr(q)) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_scan_prepare(scan._h, 65, _lib.ptr(q)) == _lib.GBRS_ERR_INVALID
    assert scan.info()["c"] == 0 and scan.info()["rank"] is None
    scan.prepare(Z)
    y = Yc.copy()
    y[30, 2] = -np.inf
    assert run(y) == _lib.GBRS_ERR_INVALID and b"phenotype 2 holds a value that is not finite (sample 30)" in lib.gbrs_last_error()
    assert untouched() and lib.gbrs_scan_run(scan._h, 0, _lib.ptr(Yc), None, None, None) == _lib.GBRS_ERR_INVALID
    with pytest.raises(ValueError, match="phenotypes have shape"):
        scan.run(Y[:-1])
    hmm, _ = run_samples(3, "benign", range(2))
    assert lib.gbrs_scan_append_hmm(scan._h, hmm._h, -1) == _lib.GBRS_ERR_INVALID and b"no grid" in lib.gbrs_last_error()
    grid = grid_cases.grids()["a"]
    hmm.set_grid(grid.positions, grid.points)
    with pytest.raises(_lib.GbrsHipError, match="the HMM handle has 5 chromosomes, the scan 3"):
        scan.append_from(hmm)
    other = GenomeScan(3, [1, 63, 64, 64, 0])
    with pytest.raises(_lib.GbrsHipError, match="grid mismatch: chromosome 3 has 65 grid points on the HMM handle, 64 on the scan"):
        other.append_from(hmm)
    more = GenomeScan(4, hmm.grid_points)
    with pytest.raises(_lib.GbrsHipError, match="the HMM handle has 3 founders, the scan 4"):
        more.append_from(hmm)
    assert lib.gbrs_scan_append_hmm(scan._h, hmm._h, 2) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error()
    assert other.n == more.n == 0 and other.info()["n"] == 0
    for s in (other, more):
        s.close()
    hmm.close()
    assert lib.gbrs_scan_append_hmm(scan._h, None, -1) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_scan_run(None, 1, _lib.ptr(Yc), None, None, None) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_scan_prepare(scan._h, 65, _lib.ptr(q)) == _lib.GBRS_ERR_INVALID      # refused prepares keep the preparation
    assert lib.gbrs_scan_prepare(scan._h, 1, _lib.ptr(q)) == _lib.GBRS_ERR_INVALID and b"sample 20" in lib.gbrs_last_error()
    assert scan.info()["n"] == 33 and scan.info()["c"] == 1 and scan.info()["rank"] is not None
    assert run(Yc) == _lib.GBRS_OK and not untouched()
    assert cases.deviation(lod, cases.expected(case)[0]) <= cases.device_tol(case)
    scan.close()


# ---- the commands --------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES, GRID_FILES, N_FILES = 2, "benign", "b", 6


@pytest.fixture
def tables(tmp_path, monkeypatch):
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid = grid_cases.grids()[GRID_FILES]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    return paths


def cohort_files(tmp_path, stem):
    """The sample file of the six samples, outbases <stem>0 .. <stem>5."""
    lines = []
    for s in range(N_FILES):
        tpm = grid_cases.write_genes_tpm(tmp_path / f"s{s}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, s))
        lines.append(f"{tpm}\t{tmp_path / f'{stem}{s}'}")
    (tmp_path / f"{stem}.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / f"{stem}.txt")


def write_table(path, ids, names, values):
    with open(path, "w") as fh:
        fh.write("id\t" + "\t".join(names) + "\n")
        for i, row in zip(ids, values):
            fh.write(i + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    return str(path)


def test_reconstruct_with_scan_pheno_and_gbrs_scan(tmp_path, tables, caplog, monkeypatch):
    """Six samples in launches of 4, the fourth without a phenotype row: it is logged and left out.  Both files hold what
    GenomeScan gives when driven by hand with the dosages that went through the handle.  `gbrs scan` on the exported
    tables of the same samples agrees to the rounding of the `%.6f` tables; the same reconstruct command without the scan
    options writes byte-identical per-sample files and no scan files."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import DiplotypeHMM
    from gbrs_amd.scan import GenomeScan, rankz
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self.grid_points, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    rng = np.random.default_rng(12)
    names = [f"gene{p}" for p in range(5)]
    values = rng.normal(size=(N_FILES, 5))
    values[:, 4] = 2.5                                                            # a constant phenotype
    sex = np.array([0, 1, 1, 0, 0, 1], dtype=float)
    have = [0, 1, 2, 4, 5]
    sample_file = cohort_files(tmp_path, "with")
    pheno = write_table(tmp_path / "pheno.tsv", [str(tmp_path / f"with{s}") for s in have], names, values[have])
    covar = write_table(tmp_path / "covar.tsv", [str(tmp_path / f"with{s}") for s in range(N_FILES)], ["sex"], sex[:, None])
    common = ["-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--batch-size", "4"]
    with caplog.at_level("WARNING", logger="gbrs"):
        assert cli.main(["reconstruct", "--sample-file", sample_file] + common +
                        ["--scan-pheno", pheno, "--scan-covar", covar, "--scan-rankz", "--scan-out", str(tmp_path / "cohort"),
                         "--scan-lod-matrix"]) == 0
    messages = [r.getMessage() for r in caplog.records]
    assert not any(r.levelname == "ERROR" for r in caplog.records), messages
    assert sum("with3 has no phenotype row and is left out" in m for m in messages) == 1
    assert [len(d) for _, d in seen] == [4, 2]
    points = seen[0][0]
    dosage = np.concatenate([d for _, d in seen])[have]
    scan = GenomeScan(H_FILES, points)
    scan.append(dosage)
    scan.prepare(np.column_stack([np.ones(5), sex[have]]))
    y = np.column_stack([rankz(values[have, p]) for p in range(5)])
    want = scan.run(y)
    rank = scan.info()["rank"]
    scan.close()
    z = np.load(tmp_path / "cohort.scan.npz")
    assert z["phenotypes"].tolist() == names and z["samples"].tolist() == [str(tmp_path / f"with{s}") for s in have]
    assert z["covariates"].tolist() == ["intercept", "sex"] and len(z["chrom"]) == len(z["pos"]) == sum(points)
    np.testing.assert_array_equal(z["rank"], rank)
    for key in ("lod", "peak_lod", "peak_index"):
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)
    assert (z["lod"][4] == 0.0).all()
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid_b = grid_cases.grids()[GRID_FILES]
    on = [c for c in p0.chroms if c in grid_b.points]
    assert z["chrom"].tolist() == [c for c in on for _ in grid_b.points[c]]
    np.testing.assert_array_equal(z["pos"], np.concatenate([grid_b.points[c] for c in on]))
    lines = open(tmp_path / "cohort.scan.peaks.tsv").read().splitlines()
    assert lines[0] == "#phenotype\tchromosome\tposition\tlod\tgenome_wide_max"
    rows = [line.split("\t") for line in lines[1:]]
    chrom_of = [c for c, m in zip(p0.chroms, points) if m]
    assert len(rows) == 5 * len(chrom_of) and sum(int(r[4]) for r in rows) == 5
    k = 0
    for p, name in enumerate(names):
        for ci, c in enumerate(p0.chroms):
            if points[ci]:
                assert rows[k][:2] == [name, c] and float(rows[k][3]) == want["peak_lod"][p, ci]
                assert float(rows[k][2]) == z["pos"][want["peak_index"][p, ci]]
                k += 1
    # the same cohort without the scan options: the same per-sample files, no scan files
    seen.clear()
    plain = cohort_files(tmp_path, "plain")
    assert cli.main(["reconstruct", "--sample-file", plain] + common) == 0
    suffixes = sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("with0."))
    assert suffixes == sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("plain0."))
    assert "interpolated.genoprobs.tsv" in suffixes
    for s in range(N_FILES):
        for suffix in suffixes:
            with open(tmp_path / f"with{s}.{suffix}", "rb") as fa, open(tmp_path / f"plain{s}.{suffix}", "rb") as fb:
                assert fa.read() == fb.read(), (s, suffix)
    assert not [f for f in os.listdir(tmp_path) if ".scan." in f and not f.startswith("cohort.")]
    # -e cannot be scanned
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["reconstruct", "-e", str(tmp_path / "s0.genes.tpm"), "-o", str(tmp_path / "single")] + common[:-2] +
                        ["--scan-pheno", pheno]) == 0
    assert any("one sample (-e) cannot be scanned" in r.getMessage() for r in caplog.records)
    assert not os.path.exists(tmp_path / "single.genoprobs.npz")
    # gbrs scan on the exported tables (grid file order), ids as in the phenotype file
    listing = tmp_path / "list.tsv"
    listing.write_text("".join(f"{tmp_path / f'with{s}'}\t{tmp_path / f'with{s}.interpolated.genoprobs.tsv'}\n" for s in range(N_FILES)))
    assert cli.main(["scan", "--dosage-list", str(listing), "--grid-file", tables["grid"], "--pheno", pheno, "--covar", covar,
                     "--scan-rankz", "--scan-out", str(tmp_path / "tables"), "--scan-lod-matrix"]) == 0
    t = np.load(tmp_path / "tables.scan.npz")
    assert t["samples"].tolist() == z["samples"].tolist() and t["phenotypes"].tolist() == names
    order = list(grid_b.points)                                                   # the grid file's chromosome order
    assert t["chrom"].tolist() == [c for c in order for _ in grid_b.points[c]]
    first = {c: z["chrom"].tolist().index(c) for c in on}
    to_handle = np.concatenate([t["chrom"].tolist().index(c) + np.arange(len(grid_b.points[c])) for c in on])
    assert all(first[c] >= 0 for c in on)
    # A table rounds a dosage by up to 5e-7, a relative change e of the design of a few 1e-6.  rss1 moves by about
    # e rss0, so a LOD moves by (n / 2 / ln 10) e rss0 / rss1, and rss0 / rss1 = 10^(2 lod / n) is known from the LOD
    # itself.  e = 2e-5 leaves an order of magnitude for the conditioning of two residual degrees of freedom.
    ratio = 10.0 ** (2.0 * z["lod"] / 5)
    moved = np.abs(t["lod"][:, to_handle] - z["lod"])
    print(f"DEVIATION gbrs scan on the exported tables against the in-run scan: worst {moved.max():.3g}, "
          f"worst share of its bound {(moved / (5 / 2 / np.log(10) * 2e-5 * ratio)).max():.3g}")
    assert (moved <= 5 / 2 / np.log(10) * 2e-5 * ratio).all()
    assert (t["lod"][4] == 0.0).all()
    assert os.path.getsize(tmp_path / "tables.scan.peaks.tsv") > 0


def test_a_sample_that_moves_to_another_table_file_is_scanned_from_that_handle(tmp_path, monkeypatch):
    """`--alt-tprob-file`: twelve samples in one launch, some of which the alternative explains better and which run again
    under a handle on that file.  The cohort of the scan is the twelve in file order, a moved sample's dosages those of
    its second run: the scan file equals GenomeScan driven by hand with those rows."""
    import loglik_cases
    from gbrs_amd.hmm import DiplotypeHMM, ReconstructContext, reconstruct_many
    from gbrs_amd.scan import GenomeScan
    H, style, n = loglik_cases.COMMAND_H, loglik_cases.COMMAND_STYLE, 12
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, grid_cases.problem(H, style), grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    alt = loglik_cases.write_candidate(tmp_path / "x_only.npz", H, style, "x_only")
    seen = []
    grid0 = DiplotypeHMM.grid

    def grid_pass(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen.append((self, out["dosage"].copy()))
        return out

    monkeypatch.setattr(DiplotypeHMM, "grid", grid_pass)
    tpms = [grid_cases.write_genes_tpm(tmp_path / f"s{s}.genes.tpm", grid_cases.sample_problem(H, style, s)) for s in range(n)]
    outbases = [str(tmp_path / f"alt{s}") for s in range(n)]
    y = np.random.default_rng(31).normal(size=(n, 3))
    pheno = write_table(tmp_path / "pheno.tsv", outbases, ["a", "b", "c"], y)
    ctx = ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"], grid_file=paths["grid"], alt_tprob_files=[alt])
    times = {}
    done = reconstruct_many(tpms, outbases, paths["tprob"], context=ctx, scan_pheno=pheno, scan_out=str(tmp_path / "alt"),
                            model_report=str(tmp_path / "models.tsv"), stage_times=times)
    assert not any("error" in d for d in done) and times["scan"] > 0
    report = [line.split("\t") for line in open(tmp_path / "models.tsv").read().splitlines() if not line.startswith("#")]
    assert [f[0] for f in report] == outbases
    moved = [s for s in range(n) if report[s][1] != paths["tprob"]]
    assert 0 < len(moved) < n
    base, other = ctx.hmm, ctx.alt_context(0).hmm
    assert seen[0][0] is base and len(seen[0][1]) == n and len(seen) == 1 + len(moved)
    assert all(h is other and len(d) == 1 for h, d in seen[1:])
    rows = np.stack([seen[1 + moved.index(s)][1][0] if s in moved else seen[0][1][s] for s in range(n)])
    scan = GenomeScan(H, base.grid_points)
    scan.append(rows)
    scan.prepare()
    want = scan.run(y)
    rank = scan.info()["rank"]
    scan.close()
    ctx.close()
    z = np.load(tmp_path / "alt.scan.npz")
    assert z["samples"].tolist() == outbases and z["covariates"].tolist() == ["intercept"]
    np.testing.assert_array_equal(z["rank"], rank)
    for key in ("lod", "peak_lod", "peak_index"):
        np.testing.assert_array_equal(z[key], want[key], err_msg=key)


def test_a_sample_whose_files_cannot_be_written_is_left_out(tmp_path, tables, caplog):
    """Six samples in launches of 4; the outbase of the second lies in a directory that does not exist.  Its write fails:
    it is reported once as failed and the scan holds the other five, in file order."""
    from gbrs_amd.hmm import reconstruct_many
    tpms = [grid_cases.write_genes_tpm(tmp_path / f"s{s}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, s))
            for s in range(N_FILES)]
    outbases = [str(tmp_path / f"w{s}") for s in range(N_FILES)]
    outbases[1] = str(tmp_path / "no_such_directory" / "w1")
    pheno = write_table(tmp_path / "pheno.tsv", outbases, ["a", "b"], np.random.default_rng(8).normal(size=(N_FILES, 2)))
    with caplog.at_level("ERROR", logger="gbrs"):
        done = reconstruct_many(tpms, outbases, tables["tprob"], tables["avecs"], tables["gpos"], batch_size=4,
                                grid_file=tables["grid"], scan_pheno=pheno, scan_out=str(tmp_path / "five"))
    assert ["error" in d for d in done] == [False, True, False, False, False, False]
    assert sum("no_such_directory" in r.getMessage() for r in caplog.records) == 1
    z = np.load(tmp_path / "five.scan.npz")
    assert z["samples"].tolist() == outbases[:1] + outbases[2:] and z["lod"].shape[0] == 2
