"""The match pass of the HIP HMM (gbrs_hmm_set_panel / gbrs_hmm_match) and `gbrs reconstruct --match-panel` over it
(needs an MI355X).  Shapes, grids and samples: tests/grid_cases.py; panels and the restatement: tests/match_cases.py.

The restatement is numpy on the device's own dosages (hmm.grid()['dosage']) and the uploaded panel: per chromosome
np.einsum('sph,jph->sj') and the two sums of squares.  Each sum has K = points_c x H non-negative terms, so whatever the
order, fused or not, it is within a relative (K + 1) 2^-53 of the exact value: the device and numpy agree to
rtol = 4 K 2^-53, atol = 0, and a sum of zeros is 0.0 on both sides."""
import os

import numpy as np
import pytest

import grid_cases
import match_cases as cases

pytestmark = pytest.mark.gpu

# founders x samples per run x panel entries.  Between them: 1, 3, 8 and 16 founders (K = 1 and 3 on the one-point
# chromosome, the 8-byte and the 16-byte staging), 1, 3, 16, 17 and 25 samples (one short, full, one into a second 16-row
# tile), 1, 15, 16, 17, 40 and 65 entries (the same around a column tile, and one entry into a second 64-entry block).
# Grids "a" and "b" bring chromosomes of 1, 63, 64, 65 and 130 points, a handle chromosome off the grid and a grid
# order that is not the handle's.
TABLE = [(1, 1, 1), (1, 3, 15), (3, 3, 16), (3, 17, 17), (8, 1, 40), (8, 16, 65), (8, 17, 16), (8, 25, 65), (16, 3, 17),
         (16, 1, 15)]


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_")):
            monkeypatch.delenv(k, raising=False)


def run_samples(H, style, samples):
    from test_grid_gpu import run_samples as run
    return run(H, style, samples)


def run_one_hot(H, n, first=0):
    """A handle whose posteriors are one-hot: emissions -inf off one state, another one per sample and chromosome.  The
    sample at position s is sample first + s of the family, whatever the size of the run."""
    from gbrs_amd.hmm import DiplotypeHMM
    p0 = grid_cases.problem(H, "benign")
    S = H * (H + 1) // 2
    hmm = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    state = lambda s, ci: (5 * (first + s) + 3 * ci + 1) % S
    eprob = []
    for ci, c in enumerate(p0.chroms):
        e = np.full((n, len(p0.gene_ids[c]), S), -np.inf)
        for s in range(n):
            e[s, :, state(s, ci)] = 0.0
        eprob.append(e)
    hmm.set_eprob(eprob)
    hmm.run()
    return hmm, p0, state


def assert_sums(got, info, want, points, H, at):
    cross, snorm, pnorm = want
    for c, m in enumerate(points):
        rt = cases.rtol(m, H)
        np.testing.assert_allclose(got["cross"][..., c, :], cross[..., c, :], rtol=rt, atol=0, err_msg=f"cross, {at} chromosome {c}")
        np.testing.assert_allclose(got["sample_norm"][..., c], snorm[..., c], rtol=rt, atol=0, err_msg=f"sample_norm, {at} chromosome {c}")
        np.testing.assert_allclose(info["panel_norm"][:, c], pnorm[:, c], rtol=rt, atol=0, err_msg=f"panel_norm, {at} chromosome {c}")
        if m == 0:
            assert (got["cross"][..., c, :] == 0.0).all() and (got["sample_norm"][..., c] == 0.0).all() and \
                (info["panel_norm"][:, c] == 0.0).all(), f"{at}: chromosome {c} is off the grid"


@pytest.mark.parametrize("H,n,M", TABLE)
def test_sums_against_the_restatement(H, n, M):
    """Every (sample, chromosome, entry) on both grids against numpy on the device's own dosages.  The pass runs before
    grid() here (it launches the grid kernel itself) and again after it (it takes grid()'s dosages): bit-equal, and so are
    two identical calls and the last sample asked for alone."""
    hmm, p0 = run_samples(H, "do", range(n))
    rng = np.random.default_rng(100 * H + M)
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        points, offsets = cases.handle_points(p0.chroms, grid)
        hmm.set_grid(grid.positions, grid.points)
        assert hmm.match_info()["n_panel"] == 0
        panel = cases.random_panel(rng, M, sum(points), H)
        panel[M // 2][offsets[1]:offsets[1] + points[1]] = 0.0          # an entry that is all zeros on one chromosome
        hmm.set_panel(panel)
        first = hmm.match()
        info = hmm.match_info()
        assert info["n_panel"] == M and first["cross"].shape == (n, len(p0.chroms), M) and first["sample_norm"].shape == (n, len(p0.chroms))
        assert info["device_bytes"] >= 8 * M * sum(points) * H
        dosage = hmm.grid()["dosage"]
        want = cases.restate(dosage, panel, points, offsets)
        assert_sums(first, info, want, points, H, f"grid {name}")
        worst = max(float(np.max(np.abs(first["cross"][:, c] - want[0][:, c]) / np.maximum(want[0][:, c], 1e-300)))
                    for c, m in enumerate(points) if m)
        print(f"DEVIATION cross against numpy, H={H} n={n} M={M} grid {name}: {worst:.3g}")
        if points[1]:
            assert (first["cross"][:, 1, M // 2] == 0.0).all() and info["panel_norm"][M // 2, 1] == 0.0
        for again in (hmm.match(), hmm.match()):                        # after grid(): its dosages, no grid launch
            np.testing.assert_array_equal(again["cross"], first["cross"])
            np.testing.assert_array_equal(again["sample_norm"], first["sample_norm"])
        one = hmm.match(sample=n - 1)
        np.testing.assert_array_equal(one["cross"], first["cross"][n - 1])
        np.testing.assert_array_equal(one["sample_norm"], first["sample_norm"][n - 1])
        whole = hmm.match()                                              # grid_dosage holds one sample now: made again
        np.testing.assert_array_equal(whole["cross"], first["cross"])
    hmm.close()


@pytest.mark.parametrize("H,n,M", [(1, 1, 1), (3, 3, 17), (8, 1, 16), (8, 25, 65), (16, 17, 15)])
def test_exact_values_are_exact(H, n, M):
    """One-hot posteriors give dosages in {0, 1/2, 1}; with a panel of such values every product and every sum is
    exactly representable, and the three sums equal the restatement with ==.  An entry that has, on every chromosome, a
    founder the sample does not carry there gives exactly 0.0."""
    hmm, p0, state = run_one_hot(H, n)
    pairs = cases.states(H)
    rng = np.random.default_rng(7 * H + M)
    for name in ("a", "b"):
        grid = grid_cases.grids()[name]
        points, offsets = cases.handle_points(p0.chroms, grid)
        hmm.set_grid(grid.positions, grid.points)
        panel = cases.one_hot_panel(rng, M, sum(points), H)
        if H >= 3:                                                      # the last entry: disjoint from sample 0
            d = np.zeros((sum(points), H))
            for ci, (m, o) in enumerate(zip(points, offsets)):
                free = [f for f in range(H) if f not in pairs[state(0, ci)]]
                d[o:o + m, free[0]] = 1.0
            panel[-1] = d
        hmm.set_panel(panel)
        got, info = hmm.match(), hmm.match_info()
        dosage = hmm.grid()["dosage"]
        assert np.isin(dosage, (0.0, 0.5, 1.0)).all(), "the dosages of this case are not exact"
        cross, snorm, pnorm = cases.restate(dosage, panel, points, offsets)
        np.testing.assert_array_equal(got["cross"], cross)
        np.testing.assert_array_equal(got["sample_norm"], snorm)
        np.testing.assert_array_equal(info["panel_norm"], pnorm)
        assert (snorm[:, [c for c, m in enumerate(points) if m]] > 0).all()
        if H >= 3:
            assert (got["cross"][0, :, -1] == 0.0).all() and (pnorm[-1] == np.asarray(points, dtype=float)).all()
    hmm.close()


def test_a_samples_numbers_do_not_depend_on_its_launch_or_on_the_panels_size():
    """25 samples of the "do" family against 40 entries: a sample's rows equal, bit for bit, the rows of match(sample=s)
    and the rows with the panel truncated to its first 17 entries over those 17 columns.
    A run of 7 against a run of 25: the HMM takes another route for another batch size and its posteriors differ in the
    last bits, so the runs compared here have one-hot posteriors - dosages in {0, 1/2, 1}, the same in every run - against
    a panel of random doubles, whose sums round and therefore depend on the order: samples 18 .. 24 at positions 0 .. 6 of
    a run of 7 have the rows they had at positions 18 .. 24 of the run of 25."""
    H, M = 8, 40
    grid = grid_cases.grids()["b"]
    hmm, p0 = run_samples(H, "do", range(25))
    points, offsets = cases.handle_points(p0.chroms, grid)
    panel = cases.random_panel(np.random.default_rng(11), M, sum(points), H)
    hmm.set_grid(grid.positions, grid.points)
    hmm.set_panel(panel)
    full = hmm.match()
    for s in (0, 15, 16, 24):
        one = hmm.match(sample=s)
        np.testing.assert_array_equal(one["cross"], full["cross"][s], err_msg=f"sample {s} alone")
        np.testing.assert_array_equal(one["sample_norm"], full["sample_norm"][s], err_msg=f"sample {s} alone")
    norms = hmm.match_info()["panel_norm"]
    hmm.set_panel(panel[:17])
    fewer = hmm.match()
    np.testing.assert_array_equal(fewer["cross"], full["cross"][:, :, :17])
    np.testing.assert_array_equal(fewer["sample_norm"], full["sample_norm"])
    np.testing.assert_array_equal(hmm.match_info()["panel_norm"], norms[:17])
    hmm.close()
    big, _, _ = run_one_hot(H, 25)
    big.set_grid(grid.positions, grid.points)
    big.set_panel(panel)
    want = big.match()
    big.close()
    on_x = np.stack(panel)[:, offsets[4]:offsets[4] + points[4]].reshape(M, -1)
    assert any(np.cumsum(x)[-1] != np.cumsum(x[::-1])[-1] for x in on_x), "the sums of this case do not depend on the order"
    assert len(np.unique(want["cross"][18:, 4, :])) > 7 * M // 2
    small, _, _ = run_one_hot(H, 7, first=18)
    small.set_grid(grid.positions, grid.points)
    small.set_panel(panel)
    got = small.match()
    small.close()
    np.testing.assert_array_equal(got["cross"], want["cross"][18:])
    np.testing.assert_array_equal(got["sample_norm"], want["sample_norm"][18:])


def test_planted_identity():
    """The panel holds the run's own samples - their dosages rounded as the `%.6f` text of a dosage table rounds them - in
    shuffled order among unrelated entries (seed: match_cases.planted_seed, chosen on the CPU with the composed oracle).
    Every sample's best entry is its own, closer than the rounding H (0.5e-6)^2 4, and ahead of the second by 1e-3 on
    the restatement's numbers."""
    from gbrs_amd.hmm import match_scores, rank_matches
    H, n = cases.PLANTED_H, cases.PLANTED_SAMPLES
    grid = grid_cases.grids()[cases.PLANTED_GRID]
    hmm, p0 = run_samples(H, cases.PLANTED_STYLE, range(n))
    points, offsets = cases.handle_points(p0.chroms, grid)
    hmm.set_grid(grid.positions, grid.points)
    dosage = hmm.grid()["dosage"]
    ids, panel, where = cases.planted_panel(dosage, cases.planted_seed())
    hmm.set_panel(panel)
    got, info = hmm.match(), hmm.match_info()
    hmm.close()
    best, margin, restated = cases.margins(dosage, panel, points, offsets)
    print(f"margins on the restatement's numbers: {np.round(margin, 4).tolist()}")
    assert best == where and min(margin) >= cases.PLANTED_MARGIN
    distance, _ = match_scores(got["cross"], got["sample_norm"], info["panel_norm"], points, np.asarray(points) > 0)
    for s in range(n):
        r = rank_matches(ids, distance[s], f"animal{s}")
        assert r["status"] == "match" and r["best"] == f"animal{s}" == ids[where[s]]
        assert r["best_distance"] < H * 0.5e-6 ** 2 * 4
        assert r["margin"] >= cases.PLANTED_MARGIN


def test_raw_call_statuses():
    """A match before a run: GBRS_ERR_STATE.  A panel without a grid, a match without a panel, a sample out of range, an
    entry with a NaN: GBRS_ERR_INVALID, outputs untouched, the handle as it was.  set_grid and n_panel = 0 drop the panel.
    A good call after the bad ones."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.hmm import DiplotypeHMM
    lib = _lib.load()
    H, n, M = 3, 2, 5
    p0 = grid_cases.problem(H, "benign")
    grid = grid_cases.grids()["a"]
    points, offsets = cases.handle_points(p0.chroms, grid)
    panel = cases.random_panel(np.random.default_rng(3), M, sum(points), H)
    nc = len(p0.chroms)
    cross, norm = np.full((n, nc, M), -1.0), np.full((n, nc), -1.0)

    def match(h, sample=-1):
        return lib.gbrs_hmm_match(h._h, sample, _lib.ptr(cross), _lib.ptr(norm))

    def set_panel(h, arrays):
        return lib.gbrs_hmm_set_panel(h._h, len(arrays), _lib.ptr_table(arrays))

    def untouched():
        return (cross == -1.0).all() and (norm == -1.0).all()

    fresh = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    assert match(fresh) == _lib.GBRS_ERR_STATE and untouched()
    assert set_panel(fresh, panel) == _lib.GBRS_ERR_INVALID and b"no grid" in lib.gbrs_last_error()
    fresh.close()
    hmm, _ = run_samples(H, "benign", range(n))
    assert set_panel(hmm, panel) == _lib.GBRS_ERR_INVALID and b"no grid" in lib.gbrs_last_error()
    hmm.set_grid(grid.positions, grid.points)
    assert match(hmm) == _lib.GBRS_ERR_INVALID and b"no panel" in lib.gbrs_last_error() and untouched()
    with pytest.raises(_lib.GbrsHipError):
        hmm.match()
    assert set_panel(hmm, panel) == _lib.GBRS_OK
    for sample in (n, -2, 25):
        assert match(hmm, sample) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error() and untouched()
    bad = [a.copy() for a in panel[:3]]
    bad[1][5, 2] = np.nan
    assert set_panel(hmm, bad) == _lib.GBRS_ERR_INVALID and b"entry 1" in lib.gbrs_last_error()
    bad[1][5, 2] = np.inf
    assert set_panel(hmm, bad) == _lib.GBRS_ERR_INVALID and b"entry 1" in lib.gbrs_last_error()
    assert lib.gbrs_hmm_set_panel(hmm._h, -1, None) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_hmm_set_panel(hmm._h, 2, None) == _lib.GBRS_ERR_INVALID
    assert hmm.match_info()["n_panel"] == M                              # the failed calls left the panel of five
    assert match(hmm) == _lib.GBRS_OK and not untouched()
    want = cases.restate(hmm.grid()["dosage"], panel, points, offsets)
    assert_sums({"cross": cross, "sample_norm": norm}, hmm.match_info(), want, points, H, "after the refusals")
    assert lib.gbrs_hmm_match(hmm._h, 1, None, None) == _lib.GBRS_OK
    one = np.full((1, nc, M), -1.0)
    assert lib.gbrs_hmm_match(hmm._h, 1, _lib.ptr(one), None) == _lib.GBRS_OK
    np.testing.assert_array_equal(one[0], cross[1])
    m, ms, nbytes = C.c_int32(), C.c_double(), C.c_uint64()
    assert lib.gbrs_hmm_match_info(hmm._h, C.byref(m), None, C.byref(ms), C.byref(nbytes)) == _lib.GBRS_OK
    assert m.value == M and ms.value > 0 and nbytes.value > 0
    cross[:], norm[:] = -1.0, -1.0
    hmm.set_grid(grid.positions, grid.points)                            # a new grid drops the panel
    assert hmm.match_info()["n_panel"] == 0 and match(hmm) == _lib.GBRS_ERR_INVALID and untouched()
    assert set_panel(hmm, panel) == _lib.GBRS_OK and hmm.match_info()["n_panel"] == M
    assert set_panel(hmm, []) == _lib.GBRS_OK and hmm.match_info()["n_panel"] == 0
    assert match(hmm) == _lib.GBRS_ERR_INVALID and untouched()
    with pytest.raises(ValueError, match="shape"):
        hmm.set_panel([panel[0][:-1]])
    hmm.set_panel(panel)
    rows = grid_cases.expression_rows(grid_cases.sample_problem(H, "benign", 2))
    hmm.set_expression(rows, expr_threshold=1.5, sigma=0.12)             # new samples on the handle, no run yet
    assert match(hmm) == _lib.GBRS_ERR_STATE and untouched()
    hmm.run()
    got = hmm.match()
    want = cases.restate(hmm.grid()["dosage"], panel, points, offsets)
    assert_sums(got, hmm.match_info(), want, points, H, "after a new run")
    assert lib.gbrs_hmm_match(None, -1, None, None) == _lib.GBRS_ERR_INVALID
    hmm.close()


# ---- the command -----------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES = cases.PLANTED_H, cases.PLANTED_STYLE


@pytest.fixture
def tables(tmp_path, monkeypatch):
    """$GBRS_DATA with the 8-founder problem and a grid file of grid "b" (its chromosome order is not the genome's)."""
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    return paths


@pytest.fixture
def seen(monkeypatch):
    """What went through the handles: every grid() call's dosages (as [n, P, H]) and every uploaded panel."""
    from gbrs_amd.hmm import DiplotypeHMM
    seen = {"dosage": [], "panel": []}
    grid0, panel0 = DiplotypeHMM.grid, DiplotypeHMM.set_panel

    def grid(self, sample=None, want=("dosage",)):
        out = grid0(self, sample=sample, want=want)
        seen["dosage"].append((self, out["dosage"].copy() if sample is None else out["dosage"][None].copy()))
        return out

    def set_panel(self, arrays):
        arrays = list(arrays)
        seen["panel"].append((self, [np.array(a) for a in arrays]))
        return panel0(self, arrays)

    monkeypatch.setattr(DiplotypeHMM, "grid", grid)
    monkeypatch.setattr(DiplotypeHMM, "set_panel", set_panel)
    return seen


def sample_tpm(tmp_path, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, sample))


def file_panel(tmp_path, samples):
    """A panel file with the oracle's rounded dosages of `samples` (ids animal<sample>) and ten unrelated entries, shuffled.
    Returns (path, ids)."""
    own = np.stack([grid_cases.expected_for(H_FILES, STYLE_FILES, s, "b")[1] for s in samples])      # grid file order
    ids, arrays, _ = cases.planted_panel(own, cases.planted_seed())
    ids = [f"animal{samples[int(x[6:])]}" if x.startswith("animal") else x for x in ids]
    return cases.write_panel(tmp_path, ids, arrays, grid_cases.problem(H_FILES, STYLE_FILES).hap_names), ids


def expected_of(dosage, panel, ids, expected, names=None):
    """What the host functions make of the restatement's sums for one sample: (cross, sample_norm, panel_norm, distance,
    similarity, rank, absolute tolerance of a distance, relative tolerance of a sum or a similarity)."""
    from gbrs_amd.hmm import match_chromosome_mask, match_scores, rank_matches
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    points, offsets = cases.handle_points(p0.chroms, grid_cases.grids()["b"])
    cross, snorm, pnorm = cases.restate(dosage[None], panel, points, offsets)
    use = match_chromosome_mask(p0.chroms, points, names)
    distance, similarity = match_scores(cross[0], snorm[0], pnorm, points, use)
    rt = cases.rtol(max(points), H_FILES)
    # a distance is (A + B - 2 X) / n of sums that each carry rt: absolutely rt (A + B + 2 X) / n <= 4 rt max(A, B) / n
    atol = 4 * rt * max(snorm[0].sum(), pnorm.sum(axis=1).max()) / sum(points)
    return cross[0], snorm[0], pnorm, distance, similarity, rank_matches(ids, distance, expected), atol, rt


def read_match_table(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "#panel_id\tdistance\tsimilarity"
    fields = [line.split("\t") for line in lines[1:]]
    assert all(len(f) == 3 and repr(float(f[1])) == f[1] and repr(float(f[2])) == f[2] for f in fields)
    return [f[0] for f in fields], np.array([float(f[1]) for f in fields]), np.array([float(f[2]) for f in fields])


def assert_match_table(path, ids, want):
    _, _, _, distance, similarity, rank, atol, rt = want
    got_ids, got_distance, got_similarity = read_match_table(path)
    assert got_ids == [ids[j] for j in rank["order"]]
    np.testing.assert_allclose(got_distance, distance[rank["order"]], rtol=0, atol=atol)
    np.testing.assert_allclose(got_similarity, similarity[rank["order"]], rtol=4 * rt, atol=0)
    assert (np.diff(got_distance) >= 0).all()


def test_a_single_sample_with_an_expected_id(tmp_path, tables, seen, caplog):
    from gbrs_amd import cli
    sample = 3
    panel_file, ids = file_panel(tmp_path, [1, 3, 5])
    common = ["reconstruct", "-v", "-e", sample_tpm(tmp_path, sample), "-t", tables["tprob"], "-x", tables["avecs"], "-g",
              tables["gpos"], "--grid-file", tables["grid"], "--match-panel", panel_file]
    with caplog.at_level("INFO", logger="gbrs"):
        assert cli.main(common + ["-o", str(tmp_path / "one"), "--match-expected", "animal3"]) == 0
        assert cli.main(common + ["-o", str(tmp_path / "auto"), "--match-expected", "animal5", "--match-chromosomes", "2,3,4"]) == 0
        assert cli.main(common + ["-o", str(tmp_path / "bad"), "--match-chromosomes", "2,Q"]) == 0
    messages = [r.getMessage() for r in caplog.records]
    assert not any(r.levelname == "ERROR" for r in caplog.records if "Q is not" not in r.getMessage())
    assert sum("Q is not a chromosome" in m for m in messages) == 1 and not os.path.exists(tmp_path / "bad.genoprobs.npz")
    assert sum("Panel match: match, best animal3" in m for m in messages) == 1
    assert sum("Panel match: mismatch, best animal3" in m for m in messages) == 1
    assert len(seen["dosage"]) == 2 and len(seen["panel"]) == 2
    for k, (stem, names) in enumerate((("one", None), ("auto", "2,3,4"))):
        want = expected_of(seen["dosage"][k][1][0], seen["panel"][k][1], ids, None, names)
        assert_match_table(tmp_path / f"{stem}.match.tsv", ids, want)
        assert os.path.getsize(tmp_path / f"{stem}.interpolated.genoprobs.tsv") > 0


def test_a_cohort_with_labels_report_and_matrix(tmp_path, tables, seen, caplog):
    """25 samples in launches of 7 with one unreadable entry: every sample's .match.tsv, the report and the matrix file
    are what the host functions make of the restatement's sums; the first seven are labelled with their own entry, one
    with another sample's, one with an id the panel lacks, the rest not at all."""
    from gbrs_amd import cli
    cohort = grid_cases.cohort(H_FILES, STYLE_FILES, 25)
    panel_file, ids = file_panel(tmp_path, list(cohort[:7]))
    lines, labels = ["# genes.tpm\toutbase", ""], ["# outbase\tpanel id"]
    for k, sample in enumerate(cohort):
        lines.append(f"{sample_tpm(tmp_path, sample)}\t{tmp_path / f'many{k}'}")
        if k == 9:
            lines.append(f"{tmp_path / 'missing.genes.tpm'}\t{tmp_path / 'missing'}")
    expected = {k: f"animal{cohort[k]}" for k in range(7)}
    expected[7], expected[8] = f"animal{cohort[0]}", "nobody"
    labels += [f"{tmp_path / f'many{k}'}\t{v}" for k, v in expected.items()] + [f"{tmp_path / 'missing'}\tanimal{cohort[1]}"]
    (tmp_path / "samples.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "labels.txt").write_text("\n".join(labels) + "\n")
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "--batch-size", "7", "-t", tables["tprob"],
                         "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--match-panel", panel_file,
                         "--match-labels", str(tmp_path / "labels.txt"), "--match-report", str(tmp_path / "report.tsv"),
                         "--match-matrix", str(tmp_path / "matrix.npz")]) == 0
    errors = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(errors) == 1 and "missing.genes.tpm" in errors[0]
    assert not os.path.exists(tmp_path / "missing.match.tsv")
    assert [len(d) for _, d in seen["dosage"]] == [7, 7, 7, 4] and len(seen["panel"]) == 1
    dosage, panel = np.concatenate([d for _, d in seen["dosage"]]), seen["panel"][0][1]
    report = open(tmp_path / "report.tsv").read().splitlines()
    assert report[0] == ("#outbase\texpected\tstatus\tbest\tbest_distance\tsecond\tsecond_distance\tmargin\texpected_distance\t"
                         "expected_rank") and len(report) == 26
    z = np.load(tmp_path / "matrix.npz")
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    points, _ = cases.handle_points(p0.chroms, grid_cases.grids()["b"])
    assert z["outbases"].tolist() == [str(tmp_path / f"many{k}") for k in range(25)] and z["panel_ids"].tolist() == ids
    assert z["chromosomes"].tolist() == list(p0.chroms) and z["points"].tolist() == points
    assert z["distance"].shape == z["similarity"].shape == (25, len(ids))
    statuses = []
    for k in range(25):
        want = expected_of(dosage[k], panel, ids, expected.get(k))
        cross, snorm, pnorm, distance, similarity, rank, atol, rt = want
        assert_match_table(tmp_path / f"many{k}.match.tsv", ids, want)
        for c, m in enumerate(points):
            r = cases.rtol(m, H_FILES)
            np.testing.assert_allclose(z["cross"][k, c], cross[c], rtol=r, atol=0)
            np.testing.assert_allclose(z["sample_norm"][k, c], snorm[c], rtol=r, atol=0)
            np.testing.assert_allclose(z["panel_norm"][:, c], pnorm[:, c], rtol=r, atol=0)
        np.testing.assert_allclose(z["distance"][k], distance, rtol=0, atol=atol)
        np.testing.assert_allclose(z["similarity"][k], similarity, rtol=4 * rt, atol=0)
        f = report[1 + k].split("\t")
        assert len(f) == 10
        assert f[:4] == [str(tmp_path / f"many{k}"), rank["expected"], rank["status"], rank["best"]] and f[5] == rank["second"]
        assert int(f[9]) == rank["expected_rank"]
        got = np.array([float(f[4]), float(f[6]), float(f[7])])
        np.testing.assert_allclose(got, [rank["best_distance"], rank["second_distance"], rank["margin"]], rtol=0, atol=2 * atol)
        if rank["expected_rank"]:
            assert abs(float(f[8]) - rank["expected_distance"]) <= atol
        else:
            assert f[8] == "nan"
        statuses.append(f[2])
    assert statuses == ["match"] * 7 + ["mismatch", "unknown-label"] + ["unlabelled"] * 16
    assert [report[1 + k].split("\t")[3] for k in range(7)] == [f"animal{cohort[k]}" for k in range(7)]


def test_a_sample_that_moves_to_another_table_file_is_matched_there(tmp_path, monkeypatch, seen):
    """`--alt-tprob-file`: a sample that the alternative explains better runs again under a handle on that file, and its
    match comes from that handle's dosages; the panel went to the two handles once each."""
    import loglik_cases
    import loglik_restate
    from gbrs_amd.hmm import ReconstructContext, choose_tables, reconstruct_many
    H, style, n = loglik_cases.COMMAND_H, loglik_cases.COMMAND_STYLE, loglik_cases.COMMAND_SAMPLES
    assert (H, style) == (H_FILES, STYLE_FILES)
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, grid_cases.problem(H, style), grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    alt = loglik_cases.write_candidate(tmp_path / "x_only.npz", H, style, "x_only")
    best, _ = choose_tables(loglik_restate.totals(H, style, range(n), ("base", "x_only")))
    assert (best == 0).any() and (best == 1).any()
    panel_file, ids = file_panel(tmp_path, list(range(n)))
    ctx = ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"], grid_file=paths["grid"], alt_tprob_files=[alt])
    times = {}
    done = reconstruct_many([sample_tpm(tmp_path, s) for s in range(n)], [str(tmp_path / f"alt{s}") for s in range(n)],
                            paths["tprob"], context=ctx, match_panel=panel_file, stage_times=times)
    assert not any("error" in d for d in done) and times["match"] > 0
    assert ctx.panel_uploads == 2 and len(seen["panel"]) == 2
    base, other = ctx.hmm, ctx.alt_context(0).hmm
    assert base.match_info()["n_panel"] == other.match_info()["n_panel"] == len(ids)
    assert seen["dosage"][0][0] is base and all(h is other and len(d) == 1 for h, d in seen["dosage"][1:])
    moved = [s for s in range(n) if best[s] == 1]
    assert len(seen["dosage"]) == 1 + len(moved)
    for s in range(n):
        dosage = seen["dosage"][1 + moved.index(s)][1][0] if s in moved else seen["dosage"][0][1][s]
        assert_match_table(tmp_path / f"alt{s}.match.tsv", ids, expected_of(dosage, seen["panel"][0][1], ids, None))
    ctx.close()


def test_without_the_options_nothing_changes(tmp_path, tables):
    """A `--grid-file` cohort run without the new options: the files of two runs of the same command are byte-identical,
    there is no match file, no `match` stage, and the handle reports no panel."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import ReconstructContext, reconstruct_many
    tpms = [sample_tpm(tmp_path, s) for s in range(3)]
    for run in ("first", "second"):
        (tmp_path / f"{run}.txt").write_text("".join(f"{tpms[s]}\t{tmp_path / f'{run}{s}'}\n" for s in range(3)))
        assert cli.main(["reconstruct", "--sample-file", str(tmp_path / f"{run}.txt"), "--batch-size", "2", "-t", tables["tprob"],
                         "-x", tables["avecs"], "-g", tables["gpos"], "--grid-file", tables["grid"], "--grid-genoprobs"]) == 0
    suffixes = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz", "interpolated.genoprobs.tsv", "interpolated.genoprobs.npz")
    for s in range(3):
        for suffix in suffixes:
            with open(tmp_path / f"first{s}.{suffix}", "rb") as fa, open(tmp_path / f"second{s}.{suffix}", "rb") as fb:
                assert fa.read() == fb.read(), (s, suffix)
    assert sorted(f.split(".", 1)[1] for f in os.listdir(tmp_path) if f.startswith("first0.")) == sorted(suffixes)
    ctx = ReconstructContext(tables["tprob"], tables["avecs"], tables["gpos"], grid_file=tables["grid"])
    times = {}
    reconstruct_many(tpms, [str(tmp_path / f"held{s}") for s in range(3)], tables["tprob"], context=ctx, batch_size=2,
                     grid_genoprobs=True, stage_times=times)
    info = ctx.hmm.match_info()
    assert info["n_panel"] == 0 and info["device_bytes"] == 0 and info["last_ms"] == 0.0 and "match" not in times
    assert ctx.panel is None and ctx.panel_uploads == 0
    for s in range(3):
        for suffix in suffixes:
            with open(tmp_path / f"first{s}.{suffix}", "rb") as fa, open(tmp_path / f"held{s}.{suffix}", "rb") as fb:
                assert fa.read() == fb.read(), (s, suffix)
    ctx.close()
