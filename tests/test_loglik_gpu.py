"""The log-likelihood pass on the device (gbrs_hmm_loglik, gbrs_hmm_loglik_tables, `gbrs reconstruct --loglik /
--alt-tprob-file / --model-report`; needs an MI355X).  The definition: tests/loglik_restate.py; its agreement
with the oracle's scaler and the margins of the selection fixtures: tests/test_loglik_cpu.py.

Tolerances.  Against the restatement: RTOL.  It started as the project's 1e-8 for posteriors against the reference; the
largest relative deviation these tests then met on an MI355X was 1.06e-15 (H = 2, 25 samples, "do"), seven orders inside it,
so the bound stands at ten times that.  Against the device's own scaler row,
summed on the host: the same numbers in another order, so n_c * 2^-53 * sum |scaler_i| absolute."""
import os

import numpy as np
import pytest

import grid_cases
import loglik_cases as cases
import loglik_restate as restate

pytestmark = pytest.mark.gpu

RTOL = 1.1e-14
# founders x samples: 1 and 3 samples take the sequential chains (the blocked scan at 8 founders), 25 the two-samples-per-wave
# chains; the candidate chain keeps its table columns in registers up to 8 founders (8, 8, 8 and 36 of them for 1, 3, 6 and
# 36 states) and streams them through L2 at 16
TABLE = [(H, n) for H in cases.HS for n in (1, 3, 25)]


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_", "GBRS_TUNING_SAMPLE_", "GBRS_TUNING_DIAG_")):
            monkeypatch.delenv(k, raising=False)


def run_samples(H, style, samples):
    """A handle on the problem's tables with the given samples run."""
    from gbrs_amd.hmm import DiplotypeHMM
    p0 = grid_cases.problem(H, style)
    hmm = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    av, ha = grid_cases.specificity(p0)
    rows = [grid_cases.expression_rows(grid_cases.sample_problem(H, style, s)) for s in samples]
    hmm.set_expression([np.stack([r[ci] for r in rows]) for ci in range(len(p0.chroms))], av, ha, 1.5, 0.12)
    hmm.run()
    return hmm, p0


def checked_samples(n):
    """The samples compared with the restatement: all of a small batch, the first, the middle and the last of a large one."""
    return sorted({0, n // 2, n - 1})


def relative(got, want):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(got == want, 0.0, d), initial=0.0))


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_base_reduction(H, n, style):
    hmm, p0 = run_samples(H, style, range(n))
    got = hmm.loglik()
    assert got.shape == (n, len(p0.chroms)) and got.dtype == np.float64
    assert hmm.loglik_info()[0] > 0
    worst = 0.0
    for s in checked_samples(n):
        want = restate.per_chromosome(H, style, s)
        np.testing.assert_allclose(got[s], want, rtol=RTOL, atol=0, err_msg=f"sample {s}")
        worst = max(worst, relative(got[s], want))
    for s in range(n):
        for ci, c in enumerate(p0.chroms):
            scaler = hmm.get(ci, sample=s, want=("scaler",))["scaler"]
            bound = len(scaler) * 2.0 ** -53 * np.abs(scaler).sum()
            assert abs(got[s, ci] - -scaler.sum()) <= bound, (s, c, got[s, ci], -scaler.sum(), bound)
    assert got.tobytes() == hmm.loglik().tobytes()                       # bit-identical between two calls
    for s in checked_samples(n):
        one = hmm.loglik(sample=s)
        assert one.shape == (1, len(p0.chroms)) and one.tobytes() == got[s].tobytes()
    hmm.close()
    print(f"DEVIATION loglik against the restatement H={H} n={n} {style}: worst relative difference {worst:.2e} (rtol {RTOL:g})")


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H", (3, 8, 16))
def test_a_sample_alone_and_in_a_batch_of_three(H, style):
    """The sum's shape depends on the chromosome alone: sample 1 run alone and as the middle slot of three, the same bits."""
    alone, _ = run_samples(H, style, [1])
    a = alone.loglik()
    alone.close()
    three, _ = run_samples(H, style, range(3))
    b = three.loglik()
    three.close()
    assert a[0].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_alternative_tables(H, n, style):
    """Five candidates in one launch per chromosome (every chromosome length; n_trans = n_c and n_c - 1; -inf entries)
    against the restatement; one and two candidates give the rows of the five bit for bit; the base's tables as a
    candidate agree with the reduction; the run's results are untouched."""
    names = ("base",) + cases.CANDIDATES
    hmm, p0 = run_samples(H, style, range(n))
    before = {ci: hmm.get(ci, sample=n - 1, want=("gamma", "calls")) for ci in range(len(p0.chroms))}
    base = hmm.loglik()
    got = np.empty((len(names), n, len(p0.chroms)))
    for ci, c in enumerate(p0.chroms):
        tabs = [cases.candidate(H, style, name)[ci] for name in names]
        assert len(tabs[4]) == len(p0.gene_ids[c]) - 1 and len(tabs[1]) == len(p0.gene_ids[c])
        got[:, :, ci] = hmm.loglik_tables(ci, tabs)
        assert hmm.loglik_info()[0] > 0
        assert hmm.loglik_tables(c, tabs[1:2]).tobytes() == got[1:2, :, ci].tobytes()                       # K = 1, by name
        assert hmm.loglik_tables(ci, [tabs[4], tabs[0]]).tobytes() == got[[4, 0], :, ci].tobytes()          # K = 2
        one = hmm.loglik_tables(ci, tabs, sample=n - 1)
        assert one.shape == (len(names), 1) and one[:, 0].tobytes() == got[:, n - 1, ci].tobytes()
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got[0], base, rtol=RTOL, atol=0)
    worst = 0.0
    for s in checked_samples(n):
        for k, name in enumerate(names):
            want = restate.per_chromosome(H, style, s, name)
            np.testing.assert_allclose(got[k, s], want, rtol=RTOL, atol=0, err_msg=f"{name} sample {s}")
            worst = max(worst, relative(got[k, s], want))
    for ci, res in before.items():
        after = hmm.get(ci, sample=n - 1, want=("gamma", "calls"))
        assert after["gamma"].tobytes() == res["gamma"].tobytes() and after["calls"].tobytes() == res["calls"].tobytes()
    assert base.tobytes() == hmm.loglik().tobytes()
    ms, nbytes = hmm.loglik_info()
    S, longest = hmm.S, max(grid_cases.LENS) - 1
    assert 16 * len(names) * longest * S * S <= nbytes <= 16 * len(names) * longest * S * S + 8 * len(names) * n + 8 * n * 5
    hmm.close()
    print(f"DEVIATION loglik_tables against the restatement H={H} n={n} {style}: worst relative difference {worst:.2e} "
          f"(rtol {RTOL:g})")


@pytest.mark.parametrize("H", (3, 8, 16))
def test_a_normaliser_that_is_not_finite_gives_minus_infinity(H):
    """+inf in a table makes a Z_i infinite: that pair's result is -inf, not NaN, and its neighbour's is untouched."""
    hmm, p0 = run_samples(H, "benign", range(3))
    good = cases.candidate(H, "benign", "base")[3]
    bad = good.copy()
    bad[40, 0, :] = np.inf
    got = hmm.loglik_tables(3, [good, bad, good])
    assert (got[1] == -np.inf).all() and np.isfinite(got[0]).all() and got[0].tobytes() == got[2].tobytes()
    np.testing.assert_allclose(got[0], hmm.loglik()[:, 3], rtol=RTOL, atol=0)
    hmm.close()


def test_raw_call_errors_leave_the_outputs_untouched():
    """Refusals that return before any launch: no run (GBRS_ERR_STATE); a sample or chromosome out of range, no table,
    too few blocks, NULL arguments (GBRS_ERR_INVALID).  Good calls after them succeed."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.hmm import DiplotypeHMM
    lib = _lib.load()
    H = 3
    p0 = grid_cases.problem(H, "benign")
    tabs = list(cases.candidate(H, "benign", "other"))
    out = np.full((2, 5), -7.0)
    out_t = np.full(4, -7.0)                         # [2 tables][2 samples]

    def tables(h, chrom, sample, k=2, n_trans=None, tprob=tabs, loglik=out_t):
        c = chrom if 0 <= chrom < 5 else 0
        count = max(k, 1)
        nt = None if n_trans == "null" else np.asarray([len(tabs[c])] * count if n_trans is None else n_trans, dtype=np.int32)
        use = None if tprob is None else _lib.ptr_table([tprob[c]] * count)
        return lib.gbrs_hmm_loglik_tables(h, chrom, k, _lib.ptr(nt), use, sample, _lib.ptr(loglik))

    def untouched():
        return (out == -7).all() and (out_t == -7).all()

    fresh = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    assert lib.gbrs_hmm_loglik(fresh._h, -1, _lib.ptr(out)) == _lib.GBRS_ERR_STATE and untouched()
    assert tables(fresh._h, 4, -1) == _lib.GBRS_ERR_STATE and untouched()
    for call in (fresh.loglik, lambda: fresh.loglik_tables(4, tabs[4:])):
        with pytest.raises(_lib.GbrsHipError) as e:
            call()
        assert e.value.status == _lib.GBRS_ERR_STATE
    assert fresh.loglik_info() == (0.0, 0)
    fresh.close()
    hmm, _ = run_samples(H, "benign", range(2))
    for sample in (2, -2, 25):
        assert lib.gbrs_hmm_loglik(hmm._h, sample, _lib.ptr(out)) == _lib.GBRS_ERR_INVALID and untouched()
        assert tables(hmm._h, 4, sample) == _lib.GBRS_ERR_INVALID and untouched()
    assert lib.gbrs_hmm_loglik(hmm._h, -1, None) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_hmm_loglik(None, -1, _lib.ptr(out)) == _lib.GBRS_ERR_INVALID and tables(None, 4, -1) == _lib.GBRS_ERR_INVALID
    for chrom in (5, -1):
        assert tables(hmm._h, chrom, -1) == _lib.GBRS_ERR_INVALID and untouched()
    for k in (0, -3):
        assert tables(hmm._h, 4, -1, k=k) == _lib.GBRS_ERR_INVALID and untouched()
    assert tables(hmm._h, 4, -1, n_trans=[200, 198]) == _lib.GBRS_ERR_INVALID and untouched()      # 200 genes need 199 blocks
    assert tables(hmm._h, 4, -1, n_trans="null") == _lib.GBRS_ERR_INVALID and untouched()
    assert tables(hmm._h, 4, -1, tprob=None) == _lib.GBRS_ERR_INVALID and untouched()
    assert tables(hmm._h, 4, -1, loglik=None) == _lib.GBRS_ERR_INVALID and untouched()
    null_table = (C.c_void_p * 2)(tabs[4].ctypes.data, None)
    nt = np.asarray([200, 200], dtype=np.int32)
    assert lib.gbrs_hmm_loglik_tables(hmm._h, 4, 2, _lib.ptr(nt), null_table, -1, _lib.ptr(out_t)) == _lib.GBRS_ERR_INVALID
    assert untouched() and hmm.loglik_info() == (0.0, 0)                                             # nothing ran
    with pytest.raises(_lib.GbrsHipError) as e:
        hmm.loglik_tables(5, tabs[4:])
    assert e.value.status == _lib.GBRS_ERR_INVALID
    with pytest.raises(ValueError, match="expected"):
        hmm.loglik_tables(4, [np.zeros((200, 3, 3))])
    # good calls after the refusals
    assert lib.gbrs_hmm_loglik(hmm._h, 1, _lib.ptr(out)) == _lib.GBRS_OK and (out[0] != -7).all() and (out[1] == -7).all()
    assert out[0].tobytes() == hmm.loglik()[1].tobytes()
    assert tables(hmm._h, 4, 0, n_trans=[199, 200]) == _lib.GBRS_OK and (out_t[:2] != -7).all() and (out_t[2:] == -7).all()
    assert out_t[0] == out_t[1] == hmm.loglik_tables(4, tabs[4:], sample=0)[0, 0]           # one sample: [2 tables][1]
    # a chromosome of one gene reads no table: none needs to be there
    none = (C.c_void_p * 1)(None)
    zero = np.zeros(1, dtype=np.int32)
    one = np.full((1, 2), -7.0)
    assert lib.gbrs_hmm_loglik_tables(hmm._h, 0, 1, _lib.ptr(zero), none, -1, _lib.ptr(one)) == _lib.GBRS_OK
    np.testing.assert_allclose(one[0], hmm.loglik()[:, 0], rtol=RTOL, atol=0)
    hmm.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

EXISTING = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz")
GRID = ("interpolated.genoprobs.tsv", "interpolated.genoprobs.npz")
SIM = ("sim_geno.npz", "sim_geno.crossovers.tsv")
DIAG = ("diagnostics.npz", "diagnostics.tsv")


def write_inputs(tmp_path, monkeypatch, H, style, alts):
    """$GBRS_DATA of the problem, a grid file, and one table file per alternative.  Returns the paths."""
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, grid_cases.problem(H, style), grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    for name in alts:
        paths[name] = cases.write_candidate(tmp_path / f"{name}.npz", H, style, name)
    return paths


def sample_tpm(tmp_path, H, style, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H, style, sample))


def same_bytes(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return fa.read() == fb.read()


def assert_loglik_file(stem, H, style, sample, names, files, selected):
    """<stem>.loglik.tsv against the restatement of the sample under the candidates `names` (table files `files`)."""
    lines = open(f"{stem}.loglik.tsv").read().splitlines()
    assert lines[0] == "chromosome\tgenes\t" + "\t".join(files)
    assert len(lines) == 3 + len(grid_cases.CHROMS) and lines[-1] == f"# selected: {files[selected]}"
    want = np.array([restate.per_chromosome(H, style, sample, name) for name in names])
    for ci, (c, genes) in enumerate(zip(grid_cases.CHROMS, grid_cases.LENS)):
        fields = lines[1 + ci].split("\t")
        assert fields[:2] == [c, str(genes)] and len(fields) == 2 + len(names)
        np.testing.assert_allclose([float(x) for x in fields[2:]], want[:, ci], rtol=RTOL, atol=0)
        assert all(repr(float(x)) == x for x in fields[2:])
    fields = lines[-2].split("\t")
    assert fields[:2] == ["total", str(sum(grid_cases.LENS))]
    np.testing.assert_allclose([float(x) for x in fields[2:]], restate.totals(H, style, [sample], names)[:, 0], rtol=RTOL, atol=0)
    return np.array([float(x) for x in fields[2:]])


def test_reconstruct_chooses_the_better_table_file(tmp_path, monkeypatch):
    """`-e` with two alternatives: the selected file is choose_tables of the restatement, and every file of the sample -
    with the grid, path draws and diagnostics too - is the one a plain run under the selected file writes."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import choose_tables
    H, style, alts = cases.SINGLE_H, cases.SINGLE_STYLE, cases.SINGLE_ALTS
    names = ("base",) + alts
    paths = write_inputs(tmp_path, monkeypatch, H, style, alts)
    files = [paths["tprob"]] + [paths[a] for a in alts]
    selected = int(choose_tables(restate.totals(H, style, [0], names))[0][0])
    assert selected == 1
    tpm = sample_tpm(tmp_path, H, style, 0)
    common = ["reconstruct", "-e", tpm, "-x", paths["avecs"], "-g", paths["gpos"]]
    alt_args = [x for a in alts for x in ("--alt-tprob-file", paths[a])]
    more = ["--grid-file", paths["grid"], "--grid-genoprobs", "--sim-geno", "8", "--diagnostics"]
    assert cli.main(common + ["-t", files[selected], "-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-t", files[0], "-o", str(tmp_path / "chosen")] + alt_args) == 0
    assert cli.main(common + more + ["-t", files[selected], "-o", str(tmp_path / "gplain")]) == 0
    assert cli.main(common + more + ["-t", files[0], "-o", str(tmp_path / "gchosen")] + alt_args) == 0
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"chosen.{suffix}"), suffix
    for suffix in EXISTING + GRID + SIM + DIAG:
        assert same_bytes(tmp_path / f"gplain.{suffix}", tmp_path / f"gchosen.{suffix}"), suffix
    assert not os.path.exists(tmp_path / "plain.loglik.tsv") and not os.path.exists(tmp_path / "gplain.loglik.tsv")
    assert_loglik_file(str(tmp_path / "chosen"), H, style, 0, names, files, selected)
    assert same_bytes(tmp_path / "chosen.loglik.tsv", tmp_path / "gchosen.loglik.tsv")


def test_loglik_alone_and_a_run_without_the_options(tmp_path, monkeypatch):
    """--loglik: one candidate column, the other files those of a plain run.  Without the options: no likelihood file, no
    device pass, no buffer - loglik_info() of the run's handle says so."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import ReconstructContext, reconstruct
    H, style = cases.COMMAND_H, cases.COMMAND_STYLE
    paths = write_inputs(tmp_path, monkeypatch, H, style, ())
    tpm = sample_tpm(tmp_path, H, style, 2)
    common = ["reconstruct", "-e", tpm, "-t", paths["tprob"], "-x", paths["avecs"], "-g", paths["gpos"]]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "scored"), "--loglik"]) == 0
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"scored.{suffix}"), suffix
    assert not os.path.exists(tmp_path / "plain.loglik.tsv")
    assert_loglik_file(str(tmp_path / "scored"), H, style, 2, ("base",), [paths["tprob"]], 0)
    ctx = ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"])
    stages = {}
    reconstruct(tpm, paths["tprob"], outbase=str(tmp_path / "held"), context=ctx, stage_times=stages)
    assert ctx.loglik_launches == 0 and ctx.hmm.loglik_info() == (0.0, 0) and "loglik" not in stages
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"held.{suffix}"), suffix
    assert not os.path.exists(tmp_path / "held.loglik.tsv")
    reconstruct(tpm, paths["tprob"], outbase=str(tmp_path / "held"), context=ctx, stage_times=stages, loglik=True)
    assert ctx.loglik_launches == 1 and ctx.hmm.loglik_info()[0] > 0 and stages["loglik"] > 0
    assert same_bytes(tmp_path / "scored.loglik.tsv", tmp_path / "held.loglik.tsv")
    ctx.close()


def test_an_exact_tie_keeps_the_first_listed_file(tmp_path, monkeypatch):
    """One founder: every table is log(1), every total ties exactly, and -t - the first candidate - is kept."""
    from gbrs_amd import cli
    H, alts = cases.TIE_H, ("other", "x_only")
    paths = write_inputs(tmp_path, monkeypatch, H, "do", alts)
    files = [paths["tprob"]] + [paths[a] for a in alts]
    tpm = sample_tpm(tmp_path, H, "do", 0)
    common = ["reconstruct", "-e", tpm, "-t", paths["tprob"], "-x", paths["avecs"], "-g", paths["gpos"]]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "tied"), "--alt-tprob-file", paths["other"], "--alt-tprob-file",
                              paths["x_only"]]) == 0
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"tied.{suffix}"), suffix
    totals = assert_loglik_file(str(tmp_path / "tied"), H, "do", 0, ("base",) + alts, files, 0)
    assert (totals == totals[0]).all()


@pytest.mark.parametrize("batch", (2, 64))
def test_sample_file_with_alternatives(tmp_path, monkeypatch, batch):
    """Five samples in launches of 2 and in one of 5: each sample's selected file is choose_tables of the restatement.  A
    sample that stayed has the files of a plain cohort run under -t with the same launches.  A sample that moved ran in a
    launch of its own under the selected file: its files are those of a plain cohort run under that file in launches of
    one (the same stream for the path draws), which but for the draws' stream is the single-sample command.  Every sample
    has its loglik.tsv and its line in the model report."""
    from gbrs_amd import cli
    from gbrs_amd.hmm import choose_tables
    H, style, alts, n = cases.COMMAND_H, cases.COMMAND_STYLE, cases.COMMAND_ALTS, cases.COMMAND_SAMPLES
    names = ("base",) + alts
    paths = write_inputs(tmp_path, monkeypatch, H, style, alts)
    files = [paths["tprob"]] + [paths[a] for a in alts]
    want_totals = restate.totals(H, style, range(n), names)
    best, margin = choose_tables(want_totals)
    assert (best == 0).any() and (best != 0).any()
    tpms = [sample_tpm(tmp_path, H, style, s) for s in range(n)]
    for run in ["many"] + [f"plain{k}_" for k in sorted(set(best.tolist()))]:
        with open(tmp_path / f"{run}.txt", "w") as fh:
            for s in range(n):
                fh.write(f"{tpms[s]}\t{tmp_path / f'{run}{s}'}\n")
    common = ["-x", paths["avecs"], "-g", paths["gpos"], "--grid-file", paths["grid"], "--sim-geno", "4", "--diagnostics"]
    for k in sorted(set(best.tolist())):
        assert cli.main(["reconstruct", "--sample-file", str(tmp_path / f"plain{k}_.txt"), "-t", files[k], "--batch-size",
                         str(batch if k == 0 else 1)] + common) == 0
    report = tmp_path / "models.tsv"
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "many.txt"), "-t", files[0], "--model-report", str(report),
                     "--batch-size", str(batch)] + [x for a in alts for x in ("--alt-tprob-file", paths[a])] + common) == 0
    lines = open(report).read().splitlines()
    assert lines[0] == "#outbase\tselected\tmargin\t" + "\t".join(files) and len(lines) == 1 + n
    for s in range(n):
        k = int(best[s])
        for suffix in EXISTING + GRID[:1] + SIM + DIAG:
            assert same_bytes(tmp_path / f"plain{k}_{s}.{suffix}", tmp_path / f"many{s}.{suffix}"), (s, suffix)
        assert not os.path.exists(tmp_path / f"plain{k}_{s}.loglik.tsv")
        totals = assert_loglik_file(str(tmp_path / f"many{s}"), H, style, s, names, files, k)
        fields = lines[1 + s].split("\t")
        assert fields[:2] == [str(tmp_path / f"many{s}"), files[k]]
        assert [float(x) for x in fields[3:]] == totals.tolist()
        assert abs(float(fields[2]) - margin[s]) <= 2 * RTOL * np.abs(want_totals[:, s]).max()      # a difference of two totals
    moved = int(np.flatnonzero(best)[-1])                               # the single-sample command under the selected file
    assert cli.main(["reconstruct", "-e", tpms[moved], "-t", files[best[moved]], "-o", str(tmp_path / "single")] + common) == 0
    for suffix in EXISTING + GRID[:1] + DIAG:
        assert same_bytes(tmp_path / f"single.{suffix}", tmp_path / f"many{moved}.{suffix}"), suffix
    print(f"selected {best.tolist()}, margins {np.round(margin, 3).tolist()}")


def test_only_the_chromosomes_that_differ_are_launched(tmp_path, monkeypatch):
    """An alternative that differs on "X" alone takes one reduction and one chain launch per device launch, and the buffers
    hold X's blocks; one that differs everywhere takes one chain launch per chromosome.  The model report is written even
    when every sample stays with -t."""
    from gbrs_amd.hmm import ReconstructContext, reconstruct_many
    H, style, n = cases.COMMAND_H, cases.COMMAND_STYLE, 3
    paths = write_inputs(tmp_path, monkeypatch, H, style, ("x_only", "other", "base"))
    tpms = [sample_tpm(tmp_path, H, style, s) for s in range(n)]
    S = H * (H + 1) // 2

    def run(tag, alts, batch):
        ctx = ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"], alt_tprob_files=[paths[a] for a in alts])
        stages = {}
        done = reconstruct_many(tpms, [str(tmp_path / f"{tag}{s}") for s in range(n)], paths["tprob"], batch_size=batch,
                                context=ctx, stage_times=stages, model_report=str(tmp_path / f"{tag}.tsv"))
        assert not any("error" in d for d in done) and stages["loglik"] > 0
        ms, nbytes = ctx.hmm.loglik_info()
        launches = ctx.loglik_launches
        ctx.close()
        return launches, ms, nbytes

    launches, ms, nbytes = run("x", ["x_only"], 64)
    assert launches == 2 and ms > 0
    assert 16 * 199 * S * S <= nbytes <= 16 * 199 * S * S + 8 * 5 * n
    launches, _, _ = run("x2", ["x_only"], 2)
    assert launches == 4                                                  # two device launches
    launches, _, nbytes = run("o", ["other", "x_only"], 64)
    assert launches == 1 + 5 and 2 * 16 * 199 * S * S <= nbytes <= 2 * 16 * 199 * S * S + 8 * 5 * n
    # a copy of the base under another name: every chromosome equal, no chain launch, every sample stays, the report is there
    launches, _, nbytes = run("b", ["base"], 64)
    assert launches == 1 and nbytes == 8 * 5 * n
    lines = open(tmp_path / "b.tsv").read().splitlines()
    assert len(lines) == 1 + n and all(ln.split("\t")[1] == paths["tprob"] and float(ln.split("\t")[2]) == 0.0 for ln in lines[1:])
