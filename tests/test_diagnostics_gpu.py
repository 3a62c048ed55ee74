"""The diagnostics on the device (gbrs_hmm_diagnostics, gbrs_hmm_pair_posterior, `gbrs reconstruct --diagnostics`;
DESIGN.md §23; needs an MI355X).  The definition: tests/diagnostics_restate.py; its agreement with the posteriors, a
leave-one-out rerun and drawn paths: tests/test_diagnostics_cpu.py.

The device's numbers are compared with the restatement fed with the device's OWN alpha, beta, eprob and gamma
(hmm.get), so the posteriors' 1e-8 plays no part.  Tolerances: xo, pswitch and xi are sums of non-negative terms whose
exponents carry about 1e-12 of absolute rounding, rtol 1e-9 and atol 1e-15; errlod is a difference of log-sums of
magnitude up to ~1500, rtol 1e-9 and atol 1e-9; maxprob and maxmarg are equal."""
import functools
import os

import numpy as np
import pytest

import diagnostics_cases as cases
import diagnostics_restate as restate
import grid_cases

pytestmark = pytest.mark.gpu

STYLES = ("benign", "do")
# founders x samples: 1, 3 and 25 samples take the three HMM routes whose buffers hmm_make_logs reads; 1 .. 8 founders keep
# the transition block in LDS, 16 read it through L2; 25 samples are two slabs of the pair pass
TABLE = [(H, n) for H in (1, 3, 8, 16) for n in (1, 3, 25)]
NAMES = ("xo", "pswitch", "errlod", "maxprob", "maxmarg")


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_", "GBRS_TUNING_SAMPLE_", "GBRS_TUNING_DIAG_")):
            monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def short_tables(H, style):
    """The table's problem with n - 1 transition blocks per chromosome."""
    from gbrs_amd import synth
    with np.errstate(divide="ignore"):
        return synth.make_hmm_problem(H=H, genes_per_chrom=list(grid_cases.LENS), chroms=list(grid_cases.CHROMS),
                                      seed=grid_cases.SEED + H, style=style, tprob_len_minus_one=True,
                                      expressed_fraction=0.4 if style == "do" else 0.5)


def run_samples(H, style, samples, p0=None):
    """A handle on the table's problem (or p0's tables) with the given samples run."""
    from gbrs_amd.hmm import DiplotypeHMM
    p0 = grid_cases.problem(H, style) if p0 is None else p0
    hmm = DiplotypeHMM(H, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    av, ha = grid_cases.specificity(p0)
    rows = [grid_cases.expression_rows(grid_cases.sample_problem(H, style, s)) for s in samples]
    hmm.set_expression([np.stack([r[ci] for r in rows]) for ci in range(len(p0.chroms))], av, ha, 1.5, 0.12)
    hmm.run()
    return hmm, p0


def assert_equals_the_restatement(hmm, p0, n, samples=None, with_xi=None):
    """Every output of every sample and chromosome; xi for the first, the middle and the last sample (the pass takes one
    sample at a time: the index only moves the rows it reads).  samples: the samples compared (default: all n);
    with_xi: those among them whose xi is compared (default: those three).  Returns the worst differences met."""
    got = hmm.diagnostics()
    ch, iv = restate.change_table(hmm.H), restate.init_vec(hmm.H)
    worst = dict(xo=0.0, pswitch=0.0, xi=0.0, errlod=0.0)
    with_xi = sorted({0, n // 2, n - 1}) if with_xi is None else list(with_xi)
    for ci, c in enumerate(p0.chroms):
        genes = len(p0.gene_ids[c])
        for k in NAMES:
            assert got[k][ci].shape == (n, genes - 1 if k in ("xo", "pswitch") else genes), (k, c)
        assert got["maxmarg"][ci].dtype == np.int32
        for s in (range(n) if samples is None else samples):
            at = f"sample {s} chromosome {c}"
            own = hmm.get(ci, sample=s, want=("alpha", "beta", "eprob", "gamma"))
            want = restate.all_of(own, p0.tprob[c], ch, iv)
            for k in ("xo", "pswitch"):
                np.testing.assert_allclose(got[k][ci][s], want[k], rtol=1e-9, atol=1e-15, err_msg=f"{k} {at}")
                if genes > 1:
                    worst[k] = max(worst[k], float(np.abs(got[k][ci][s] - want[k]).max()))
            np.testing.assert_allclose(got["errlod"][ci][s], want["errlod"], rtol=1e-9, atol=1e-9, err_msg=at)
            worst["errlod"] = max(worst["errlod"], float(np.abs(got["errlod"][ci][s] - want["errlod"]).max()))
            np.testing.assert_array_equal(got["maxprob"][ci][s], want["maxprob"], err_msg=at)
            np.testing.assert_array_equal(got["maxmarg"][ci][s], want["maxmarg"], err_msg=at)
            if s in with_xi:
                xi = hmm.pair_posterior(ci, sample=s)
                assert xi.shape == (genes - 1, hmm.S, hmm.S)
                np.testing.assert_allclose(xi, want["xi"], rtol=1e-9, atol=1e-15, err_msg=f"xi {at}")
                if genes > 1:
                    worst["xi"] = max(worst["xi"], float(np.abs(xi - want["xi"]).max()))
    return worst


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_outputs_equal_the_restatement(H, n, style):
    hmm, p0 = run_samples(H, style, range(n))
    worst = assert_equals_the_restatement(hmm, p0, n)
    assert hmm.diagnostics_info() > 0
    hmm.close()
    print(f"DEVIATION diagnostics against the restatement H={H} n={n} {style}: worst absolute differences "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", (8, 16))
def test_tables_one_shorter_than_the_genes(H, style):
    """n_trans = n - 1: only T[0 .. n-2] are read."""
    p0 = short_tables(H, style)
    assert all(len(p0.tprob[c]) == len(p0.gene_ids[c]) - 1 for c in p0.chroms)
    hmm, _ = run_samples(H, style, range(3), p0)
    assert_equals_the_restatement(hmm, p0, 3)
    hmm.close()


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", (3, 8, 16))
def test_pair_posteriors_sum_to_the_marginals(H, style):
    """Row and column sums of the device's xi against the device's gamma."""
    hmm, p0 = run_samples(H, style, range(2))
    worst = 0.0
    for ci, c in enumerate(p0.chroms):
        gamma = hmm.get(ci, sample=1, want=("gamma",))["gamma"]
        xi = hmm.pair_posterior(c, sample=1)                          # by name
        if gamma.shape[1] < 2:
            assert xi.shape == (0, hmm.S, hmm.S)
            continue
        for got, want in ((xi.sum(axis=2).T, gamma[:, :-1]), (xi.sum(axis=1).T, gamma[:, 1:])):
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
            np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-300)
    hmm.close()
    print(f"DEVIATION device pair marginals H={H} {style}: worst relative difference {worst:.2e} (rtol 1e-8)")


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", (3, 8, 16))
def test_expected_crossovers_are_those_of_the_draws(H, style):
    """sum xo per chromosome against the mean founder changes of K = 4096 paths drawn on the device: six standard errors of
    the mean, the variance floored at 4 / K (tests/test_sim_geno_cpu.py's floor)."""
    K = 4096
    hmm, p0 = run_samples(H, style, [0])
    xo = hmm.diagnostics(sample=0, want=("xo",))["xo"]
    drawn = hmm.sample_paths(K, seed=20240229, sample=0)
    assert drawn["degenerate"] == 0
    worst = 0.0
    for ci in range(len(p0.chroms)):
        counts = drawn["changes"][:, ci].astype(np.float64)
        worst = max(worst, abs(counts.mean() - xo[ci].sum()) / np.sqrt(max(counts.var(ddof=1), 4.0 / K) / K))
    hmm.close()
    print(f"DEVIATION expected crossovers against {K} device draws H={H} {style}: worst {worst:.2f} standard errors (bound 6)")
    assert worst <= 6.0


def flat(got):
    return {k: np.concatenate(v, axis=-1) for k, v in got.items()}


def assert_same_bits(a, b):
    a, b = flat(a), flat(b)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_selection_slabs_and_repeats_change_no_bit(monkeypatch):
    n = 25
    hmm, p0 = run_samples(8, "do", range(n))
    whole = hmm.diagnostics()
    assert_same_bits(hmm.diagnostics(), whole)                                  # two calls
    for s in (0, 7, 24):                                                        # one sample = its slice of all
        one = hmm.diagnostics(sample=s)
        assert one["xo"][3].shape == (64,) and one["maxmarg"][4].shape == (200,)
        assert_same_bits(one, {k: [a[s] for a in v] for k, v in whole.items()})
    for slab in ("1", "7", "64"):                                               # 25 slabs, 3 full + one of 4, one
        monkeypatch.setenv("GBRS_TUNING_DIAG_SLAB", slab)
        assert_same_bits(hmm.diagnostics(), whole)
    monkeypatch.delenv("GBRS_TUNING_DIAG_SLAB")
    part = hmm.diagnostics(want=("pswitch", "maxmarg"))                         # a subset is the same numbers
    assert sorted(part) == ["maxmarg", "pswitch"]
    assert_same_bits(part, {k: whole[k] for k in part})
    xi = hmm.pair_posterior(4, sample=9)
    assert xi.tobytes() == hmm.pair_posterior(4, sample=9).tobytes()
    with pytest.raises(ValueError, match="unknown diagnostics"):
        hmm.diagnostics(want=("xo", "lod"))
    hmm.close()


def test_last_gene_slots_and_a_one_gene_chromosome():
    """The raw call: [n][total_genes], the slot of every chromosome's last gene 0.0 in xo and pswitch - the one-gene
    chromosome "1" is such a slot and nothing else."""
    from gbrs_amd import _lib
    lib = _lib.load()
    hmm, p0 = run_samples(8, "benign", range(3))
    G = sum(grid_cases.LENS)
    xo, ps = np.full((3, G), -7.0), np.full((3, G), -7.0)
    lod, top, at = np.full((3, G), -7.0), np.full((3, G), -7.0), np.full((3, G), -7, dtype=np.int32)
    assert lib.gbrs_hmm_diagnostics(hmm._h, -1, _lib.ptr(xo), _lib.ptr(ps), _lib.ptr(lod), _lib.ptr(top), _lib.ptr(at)) == 0
    last = np.cumsum(grid_cases.LENS) - 1
    assert (xo[:, last] == 0.0).all() and (ps[:, last] == 0.0).all() and last[0] == 0
    inner = np.setdiff1d(np.arange(G), last)
    assert (xo[:, inner] > 0).all() and (ps[:, inner] > 0).all() and (xo >= 0).all()
    assert np.isfinite(lod).all() and (top > 0).all() and (top <= 1 + 1e-12).all() and (at >= 0).all() and (at < 36).all()
    got = hmm.diagnostics()
    assert got["xo"][0].shape == (3, 0) and got["errlod"][0].shape == (3, 1)
    np.testing.assert_array_equal(np.concatenate(got["errlod"], axis=1), lod)
    np.testing.assert_array_equal(got["xo"][4], xo[:, last[3] + 1:last[4]])
    assert hmm.pair_posterior(0).shape == (0, 36, 36)
    hmm.close()


def test_raw_call_errors_leave_the_outputs_untouched():
    """Refusals that return before any launch: no run (GBRS_ERR_STATE); a sample or chromosome out of range, xi == NULL
    (GBRS_ERR_INVALID).  A good call after them succeeds."""
    from gbrs_amd import _lib
    from gbrs_amd.hmm import DiplotypeHMM
    lib = _lib.load()
    p0 = grid_cases.problem(3, "benign")
    G = sum(grid_cases.LENS)
    out = [np.full((2, G), -7.0) for _ in range(4)] + [np.full((2, G), -7, dtype=np.int32)]
    xi = np.full((199, 6, 6), -7.0)

    def call(h, sample):
        return lib.gbrs_hmm_diagnostics(h, sample, *[_lib.ptr(a) for a in out])

    def untouched():
        return all((a == -7).all() for a in out) and (xi == -7).all()

    fresh = DiplotypeHMM(3, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    assert call(fresh._h, -1) == _lib.GBRS_ERR_STATE and untouched()
    assert lib.gbrs_hmm_pair_posterior(fresh._h, 0, 4, _lib.ptr(xi)) == _lib.GBRS_ERR_STATE and untouched()
    with pytest.raises(_lib.GbrsHipError) as e:
        fresh.diagnostics()
    assert e.value.status == _lib.GBRS_ERR_STATE
    with pytest.raises(_lib.GbrsHipError) as e:
        fresh.pair_posterior(4)
    assert e.value.status == _lib.GBRS_ERR_STATE
    fresh.close()
    hmm, _ = run_samples(3, "benign", range(2))
    for sample in (2, -2, 25):
        assert call(hmm._h, sample) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error() and untouched()
    for sample, chrom in ((2, 4), (-1, 4), (0, 5), (0, -1)):
        assert lib.gbrs_hmm_pair_posterior(hmm._h, sample, chrom, _lib.ptr(xi)) == _lib.GBRS_ERR_INVALID and untouched()
    assert lib.gbrs_hmm_pair_posterior(hmm._h, 0, 4, None) == _lib.GBRS_ERR_INVALID and untouched()
    assert call(None, -1) == _lib.GBRS_ERR_INVALID and lib.gbrs_hmm_pair_posterior(None, 0, 4, _lib.ptr(xi)) == _lib.GBRS_ERR_INVALID
    with pytest.raises(_lib.GbrsHipError) as e:
        hmm.pair_posterior(5)
    assert e.value.status == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_hmm_diagnostics(hmm._h, -1, None, None, None, None, None) == _lib.GBRS_OK and untouched()   # nothing asked
    assert hmm.diagnostics_info() == 0.0
    # good calls after the refusals
    assert call(hmm._h, 1) == _lib.GBRS_OK
    assert all((a[0] != -7).all() and (a[1] == -7).all() for a in out)           # one sample: the first row only
    assert lib.gbrs_hmm_pair_posterior(hmm._h, 1, 4, _lib.ptr(xi)) == _lib.GBRS_OK and (xi >= 0).all()
    np.testing.assert_allclose(xi.sum(axis=(1, 2)), 1.0, rtol=1e-12)
    want = hmm.diagnostics(sample=1)
    np.testing.assert_array_equal(np.concatenate(want["errlod"]), out[2][0])
    assert lib.gbrs_hmm_diagnostics(hmm._h, 0, None, None, None, None, _lib.ptr(out[4][1])) == _lib.GBRS_OK    # nullable outputs
    np.testing.assert_array_equal(out[4][1], np.concatenate(hmm.diagnostics(sample=0)["maxmarg"]))
    hmm.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES = 8, "benign"
EXISTING = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz")
GRID = ("interpolated.genoprobs.tsv", "interpolated.genoprobs.npz")
SIM = ("sim_geno.npz", "sim_geno.crossovers.tsv")
NEW = ("diagnostics.npz", "diagnostics.tsv")


def write_inputs(tmp_path, monkeypatch, p0):
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    return paths


@pytest.fixture
def tables(tmp_path, monkeypatch):
    return write_inputs(tmp_path, monkeypatch, grid_cases.problem(H_FILES, STYLE_FILES))


def sample_tpm(tmp_path, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, sample))


def same_bytes(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return fa.read() == fb.read()


def assert_diagnostics_files(stem, hmm, slot, sample, threshold):
    """The two files of a sample against diagnostics() on a handle that ran the same samples.  Returns (errlod, expressed)
    over the handle's genes."""
    from gbrs_amd.hmm import change_table, viterbi_changes
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    p = grid_cases.sample_problem(H_FILES, STYLE_FILES, sample)
    want = hmm.diagnostics(sample=slot)
    z = np.load(f"{stem}.diagnostics.npz")
    assert sorted(z.files) == sorted([f"{k}_{c}" for k in NAMES + ("expressed",) for c in p0.chroms] + ["diplotypes"])
    assert list(z["diplotypes"]) == [a + b for ai, a in enumerate(p0.hap_names) for b in p0.hap_names[ai:]]
    lines = open(f"{stem}.diagnostics.tsv").read().splitlines()
    assert lines[0] == "#Chromosome\tGenes\tExpressed\tViterbi\tExpectedCrossovers\tFlagged\tMaxErrorLOD\tMeanMaxProb"
    assert len(lines) == 2 + len(p0.chroms)
    table = change_table(H_FILES)
    totals = dict(genes=0, on=0, viterbi=0, flagged=0)
    for ci, c in enumerate(p0.chroms):
        for k in NAMES:
            assert z[f"{k}_{c}"].dtype == want[k][ci].dtype
            np.testing.assert_array_equal(z[f"{k}_{c}"], want[k][ci], err_msg=f"{k} {c}")
        on = restate.expressed([p.expr[g] for g in p.gene_ids[c]], 1.5)
        assert z[f"expressed_{c}"].dtype == bool
        np.testing.assert_array_equal(z[f"expressed_{c}"], on)
        lod = want["errlod"][ci]
        viterbi = viterbi_changes(hmm.get(ci, sample=slot, want=("calls",))["calls"], table)
        assert lines[1 + ci] == "%s\t%d\t%d\t%d\t%.6f\t%d\t%.6f\t%.6f" % (
            c, len(lod), on.sum(), viterbi, want["xo"][ci].sum(), (lod[on] > threshold).sum(),
            lod[on].max() if on.any() else np.nan, want["maxprob"][ci].mean())
        for k, v in (("genes", len(lod)), ("on", int(on.sum())), ("viterbi", viterbi), ("flagged", int((lod[on] > threshold).sum()))):
            totals[k] += v
    fields = lines[-1].split("\t")
    assert fields[0] == "total" and [int(fields[k]) for k in (1, 2, 3, 5)] == [totals[k] for k in ("genes", "on", "viterbi", "flagged")]
    assert abs(float(fields[4]) - sum(x.sum() for x in want["xo"])) < 1e-6
    return np.concatenate(want["errlod"]), np.concatenate([z[f"expressed_{c}"] for c in p0.chroms])


def test_reconstruct_with_diagnostics(tmp_path, tables):
    """`-e`: the files of a plain run, and with --grid-file and --sim-geno the seven, are byte-identical with and without the
    option; a run without it writes no diagnostics file."""
    from gbrs_amd import cli
    tpm = sample_tpm(tmp_path, 0)
    common = ["reconstruct", "-e", tpm, "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"]]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "diag"), "--diagnostics", "--error-lod-threshold", "0.5"]) == 0
    more = ["--grid-file", tables["grid"], "--grid-genoprobs", "--sim-geno", "8"]
    assert cli.main(common + more + ["-o", str(tmp_path / "gplain")]) == 0
    assert cli.main(common + more + ["-o", str(tmp_path / "gdiag"), "--diagnostics"]) == 0
    for suffix in NEW:
        assert not os.path.exists(tmp_path / f"plain.{suffix}") and not os.path.exists(tmp_path / f"gplain.{suffix}")
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"diag.{suffix}"), suffix
    for suffix in EXISTING + GRID + SIM:
        assert same_bytes(tmp_path / f"gplain.{suffix}", tmp_path / f"gdiag.{suffix}"), suffix
    hmm, _ = run_samples(H_FILES, STYLE_FILES, [0])
    assert_diagnostics_files(str(tmp_path / "diag"), hmm, 0, 0, 0.5)
    assert_diagnostics_files(str(tmp_path / "gdiag"), hmm, 0, 0, 2.0)
    hmm.close()


@pytest.mark.parametrize("batch", (2, 64))
def test_sample_file_with_diagnostics(tmp_path, tables, batch):
    """Five samples in launches of 2 and in one of 5: every sample's files, the existing ones byte-identical, and the gene
    report against the per-sample arrays."""
    from gbrs_amd import cli
    n, threshold = 5, 0.25
    with open(tmp_path / "samples.txt", "w") as fh:
        fh.write("# cohort\n")
        for s in range(n):
            fh.write(f"{sample_tpm(tmp_path, s)}\t{tmp_path / f'many{s}'}\n\n")
    with open(tmp_path / "samples.txt") as src, open(tmp_path / "plain.txt", "w") as dst:
        dst.write(src.read().replace("many", "plain"))
    common = ["--batch-size", str(batch), "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"],
              "--grid-file", tables["grid"], "--sim-geno", "4"]
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "plain.txt")] + common) == 0
    report = tmp_path / "genes.tsv"
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "--diagnostics", "--error-lod-threshold",
                     str(threshold), "--gene-report", str(report)] + common) == 0
    for s in range(n):
        for suffix in NEW:
            assert not os.path.exists(tmp_path / f"plain{s}.{suffix}")
        for suffix in EXISTING + GRID[:1] + SIM:
            assert same_bytes(tmp_path / f"plain{s}.{suffix}", tmp_path / f"many{s}.{suffix}"), (s, suffix)
    lods, ons = [], []
    for lo in range(0, n, batch):                    # the launches the command made
        members = list(range(lo, min(lo + batch, n)))
        hmm, _ = run_samples(H_FILES, STYLE_FILES, members)
        for slot, s in enumerate(members):
            lod, on = assert_diagnostics_files(str(tmp_path / f"many{s}"), hmm, slot, s, threshold)
            lods.append(lod)
            ons.append(on)
        hmm.close()
    lods, ons = np.array(lods), np.array(ons)
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    ids = [(g, c) for c in p0.chroms for g in p0.gene_ids[c]]
    lines = open(report).read().splitlines()
    assert lines[0] == "#Gene_ID\tChromosome\tSamples\tExpressed\tFlagged\tMeanErrorLOD\tMaxErrorLOD" and len(lines) == 1 + len(ids)
    assert ons.any(axis=0).sum() > 100
    for k, (g, c) in enumerate(ids):
        on = ons[:, k]
        mean = lods[on, k].sum() / on.sum() if on.any() else np.nan
        assert lines[1 + k] == "%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f" % (
            g, c, n, on.sum(), (on & (lods[:, k] > threshold)).sum(), mean, lods[on, k].max() if on.any() else np.nan), g


@pytest.mark.parametrize("H,style", cases.PLANT_TABLE)
def test_planted_gene_through_the_command(tmp_path, monkeypatch, H, style):
    """Gene 30 of chromosome "4" contradicts its neighbours: in the command's .npz it is the chromosome's unique error LOD
    maximum, more than 0.5 above the runner-up; the unexpressed gene 10 is not expressed and so counted nowhere."""
    from gbrs_amd import cli
    p = cases.planted(H, style)
    paths = write_inputs(tmp_path, monkeypatch, p)
    tpm = grid_cases.write_genes_tpm(tmp_path / "planted.genes.tpm", p)
    stem = str(tmp_path / "planted")
    assert cli.main(["reconstruct", "-e", tpm, "-t", paths["tprob"], "-x", paths["avecs"], "-g", paths["gpos"], "-o", stem,
                     "--diagnostics"]) == 0
    z = np.load(stem + ".diagnostics.npz")
    errlod, on = z[f"errlod_{cases.PLANT_CHROM}"], z[f"expressed_{cases.PLANT_CHROM}"]
    gap, silent_expressed = cases.gap_of_the_planted_gene(errlod, on)
    print(f"DEVIATION planted gene on the device H={H} {style}: gap {gap:.3g} (bound 0.5)")
    assert int(errlod.argmax()) == cases.PLANT_GENE and gap > 0.5
    assert not silent_expressed and on.sum() == len(on) - 1
    row = [ln.split("\t") for ln in open(stem + ".diagnostics.tsv").read().splitlines() if ln.startswith(cases.PLANT_CHROM + "\t")][0]
    assert int(row[2]) == 64 and int(row[5]) == int((errlod[on] > 2.0).sum()) and abs(float(row[6]) - errlod[cases.PLANT_GENE]) < 1e-6
