"""Diplotype paths drawn on the device (gbrs_hmm_sample_paths, `gbrs reconstruct --sim-geno`; needs an
MI355X).  The definition: tests/sim_geno_restate.py; its agreement with the posterior: tests/test_sim_geno_cpu.py.

The paths are compared element for element with the restatement fed with the device's OWN alpha (hmm.get(...,
want=('alpha',))), so the posteriors' 1e-8 plays no part.  The device forms a weight as exp(alpha) * exp(T) where the
restatement takes exp(alpha + T), a relative difference of a few 2^-53 per weight and of S times that in a cumulative sum;
a decision whose threshold is within 1e-12 of a cumulative sum (relative to the total) may therefore come out otherwise,
and that draw is left out from there downwards.  None may be left out at the seeds used here: the restatement reports the
smallest margin, and the tests assert it is above the floor (smallest met on an MI355X over the table below: 2.2e-10 at
16 founders, 25 samples, benign tables; every other case above 1e-8)."""
import functools
import os

import numpy as np
import pytest

import grid_cases
import sim_geno_restate as restate

pytestmark = pytest.mark.gpu

STYLES = ("benign", "do")
# founders x samples: 1, 3 and 25 samples take the three HMM routes whose buffers hmm_make_logs reads; 1 .. 8 founders keep
# the transition block in LDS, 16 read it through L2
TABLE = [(H, n) for H in (1, 3, 8, 16) for n in (1, 3, 25)]
DRAWS = (1, 64, 65, 300)        # a lone lane, a full wave, one lane into a second, more than one 256-draw block
SEED = 0x5EED00000000 + 77      # both key words in use
FLOOR = 1e-12


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_", "GBRS_TUNING_SAMPLE_")):
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


def assert_equals_the_restatement(hmm, p0, n, seed, streams=None, samples=None, draws=DRAWS):
    """Every count of `draws` against the restatement of max(draws) draws (a draw is keyed by its number, so fewer draws
    are a prefix), for the given samples of the launch (default: all n).  Returns the smallest margin met."""
    K = max(draws)
    table = restate.change_table(hmm.H)
    got = {k: hmm.sample_paths(k, seed=seed, streams=streams) for k in draws}
    smallest = np.inf
    for k in draws:
        assert got[k]["degenerate"] == 0
        assert got[k]["changes"].shape == (n, k, len(p0.chroms)) and got[k]["changes"].dtype == np.int32
    for s in (range(n) if samples is None else samples):
        stream = s if streams is None else streams[s]
        for ci, c in enumerate(p0.chroms):
            alpha = hmm.get(ci, sample=s, want=("alpha",))["alpha"]
            paths, changes, margins, degenerate = restate.sample_paths(alpha, p0.tprob[c], seed, stream, ci, K, table)
            genes, whole = restate.comparable(margins, FLOOR)
            smallest = min(smallest, float(margins.min()))
            assert degenerate == 0
            for k in draws:
                at = f"sample {s} chromosome {c} K={k}"
                dev = got[k]["paths"][ci]
                assert dev.shape == (n, k, alpha.shape[1]) and dev.dtype == np.uint8, at
                np.testing.assert_array_equal(dev[s][genes[:k]], paths[:k][genes[:k]], err_msg=at)
                np.testing.assert_array_equal(got[k]["changes"][s, :, ci][whole[:k]], changes[:k][whole[:k]], err_msg=at)
    return smallest


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H,n", TABLE)
def test_paths_equal_the_restatement(H, n, style):
    hmm, p0 = run_samples(H, style, range(n))
    smallest = assert_equals_the_restatement(hmm, p0, n, SEED)
    hmm.close()
    print(f"DEVIATION smallest decision margin H={H} n={n} {style}: {smallest:.3g} (floor {FLOOR:g})")
    assert smallest >= FLOOR, "a draw was left out of the comparison: pick another seed on the CPU"


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", (8, 16))
def test_tables_one_shorter_than_the_genes(H, style):
    """n_trans = n - 1: only T[0 .. n-2] are read."""
    p0 = short_tables(H, style)
    assert all(len(p0.tprob[c]) == len(p0.gene_ids[c]) - 1 for c in p0.chroms)
    hmm, _ = run_samples(H, style, range(3), p0)
    smallest = assert_equals_the_restatement(hmm, p0, 3, SEED + 1, streams=[5, 2 ** 32 - 1, 0])
    hmm.close()
    assert smallest >= FLOOR


def flat(drawn):
    return np.concatenate(drawn["paths"], axis=-1)


def test_keying(monkeypatch):
    hmm, p0 = run_samples(8, "do", range(3))
    K = 300
    whole = hmm.sample_paths(K, seed=SEED)
    again = hmm.sample_paths(K, seed=SEED)
    np.testing.assert_array_equal(flat(again), flat(whole))                     # two calls, identical bytes
    np.testing.assert_array_equal(again["changes"], whole["changes"])
    one = hmm.sample_paths(K, seed=SEED, sample=1)                              # sample 1 alone = slice 1 of all
    assert one["changes"].shape == (K, len(p0.chroms))
    np.testing.assert_array_equal(flat(one), flat(whole)[1])
    np.testing.assert_array_equal(one["changes"], whole["changes"][1])
    other = hmm.sample_paths(K, seed=SEED + 1)
    assert (flat(other) != flat(whole)).mean() > 0.01                           # another seed, other paths
    keyed = hmm.sample_paths(K, seed=SEED, streams=[7, 8, 9])
    assert (flat(keyed) != flat(whole)).mean() > 0.01                           # another stream, other paths
    # slabs of 37 draws (eight full ones and one of 4): the same bytes
    monkeypatch.setenv("GBRS_TUNING_SAMPLE_SLAB", "37")
    cut = hmm.sample_paths(K, seed=SEED, streams=[7, 8, 9])
    monkeypatch.delenv("GBRS_TUNING_SAMPLE_SLAB")
    np.testing.assert_array_equal(flat(cut), flat(keyed))
    np.testing.assert_array_equal(cut["changes"], keyed["changes"])
    assert hmm.sample_info()[0] > 0 and hmm.sample_info()[1] > 0
    hmm.close()
    # the same sample in a run of its own, with its stream: the batch and the slot play no part
    alone, _ = run_samples(8, "do", [1])
    single = alone.sample_paths(K, seed=SEED, streams=[8])
    np.testing.assert_array_equal(flat(single)[0], flat(keyed)[1])
    np.testing.assert_array_equal(single["changes"][0], keyed["changes"][1])
    alone.close()


def test_marginals_on_the_device():
    """K = 4096 draws at 8 founders, "do": every state's frequency at every gene within six standard errors of the device's
    own gamma, the variance floored at 4 / K (tests/test_sim_geno_cpu.py's bound)."""
    K = 4096
    hmm, p0 = run_samples(8, "do", [0])
    drawn = hmm.sample_paths(K, seed=SEED, sample=0)
    assert drawn["degenerate"] == 0
    worst = 0.0
    for ci, c in enumerate(p0.chroms):
        gamma = hmm.get(ci, want=("gamma",))["gamma"]
        freq = np.stack([(drawn["paths"][ci] == k).mean(axis=0) for k in range(hmm.S)])
        z = np.abs(freq - gamma) / np.sqrt(np.maximum(gamma * (1.0 - gamma), 4.0 / K) / K)
        worst = max(worst, float(z.max()))
    hmm.close()
    print(f"DEVIATION device marginals: worst {worst:.2f} standard errors (bound 6)")
    assert worst <= 6.0


def test_raw_call_errors_leave_the_outputs_untouched():
    """Refusals that return before any launch: no run (GBRS_ERR_STATE); n_draws < 1, a sample out of range, paths == NULL
    (GBRS_ERR_INVALID)."""
    import ctypes as C
    from gbrs_amd import _lib
    from gbrs_amd.hmm import DiplotypeHMM
    lib = _lib.load()
    p0 = grid_cases.problem(3, "benign")
    G = sum(grid_cases.LENS)
    paths, changes = np.full((2, 4, G), 0xAB, dtype=np.uint8), np.full((2, 4, 5), -7, dtype=np.int32)
    count = C.c_uint64(99)

    def call(h, sample, n_draws, out=paths):
        return lib.gbrs_hmm_sample_paths(h, sample, n_draws, 1, None, _lib.ptr(out), _lib.ptr(changes), C.byref(count))

    def untouched():
        return (paths == 0xAB).all() and (changes == -7).all() and count.value == 99

    fresh = DiplotypeHMM(3, p0.chroms, [len(p0.gene_ids[c]) for c in p0.chroms], [p0.tprob[c] for c in p0.chroms])
    assert call(fresh._h, -1, 4) == _lib.GBRS_ERR_STATE and untouched()
    with pytest.raises(_lib.GbrsHipError) as e:
        fresh.sample_paths(4)
    assert e.value.status == _lib.GBRS_ERR_STATE
    fresh.close()
    hmm, _ = run_samples(3, "benign", range(2))
    for n_draws in (0, -1):
        assert call(hmm._h, -1, n_draws) == _lib.GBRS_ERR_INVALID and b"n_draws" in lib.gbrs_last_error() and untouched()
    for sample in (2, -2, 25):
        assert call(hmm._h, sample, 4) == _lib.GBRS_ERR_INVALID and b"sample out of range" in lib.gbrs_last_error()
        assert untouched()
    assert call(hmm._h, -1, 4, out=None) == _lib.GBRS_ERR_INVALID and untouched()
    assert call(None, -1, 4) == _lib.GBRS_ERR_INVALID and untouched()
    with pytest.raises(ValueError, match="streams"):
        hmm.sample_paths(4, streams=[1])
    # new samples on the handle, no run yet
    hmm.set_expression(grid_cases.expression_rows(grid_cases.sample_problem(3, "benign", 2)), expr_threshold=1.5, sigma=0.12)
    assert call(hmm._h, -1, 4) == _lib.GBRS_ERR_STATE and untouched()
    hmm.run()
    assert call(hmm._h, 0, 4) == _lib.GBRS_OK and (paths[0] < 6).all() and (paths[1] == 0xAB).all() and count.value == 0
    assert lib.gbrs_hmm_sample_paths(hmm._h, 0, 4, 1, None, _lib.ptr(paths[1]), None, None) == _lib.GBRS_OK     # nullable outputs
    np.testing.assert_array_equal(paths[1], paths[0])
    hmm.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

H_FILES, STYLE_FILES = 8, "benign"
EXISTING = ("genotypes.tsv", "genoprobs.npz", "genotypes.npz")
GRID = ("interpolated.genoprobs.tsv", "interpolated.genoprobs.npz")
NEW = ("sim_geno.npz", "sim_geno.crossovers.tsv")


@pytest.fixture
def tables(tmp_path, monkeypatch):
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    grid = grid_cases.grids()["b"]
    paths = grid_cases.write_tables(tmp_path, p0, grid.positions)
    paths["grid"] = grid_cases.write_grid_file(tmp_path / "grid.txt", grid.points)
    return paths


def sample_tpm(tmp_path, sample):
    return grid_cases.write_genes_tpm(tmp_path / f"s{sample}.genes.tpm", grid_cases.sample_problem(H_FILES, STYLE_FILES, sample))


def assert_sim_geno_files(stem, hmm, sample, stream, seed, K):
    """The two files of a sample against sample_paths on a handle that ran the same samples."""
    from gbrs_amd.hmm import change_table, viterbi_changes
    p0 = grid_cases.problem(H_FILES, STYLE_FILES)
    want = hmm.sample_paths(K, seed=seed, sample=sample, streams=[stream])
    z = np.load(f"{stem}.sim_geno.npz")
    assert sorted(z.files) == sorted(list(p0.chroms) + ["diplotypes", "seed", "stream"])
    assert int(z["seed"]) == seed and int(z["stream"]) == stream
    names = [a + b for ai, a in enumerate(p0.hap_names) for b in p0.hap_names[ai:]]
    assert list(z["diplotypes"]) == names
    lines = open(f"{stem}.sim_geno.crossovers.tsv").read().splitlines()
    assert lines[0] == "#Chromosome\tGenes\tViterbi\tMean\tSD\tMin\tMax" and len(lines) == 1 + len(p0.chroms)
    table = change_table(H_FILES)
    for ci, c in enumerate(p0.chroms):
        assert z[c].dtype == np.uint8 and z[c].shape == (K, len(p0.gene_ids[c]))
        np.testing.assert_array_equal(z[c], want["paths"][ci])
        x = want["changes"][:, ci].astype(np.float64)
        viterbi = viterbi_changes(hmm.get(ci, sample=sample, want=("calls",))["calls"], table)
        assert lines[1 + ci] == "%s\t%d\t%d\t%.6f\t%.6f\t%d\t%d" % (c, z[c].shape[1], viterbi, x.mean(), x.std(ddof=1),
                                                                   x.min(), x.max())


def same_bytes(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        return fa.read() == fb.read()


def test_reconstruct_with_sim_geno(tmp_path, tables):
    """`-e`: stream 0.  The three files of a plain run, and with --grid-file the five, are byte-identical with and without
    the option; a run without it writes no sim_geno file."""
    from gbrs_amd import cli
    tpm = sample_tpm(tmp_path, 0)
    common = ["reconstruct", "-e", tpm, "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"]]
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "sim"), "--sim-geno", "8", "--sim-geno-seed", "41"]) == 0
    grid = ["--grid-file", tables["grid"], "--grid-genoprobs"]
    assert cli.main(common + grid + ["-o", str(tmp_path / "gplain")]) == 0
    assert cli.main(common + grid + ["-o", str(tmp_path / "gsim"), "--sim-geno", "8"]) == 0
    for suffix in NEW:
        assert not os.path.exists(tmp_path / f"plain.{suffix}") and not os.path.exists(tmp_path / f"gplain.{suffix}")
    for suffix in EXISTING:
        assert same_bytes(tmp_path / f"plain.{suffix}", tmp_path / f"sim.{suffix}"), suffix
    for suffix in EXISTING + GRID:
        assert same_bytes(tmp_path / f"gplain.{suffix}", tmp_path / f"gsim.{suffix}"), suffix
    hmm, _ = run_samples(H_FILES, STYLE_FILES, [0])
    assert_sim_geno_files(str(tmp_path / "sim"), hmm, 0, 0, 41, 8)
    assert_sim_geno_files(str(tmp_path / "gsim"), hmm, 0, 0, 0, 8)
    hmm.close()


def test_sample_file_with_sim_geno(tmp_path, tables):
    """Five samples in launches of 2: a sample's stream is its position in the sample file, whichever launch and slot it
    ran in."""
    from gbrs_amd import cli
    n = 5
    with open(tmp_path / "samples.txt", "w") as fh:
        fh.write("# cohort\n")
        for s in range(n):
            fh.write(f"{sample_tpm(tmp_path, s)}\t{tmp_path / f'many{s}'}\n\n")
    with open(tmp_path / "samples.txt") as src, open(tmp_path / "plain.txt", "w") as dst:
        dst.write(src.read().replace("many", "plain"))
    common = ["--batch-size", "2", "-t", tables["tprob"], "-x", tables["avecs"], "-g", tables["gpos"]]
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "plain.txt")] + common) == 0
    assert cli.main(["reconstruct", "--sample-file", str(tmp_path / "samples.txt"), "--sim-geno", "8"] + common) == 0
    for s in range(n):
        for suffix in NEW:
            assert not os.path.exists(tmp_path / f"plain{s}.{suffix}")
        for suffix in EXISTING:
            assert same_bytes(tmp_path / f"plain{s}.{suffix}", tmp_path / f"many{s}.{suffix}"), (s, suffix)
    for lo in range(0, n, 2):                    # the launches the command made
        members = list(range(lo, min(lo + 2, n)))
        hmm, _ = run_samples(H_FILES, STYLE_FILES, members)
        for slot, s in enumerate(members):
            assert_sim_geno_files(str(tmp_path / f"many{s}"), hmm, slot, s, 0, 8)
        hmm.close()
