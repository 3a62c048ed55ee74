"""The two-samples-per-wave chains of the HIP HMM against the oracle (needs an MI355X).

From 24 samples on (hmm_route.h: `batched`) alpha_wave, delta_wave and back_wave launch forward_wave_kernel and
backward_wave_kernel with two samples per wavefront and a three-set prefetch ring, until the MFMA sweeps and the
samples-on-lanes kernels take over at 64: the default path of `gbrs reconstruct` for 24 to 63 samples at 8 founders, and
for any batch from 24 samples on at 3, 4 and 7 founders.  The rows of tests/hmm_batched_cases.py run here;
tests/test_hmm_route_cpu.py proves on the CPU that each of them takes the route it names.

Every comparison is against oracle.hmm_oracle.reconstruct_arrays (float64 numpy in the reference's order), sample by
sample, at the tolerances of tests/test_hmm_gpu.py.  The samples of a batch are distinct problems (seed + s): a swap of
a wave's two samples, or a read of the other sample's row, changes the numbers.  The Viterbi path and the calls are
compared exactly, which is legitimate only where no decision of the oracle's own backtrace is a near-tie: every sample's
smallest decision margin is asserted to be above MARGIN_MIN first (the seeds were chosen on the CPU so that it is)."""
import functools
import os

import numpy as np
import pytest

from conftest import viterbi_decision_margins
from hmm_batched_cases import CASES, case_id, genes_per_chrom

pytestmark = pytest.mark.gpu

WANT = ("gamma", "states", "calls", "alpha", "beta", "delta", "scaler")
MARGIN_MIN = 1e-6
SEED = 1234               # tables of the table's rows and of the pair test; their samples draw SEED + s, except:
# 3, 4, 5 and 7 founders - a chromosome of one gene none of whose haplotypes is expressed is an exact tie of the oracle's
# (a fifth of the seeds at 3 founders): the first 25 seeds from SEED on without one, in either tprob convention
SAMPLE_SEEDS = {
    7: [1235, 1236, 1237, 1238, 1239, 1240, 1241, 1242, 1243, 1244, 1245, 1246, 1247, 1248, 1249, 1250, 1251, 1252, 1253,
        1254, 1255, 1256, 1257, 1260, 1261],
    5: [1234, 1237, 1238, 1239, 1240, 1241, 1242, 1243, 1244, 1245, 1248, 1250, 1251, 1252, 1253, 1254, 1255, 1258, 1259,
        1260, 1261, 1263, 1264, 1265, 1266],
    4: [1234, 1235, 1236, 1237, 1238, 1239, 1240, 1241, 1243, 1244, 1245, 1246, 1247, 1248, 1250, 1253, 1254, 1257, 1258,
        1259, 1262, 1263, 1264, 1265, 1268],
    3: [1234, 1235, 1236, 1237, 1238, 1239, 1240, 1241, 1243, 1244, 1245, 1246, 1249, 1253, 1254, 1261, 1265, 1266, 1269,
        1270, 1271, 1272, 1274, 1275, 1281],
}
SEED_DO = 5281            # DO-like tables
SEEDS_HANDLE = {40: 5000, 25: 6000, 5: 7000, 24: 8000}     # test_one_handle_shrinking_and_growing_batches: by batch size, in order


def use_env(monkeypatch, env):
    """The library's defaults, then the row's variables."""
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_")):
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ inputs and oracle

@functools.lru_cache(maxsize=None)
def base_problem(H, lens, seed, minus_one, style):
    """Sample 0's problem: its transition tables and specificity entries serve the whole batch."""
    from gbrs_amd import synth
    return synth.make_hmm_problem(H=H, genes_per_chrom=list(lens), seed=seed, tprob_len_minus_one=minus_one, style=style,
                                  expressed_fraction=0.3 if style == "do" else 0.5)


@functools.lru_cache(maxsize=None)
def sample_reference(H, lens, tables_seed, sample_seed, minus_one=False, style="benign", expressed=0.5, silent=False):
    """One sample of a batch on the tables and specificity entries of base_problem(H, lens, tables_seed, ...), its
    expression drawn with sample_seed: (expression rows per chromosome, the oracle's arrays per chromosome, the smallest
    non-zero margin of the oracle's own Viterbi decisions, the number of its exact ties).  Computed once, shared by the
    tests, read-only.  `silent` puts the sample below the expression threshold everywhere."""
    from gbrs_amd import synth
    from oracle import hmm_oracle
    p0 = base_problem(H, lens, tables_seed, minus_one, style)
    p = synth.make_hmm_problem(H=H, genes_per_chrom=list(lens), seed=sample_seed, tprob_len_minus_one=minus_one,
                               style=style, expressed_fraction=expressed)
    scale = 1e-9 if silent else 1.0
    expr = {g: p.expr[g] * scale for c in p0.chroms for g in p0.gene_ids[c]}
    res = hmm_oracle.reconstruct_arrays(p0.hap_names, p0.chroms, p0.gene_ids, p0.tprob, expr, p0.avecs)
    rows = [np.array([expr[g] for g in p0.gene_ids[c]]) for c in p0.chroms]
    gaps = np.concatenate([viterbi_decision_margins(p0.tprob[c], res[c]["delta"]) for c in p0.chroms])
    for a in rows + [v for c in p0.chroms for v in res[c].values()]:
        a.setflags(write=False)
    return rows, [res[c] for c in p0.chroms], float(gaps[gaps > 0].min()), int((gaps == 0).sum())


def make_handle(p0, H):
    from gbrs_amd.hmm import DiplotypeHMM
    chroms = p0.chroms
    hmm = DiplotypeHMM(H, chroms, [len(p0.gene_ids[c]) for c in chroms], [p0.tprob[c] for c in chroms])
    ha = [np.array([g in p0.avecs for g in p0.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([p0.avecs.get(g, np.zeros((H, H))) for g in p0.gene_ids[c]]) for c in chroms]
    return hmm, av, ha


def run_batch(hmm, av, ha, members):
    """members: one sample_reference() result per sample."""
    n_chrom = len(members[0][0])
    hmm.set_expression([np.stack([m[0][ci] for m in members]) for ci in range(n_chrom)], av, ha, 1.5, 0.12)
    hmm.run()


def check_batch(hmm, members, label, exact_ties=()):
    """Every sample against the oracle.  Prints the largest deviations (absolute for the log-domain arrays, relative
    for the posteriors) before it asserts anything about them.  `exact_ties`: samples whose oracle may hold exact ties
    (see test_do_tables_sparse_expression); no sample may hold a near-tie."""
    for s, (_, _, margin, ties) in enumerate(members):
        assert margin > MARGIN_MIN, f"{label} sample {s}: the oracle's own closest decision is won by {margin:.3g} - pick another seed"
        assert ties == 0 or s in exact_ties, f"{label} sample {s}: {ties} exact ties in the oracle's decisions - pick another seed"
    got = [[hmm.get(ci, sample=s, want=WANT) for ci in range(len(m[1]))] for s, m in enumerate(members)]
    dev = dict.fromkeys(("alpha", "beta", "delta", "scaler", "gamma"), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for rs, (_, ref, _, _) in zip(got, members):
            for r, want in zip(rs, ref):
                for k in ("alpha", "beta", "delta", "scaler"):
                    d = np.abs(r[k] - want[k])[np.isfinite(want[k])]
                    dev[k] = max(dev[k], float(d.max()) if d.size else 0.0)
                d = (np.abs(r["gamma"] - want["gamma"]) / want["gamma"])[want["gamma"] > 0]
                dev["gamma"] = max(dev["gamma"], float(d.max()) if d.size else 0.0)
    print(f"DEVIATION {label}: " + " ".join(f"{k}={v:.3g}" for k, v in dev.items()))
    for s, (rs, (_, ref, _, _)) in enumerate(zip(got, members)):
        for ci, (r, want) in enumerate(zip(rs, ref)):
            at = f"{label} sample {s} chromosome {ci}"
            np.testing.assert_array_equal(r["states"], want["states"], err_msg=f"states {at}")
            np.testing.assert_array_equal(r["calls"], want["calls"], err_msg=f"calls {at}")
            for k in ("alpha", "beta", "delta", "scaler"):
                np.testing.assert_allclose(r[k], want[k], rtol=1e-9, atol=1e-9, err_msg=f"{k} {at}")
            np.testing.assert_allclose(r["gamma"], want["gamma"], rtol=1e-8, atol=1e-300, err_msg=f"gamma {at}")
            np.testing.assert_allclose(r["gamma"].sum(axis=0), 1.0, rtol=1e-12, err_msg=f"gamma columns {at}")
    return got


def table_members(case, minus_one):
    lens = tuple(genes_per_chrom(case.founders))
    if case.n_samples > 40:
        lens = lens[:-2]          # the oracle's time on the CPU: 63 samples without the two longest chromosomes
    seeds = SAMPLE_SEEDS.get(case.founders, range(SEED, SEED + case.n_samples))
    return lens, [sample_reference(case.founders, lens, SEED, seeds[s], minus_one) for s in range(case.n_samples)]


# ------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("minus_one", [False, True], ids=["tprob_n", "tprob_n_minus_1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_table_against_oracle(case, minus_one, monkeypatch):
    """Every row of the table, both tprob-length conventions: chromosomes of 1 to 7 genes (0 to 6 steps around the
    three-set ring and its unrolled tail), lengths around the backtrace chunk, an even and an odd sample count (the lone
    sample of a last wave), a partly filled group of the samples-on-lanes backpointer kernel, the mixed routes and the
    stream orderings, 28 / 10 / 6 states, and the quad and generic grids at 25 samples."""
    use_env(monkeypatch, case.env)
    H = case.founders
    lens, members = table_members(case, minus_one)
    hmm, av, ha = make_handle(base_problem(H, lens, SEED, minus_one, "benign"), H)
    run_batch(hmm, av, ha, members)
    check_batch(hmm, members, f"{case_id(case)} {'tprob_n_minus_1' if minus_one else 'tprob_n'}")
    hmm.close()


@pytest.mark.parametrize("n_samples", [25, 40])
def test_do_tables_sparse_expression(n_samples, monkeypatch):
    """DO-like tables (entries down to exp(-69), structural zeros: exp(T) = 0 in the alpha stream, -inf in the delta
    stream) and sparsely expressed samples on the library's defaults.  Sample 1, the second slot of the first wave, is
    below the expression threshold everywhere: its emissions are the prior at every gene while its partner's are not.
    With nothing but the prior, that sample's chromosomes of one and two genes are exact ties of the oracle's for every
    seed (all homozygotes, and all heterozygotes, carry the same init + prior).  Both sides settle them by the first
    index, and the tied values are sums of the same constants on both sides, so its path is still compared exactly;
    its other decisions, like every decision of every other sample, are held to MARGIN_MIN."""
    use_env(monkeypatch, {})
    lens = (1, 2, 17, 64, 150)
    members = [sample_reference(8, lens, SEED_DO, SEED_DO + s, False, "do", 0.9 if s % 3 else 0.3, s == 1)
               for s in range(n_samples)]
    assert all(np.ptp(ref["eprob"], axis=0).max() == 0.0 for ref in members[1][1])        # constant along the chromosome
    assert any(np.ptp(ref["eprob"], axis=0).max() > 0.0 for ref in members[0][1])
    hmm, av, ha = make_handle(base_problem(8, lens, SEED_DO, False, "do"), 8)
    run_batch(hmm, av, ha, members)
    check_batch(hmm, members, f"do tables, {n_samples} samples", exact_ties={1})
    hmm.close()


def test_one_handle_shrinking_and_growing_batches(monkeypatch):
    """One handle, 40 then 25 then 5 then 24 samples of other seeds: `batched` goes off and on again, the grid halves,
    and rows of the larger runs stay behind in the buffers.  A shadow sample that stored, or a last_state left over from
    an earlier run, shows as a wrong sample here."""
    use_env(monkeypatch, {})
    lens = (1, 2, 3, 5, 64, 65, 130)
    tables = SEEDS_HANDLE[40]
    hmm, av, ha = make_handle(base_problem(8, lens, tables, False, "benign"), 8)
    for n_samples, seed in SEEDS_HANDLE.items():
        members = [sample_reference(8, lens, tables, seed + s) for s in range(n_samples)]
        run_batch(hmm, av, ha, members)
        check_batch(hmm, members, f"one handle, {n_samples} samples")
    hmm.close()


def test_pairs_are_independent(monkeypatch):
    """26 samples, then the same samples with 2k and 2k + 1 exchanged for every k: every output of a sample is the same
    bit for bit in either slot of its wave, beside a partner that went first or second."""
    use_env(monkeypatch, {})
    case = CASES[0]._replace(n_samples=26)
    lens, members = table_members(case, False)
    swapped = [members[s ^ 1] for s in range(26)]
    hmm, av, ha = make_handle(base_problem(8, lens, SEED, False, "benign"), 8)
    run_batch(hmm, av, ha, members)
    first = check_batch(hmm, members, "pairs, first order")
    run_batch(hmm, av, ha, swapped)
    for s in range(26):
        for ci in range(len(lens)):
            r = hmm.get(ci, sample=s ^ 1, want=WANT)
            for k in WANT:
                np.testing.assert_array_equal(r[k], first[s][ci][k], err_msg=f"{k} of sample {s} in the other slot, chromosome {ci}")
    hmm.close()
