"""What a handle keeps of a run does not outlive it: after new emissions and a new run, every pass over the run - panel
match, grid dosages and probabilities, SNP dosages, diagnostics, log-likelihoods - returns what a handle that has only ever
seen the new emissions returns, byte for byte (the same kernels on the same inputs: no tolerance).  The match runs before
the grid pass, so after the first round the handle holds the grid dosages, the SNP pass's founder dosages and the
log-domain arrays of the old run, each marked as made: a flag that a new run failed to clear would serve the old
numbers."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, GENES = 3, (12, 7)
S = H * (H + 1) // 2


@pytest.fixture(autouse=True)
def library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_")):
            monkeypatch.delenv(k, raising=False)


def setting():
    """Tables, specificities, gene and grid positions, a panel of three and ten SNPs for two chromosomes of 12 and 7 genes."""
    from gbrs_amd import synth
    p = synth.make_hmm_problem(H=H, genes_per_chrom=list(GENES), seed=77)
    rng = np.random.default_rng(78)
    where = [np.sort(rng.uniform(1.0, 90.0, size=n)) for n in GENES]
    grid = [np.linspace(0.0, 95.0, 9), np.linspace(0.5, 91.0, 5)]
    panel = [rng.random((9 + 5, H)) for _ in range(3)]
    snps = [np.sort(rng.uniform(0.0, 95.0, size=6)), np.sort(rng.uniform(0.0, 95.0, size=4))]
    masks = [rng.integers(0, 1 << H, size=len(x), dtype=np.uint32) for x in snps]
    return p, where, grid, panel, snps, masks


def new_handle(cfg):
    from gbrs_amd.hmm import DiplotypeHMM
    p, where, grid, panel, snps, masks = cfg
    hmm = DiplotypeHMM(H, p.chroms, list(GENES), [p.tprob[c] for c in p.chroms])
    hmm.set_grid(where, grid)
    hmm.set_panel(panel)
    hmm.set_snps(where, snps, masks)
    return hmm


def expression(cfg, seed):
    """Two samples' rows, [2, n_c, H] per chromosome, with the specificity tables."""
    p = cfg[0]
    rng = np.random.default_rng(seed)
    rows = [rng.gamma(1.0, 5.0, size=(2, n, H)) * (rng.random((2, n, H)) < 0.6) for n in GENES]
    av = [np.array([p.avecs.get(g, np.zeros((H, H))) for g in p.gene_ids[c]]) for c in p.chroms]
    ha = [np.array([g in p.avecs for g in p.gene_ids[c]], dtype=np.uint8) for c in p.chroms]
    return rows, av, ha


def emissions(seed):
    """Two samples' log emission rows, [2, n_c, S] per chromosome."""
    rng = np.random.default_rng(seed)
    rows = [rng.random((2, n, S)) + 0.05 for n in GENES]
    return [np.log(r / r.sum(axis=-1, keepdims=True)) for r in rows]


def passes(hmm):
    """Every pass with sample = -1, the match first (it makes or reuses the grid dosages), as flat arrays by name."""
    match = hmm.match()
    grid = hmm.grid(want=("dosage", "gamma_grid"))
    out = {"cross": match["cross"], "sample_norm": match["sample_norm"], "dosage": grid["dosage"],
           "gamma_grid": np.concatenate([g.ravel() for per in grid["gamma_grid"] for g in per]),
           "impute": hmm.impute(), "loglik": hmm.loglik()}
    for name, per in hmm.diagnostics().items():
        out[name] = np.concatenate([a.ravel() for a in per])
    return out


def load(hmm, cfg, kind, seed):
    if kind == "expression":
        rows, av, ha = expression(cfg, seed)
        hmm.set_expression(rows, av, ha, 1.5, 0.12)
    else:
        hmm.set_eprob(emissions(seed))
    hmm.run()


@pytest.mark.parametrize("kind", ("expression", "eprob"))
def test_a_second_run_of_the_same_emissions_equals_the_first(kind):
    """run, the passes (the log-domain arrays are made), run again with no new emissions, the passes again: the arrays are
    made once per run, from that run, and everything equals the first round and a fresh handle's."""
    cfg = setting()
    used = new_handle(cfg)
    load(used, cfg, kind, 2)
    first = passes(used)
    used.run()
    second = passes(used)
    used.close()
    fresh = new_handle(cfg)
    load(fresh, cfg, kind, 2)
    want = passes(fresh)
    fresh.close()
    for name in want:
        np.testing.assert_array_equal(first[name], want[name], err_msg=name)
        np.testing.assert_array_equal(second[name], want[name], err_msg=name)


@pytest.mark.parametrize("kind", ("expression", "eprob"))
def test_a_rerun_handle_equals_a_fresh_one(kind):
    cfg = setting()
    used = new_handle(cfg)
    load(used, cfg, kind, 1)
    first = passes(used)
    load(used, cfg, kind, 2)
    second = passes(used)
    used.close()
    fresh = new_handle(cfg)
    load(fresh, cfg, kind, 2)
    want = passes(fresh)
    fresh.close()
    assert set(second) == set(want) and len(want) == 11
    for name in want:
        assert want[name].size > 0 and np.isfinite(want[name]).all(), name
        assert not np.array_equal(first[name], want[name]), f"{name}: the two runs have to differ for this test to see anything"
        np.testing.assert_array_equal(second[name], want[name], err_msg=name)
