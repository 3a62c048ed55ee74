"""Multiread models 1-3: the emmodel_*.npz fixtures (made by running the reference) against the closed-form numpy
restatement of tests/em_models_restate.py (no GPU)."""
import numpy as np
import pytest

from conftest import golden_files, load_golden
from em_models_restate import ModelsEM, fixture_inputs

FIXTURES = golden_files("emmodel")


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def restatement(g):
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    return ModelsEM(R, L, H, indptr, indices, count, eff_len, groups, gtmask), groups


def test_fixtures_present():
    assert len(FIXTURES) >= 21
    assert {int(load_golden(p)["model"]) for p in FIXTURES} == {1, 2, 3}
    assert not golden_files("em") or all("emmodel" not in p for p in golden_files("em"))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-4])
def test_restatement_reproduces_fixture(path):
    g = load_golden(path)
    cpu, groups = restatement(g)
    model = int(g["model"])
    snaps = {}
    theta, counts, hist = cpu.run(g["theta0"].copy(), model, float(g["tol"]), int(g["max_iters"]),
                                  on_iter=lambda i, t: snaps.__setitem__(i, t.copy()))
    assert len(hist) == int(g["num_iters"])
    for k in (1, 2, 5):
        if f"theta_iter{k}" in g:
            assert rel(snaps[k], g[f"theta_iter{k}"]) < 1e-12
    assert rel(theta, g["theta_final"]) < 1e-12
    assert rel(counts, g["expected_counts"]) < 1e-12
    np.testing.assert_allclose(hist, g["err_history"], rtol=1e-9)
    np.testing.assert_allclose(cpu.group_sums(theta, groups), g["gene_theta"], rtol=1e-12)
    np.testing.assert_allclose(cpu.group_sums(counts, groups), g["gene_counts"], rtol=1e-12)


@pytest.mark.parametrize("path", [p for p in FIXTURES if "_m1_" in p], ids=lambda p: p.split("/")[-1][:-4])
def test_fixtures_separate_the_models(path):
    """One step from theta0 gives four different answers (one haplotype: models 1-3 coincide, only 4 differs), and
    the stored first snapshot is the fixture's own model's."""
    g = load_golden(path)
    cpu, _ = restatement(g)
    one = {m: cpu.step(g["theta0"], m)[0] for m in (1, 2, 3, 4)}
    for a in (1, 2, 3):
        for b in range(a + 1, 5):
            if int(g["num_haps"]) > 1 or b == 4:
                assert rel(one[a], one[b]) > 1e-3, (a, b)
    assert rel(one[1], g["theta_iter1"]) < 1e-12


def test_cross_gene_reads_present():
    """Model 3 equals Model 4 when every read stays inside one gene: the fixtures have reads that cross genes and
    loci in no group."""
    g = load_golden(FIXTURES[0])
    cpu, groups = restatement(g)
    n_genes_per_read = np.array([len(np.unique(cpu.g[cpu.r == r])) for r in range(cpu.R)])
    assert (n_genes_per_read > 1).sum() > 50
    grouped = np.zeros(cpu.L, dtype=bool)
    grouped[np.concatenate([np.asarray(m) for m in groups])] = True
    assert (~grouped).sum() > 0
