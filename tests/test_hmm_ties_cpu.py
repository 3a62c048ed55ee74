"""Viterbi decisions that are exact ties or inside the rounding of delta: the fixtures' conditions, the oracle against
the recorded reference outputs, the path helper against itself, the generator's jitter switch (no GPU)."""
import hashlib
from itertools import combinations_with_replacement

import numpy as np
import pytest

import hmm_ties
from conftest import golden_files, hmm_case_inputs, load_golden, viterbi_decision_margins
from oracle import hmm_oracle

TIE_FILES = golden_files("hmmtie")
IDS = [p.split("/")[-1][:-4] for p in TIE_FILES]


def decision_counts(g, c, ch):
    margins, slacks = hmm_ties.decision_table(c["tprob"][ch], g[f"delta_{ch}"], g[f"states_{ch}"])
    return margins, slacks


def test_tie_fixture_set_is_complete():
    assert IDS == ["hmmtie_h16_silent_weak", "hmmtie_h4_silent_weak", "hmmtie_h8_equal_founders",
                   "hmmtie_h8_silent_only", "hmmtie_h8_weak"]
    # the wide-margin test and the existing golden tests glob hmm_*.npz: no tie fixture may enter them
    assert not set(TIE_FILES) & set(golden_files("hmm"))


@pytest.mark.parametrize("path", TIE_FILES, ids=IDS)
def test_hmm_oracle_matches_reference_outputs_on_ties(path):
    """The Viterbi recursion and the backtrace are adds, max and argmax: from the stored emissions and tables the oracle
    gives the reference's delta, path and calls bit for bit on any machine.  The quantities that go through exp / log are
    held at test_hmm_oracle_matches_reference_outputs's tolerances."""
    g = load_golden(path)
    c = hmm_case_inputs(g)
    iv = hmm_oracle.init_vector(c["H"])
    np.testing.assert_array_equal(iv, g["init_vec"])
    for ch in c["chroms"]:
        n = len(c["genes"][ch])
        T = c["tprob"][ch]
        delta, states, calls = hmm_oracle.viterbi(T, g[f"eprob_{ch}"], g["init_vec"])
        np.testing.assert_array_equal(delta, g[f"delta_{ch}"])
        np.testing.assert_array_equal(states, g[f"states_{ch}"])
        np.testing.assert_array_equal(calls, g[f"calls_{ch}"])
        E = np.array([hmm_oracle.emission(c["expr"][ch][i], c["avecs"][ch][i] if c["has_avec"][ch][i] else None, iv,
                                          float(g["expr_threshold"]), float(g["sigma"])) for i in range(n)])
        np.testing.assert_allclose(E, g[f"eprob_{ch}"], rtol=1e-12, atol=0)
        alpha, scaler = hmm_oracle.forward(T, E, iv)
        gamma = hmm_oracle.posterior(alpha, hmm_oracle.backward(T, E, scaler))
        np.testing.assert_allclose(gamma, g[f"gamma_{ch}"], rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(gamma.sum(axis=0), 1.0, rtol=1e-12)
        if len(T) == n - 1:
            assert calls[-1] == -1 and len(states) == n
        else:
            assert len(T) == n and (calls >= 0).all() and len(states) == n + 1


@pytest.mark.parametrize("path", TIE_FILES, ids=IDS)
def test_every_tie_fixture_has_an_exact_tie_and_few_close_decisions(path):
    g = load_golden(path)
    c = hmm_case_inputs(g)
    zero = close = total = 0
    for ch in c["chroms"]:
        margins, slacks = decision_counts(g, c, ch)
        # the helper's margins are conftest's
        np.testing.assert_array_equal(margins, viterbi_decision_margins(c["tprob"][ch], g[f"delta_{ch}"]))
        zero += int((margins == 0).sum())
        close += int((margins <= slacks).sum())
        total += len(margins)
    assert zero >= 1
    assert close <= 0.05 * total, (close, total)


def test_the_tie_fixtures_hold_a_decision_inside_the_rounding():
    """0 < margin <= slack somewhere in the set: a call that rounding decides, not the first-index rule."""
    near = 0
    for path in TIE_FILES:
        g = load_golden(path)
        c = hmm_case_inputs(g)
        for ch in c["chroms"]:
            margins, slacks = decision_counts(g, c, ch)
            near += int(((margins > 0) & (margins <= slacks)).sum())
    assert near >= 1


def test_silent_only_fixture_ties_only_where_every_emission_is_the_prior():
    """hmmtie_h8_silent_only: every decision is wide or an exact tie, and the exact ties sit in chromosomes none of whose
    genes reaches the expression threshold - there a device-computed emission is the prior itself, so the report text
    must be identical with device emissions too."""
    g = load_golden([p for p in TIE_FILES if p.endswith("hmmtie_h8_silent_only.npz")][0])
    c = hmm_case_inputs(g)
    ties = 0
    for ch in c["chroms"]:
        margins, slacks = decision_counts(g, c, ch)
        assert not ((margins > 0) & (margins <= slacks)).any(), ch
        if (margins == 0).any():
            ties += 1
            assert (c["expr"][ch].sum(axis=1) < float(g["expr_threshold"])).all(), ch
            np.testing.assert_array_equal(g[f"eprob_{ch}"], np.tile(g["init_vec"], (len(c["genes"][ch]), 1)))
    assert ties >= 3


# ------------------------------------------------------------------------------------------------ the helper itself

def tie_problem():
    """A class-constant problem with prior emissions: the final argmax ties among the heterozygotes."""
    H, n = 8, 30
    T = hmm_ties.class_constant_tables(H, n, seed=3)
    E = hmm_ties.symmetric_emissions(H, n, "prior", seed=4)
    iv = hmm_oracle.init_vector(H)
    delta, states, _ = hmm_oracle.viterbi(T, E, iv)
    return T, delta, states


def test_helper_accepts_the_reference_path():
    T, delta, states = tie_problem()
    assert hmm_ties.assert_path_eps_optimal(T, delta, states) == 0
    for path in TIE_FILES:
        g = load_golden(path)
        c = hmm_case_inputs(g)
        for ch in c["chroms"]:
            assert hmm_ties.assert_path_eps_optimal(c["tprob"][ch], g[f"delta_{ch}"], g[f"states_{ch}"]) == 0


def test_helper_accepts_another_candidate_of_an_exact_tie():
    T, delta, states = tie_problem()
    last = delta[:, -1]
    tied = np.flatnonzero(last == last.max())
    assert len(tied) == 28 and states[-1] == tied[0]          # the heterozygotes; np.argmax took the first
    other = np.array(states)
    other[-1] = tied[5]
    other = hmm_ties.follow_argmax(T, delta, other, len(other) - 1)
    assert not np.array_equal(other, states)
    assert hmm_ties.assert_path_eps_optimal(T, delta, other) == 1


def test_helper_rejects_a_decision_worse_than_the_slack():
    T, delta, states = tie_problem()
    # a tie moved apart by five times the slack: the loser is no longer acceptable
    d2 = delta.copy()
    tied = np.flatnonzero(d2[:, -1] == d2[:, -1].max())
    d2[tied[0], -1] += 5 * hmm_ties.slack(d2[:, -1])
    bad = np.array(states)
    bad[-1] = tied[5]
    bad = hmm_ties.follow_argmax(T, d2, bad, len(bad) - 1)
    with pytest.raises(AssertionError, match="backtrace step 0"):
        hmm_ties.assert_path_eps_optimal(T, d2, bad)
    # ... and inside the slack it still is
    d3 = delta.copy()
    d3[tied[0], -1] += 0.5 * hmm_ties.slack(d3[:, -1])
    assert hmm_ties.assert_path_eps_optimal(T, d3, hmm_ties.follow_argmax(T, d3, bad, len(bad) - 1)) == 1


def test_helper_rejects_a_path_that_differs_at_a_wide_decision():
    g = load_golden([p for p in TIE_FILES if p.endswith("hmmtie_h8_silent_only.npz")][0])
    c = hmm_case_inputs(g)
    ch = c["chroms"][3]                                        # the ordinary chromosome: every margin is wide
    T, delta, states = c["tprob"][ch], g[f"delta_{ch}"], g[f"states_{ch}"]
    margins, slacks = hmm_ties.decision_table(T, delta, states)
    assert (margins > slacks).all()
    for at in (len(states) - 1, len(states) // 2, 0):
        bad = np.array(states)
        bad[at] = (bad[at] + 1) % delta.shape[0]
        with pytest.raises(AssertionError, match="backtrace step"):
            hmm_ties.assert_path_eps_optimal(T, delta, hmm_ties.follow_argmax(T, delta, bad, at))
    with pytest.raises(AssertionError):
        hmm_ties.assert_path_eps_optimal(T, delta, states[:-1])


@pytest.mark.parametrize("H", [2, 3, 4, 5, 7, 8, 9, 16])
@pytest.mark.parametrize("kind", ["prior", "one", "two"])
def test_class_constant_problems_tie(H, kind):
    """The in-test inputs of the GPU tiers do hold exact ties (bit-identical candidates) at every founder count with
    symmetric states (3 founders on): in the recursion, at the final argmax and inside the backtrace."""
    n = 65
    T = hmm_ties.class_constant_tables(H, n, seed=10 + H)
    assert len(np.unique(T[0])) == 3 and np.isneginf(T[1]).any() and len(np.unique(T[4])) == 1
    E = hmm_ties.symmetric_emissions(H, n, kind, seed=20 + H)
    delta, states, _ = hmm_oracle.viterbi(T, E, hmm_oracle.init_vector(H))
    margins, slacks = hmm_ties.decision_table(T, delta, states)
    assert not ((margins > 0) & (margins <= slacks)).any()     # exact ties only: nothing here is left to rounding
    if H == 2:
        return                                                 # AA, AB, BB: the prior favours AB, nothing is symmetric to it
    assert (margins[1:] == 0).any(), margins                   # margins[0] is the final argmax
    # the recursion itself ties: some state's best predecessor is not unique at some gene
    v = delta[:, :-1].T[:, None, :] + T[:n - 1]
    top = np.sort(v, axis=2)
    assert (top[:, :, -1] == top[:, :, -2]).any()


# ------------------------------------------------------------------------------------------------ the generator switch

def ulp_distance(a, b):
    """Largest difference in units of the last place.  The entries are logs of column-normalised probabilities; a
    relabelling changes the order in which a column was summed, which moves the probability by an ulp or two of itself
    and its log by that much in absolute terms.  On the near-zero logs of the near-one diagonal that is many ulps of
    the entry, so the unit is the ulp of max(|entry|, 1)."""
    fin = np.isfinite(a)
    np.testing.assert_array_equal(fin, np.isfinite(b))
    return np.max(np.abs(a[fin] - b[fin]) / np.spacing(np.maximum(np.abs(a[fin]), 1.0)))


@pytest.mark.parametrize("H", [4, 8])
def test_jitter_zero_tables_are_symmetric_under_founder_relabelling(H):
    from gbrs_amd import synth
    prob = synth.make_hmm_problem(H=H, genes_per_chrom=[9, 6], seed=5, style="do", jitter=0)
    pairs = list(combinations_with_replacement(range(H), 2))
    index = {p: k for k, p in enumerate(pairs)}
    rng = np.random.default_rng(1)
    perms = [tuple(reversed(range(H))), tuple(np.roll(np.arange(H), 1))] + [tuple(rng.permutation(H)) for _ in range(3)]
    for perm in perms:
        image = np.array([index[tuple(sorted((perm[a], perm[b])))] for a, b in pairs])
        for ch in prob.chroms:
            T = prob.tprob[ch]
            assert ulp_distance(T[:, image][:, :, image], T) <= 4
    # and the default call is not: that is what the jitter is for
    jit = synth.make_hmm_problem(H=H, genes_per_chrom=[9, 6], seed=5, style="do")
    T = jit.tprob[jit.chroms[0]]
    image = np.array([index[tuple(sorted((perms[0][a], perms[0][b])))] for a, b in pairs])
    assert ulp_distance(T[:, image][:, :, image], T) > 1e6


def test_default_jitter_draws_the_tables_of_the_earlier_generator():
    """The default call is unchanged by the switch: a table hashed (rounded to 1e-6, far above the last bits in which
    np.log may differ between machines) against the value computed from the generator before the switch existed, and a
    committed fixture regenerated."""
    from gbrs_amd import synth
    prob = synth.make_hmm_problem(H=8, genes_per_chrom=[12], seed=2024, style="do")
    T = prob.tprob[prob.chroms[0]]
    key = np.where(np.isfinite(T), np.round(T, 6) + 0.0, -1e300)
    assert hashlib.sha256(key.tobytes()).hexdigest() == PARENT_TABLE_SHA256
    g = load_golden([p for p in golden_files("hmm") if p.endswith("hmm_h8_do_short.npz")][0])
    again = synth.make_hmm_problem(H=8, genes_per_chrom=[70, 45, 30], seed=36, tprob_len_minus_one=True, style="do")
    for ch in again.chroms:
        np.testing.assert_allclose(again.tprob[ch], g[f"tprob_{ch}"], rtol=1e-14, atol=0)
        np.testing.assert_array_equal(np.array([again.expr[x] for x in again.gene_ids[ch]]), g[f"expr_{ch}"])


PARENT_TABLE_SHA256 = "f9e111a793b2c9efb24185bbab8bbb7f4d8682604e7d9f1972ae05e91d59d8ab"
