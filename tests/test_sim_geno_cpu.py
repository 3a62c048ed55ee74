"""The definition of `gbrs reconstruct --sim-geno` checked on the CPU: tests/sim_geno_restate.py draws
from the posterior that oracle.hmm_oracle.reconstruct_arrays computes - every state's frequency at every gene against
`gamma`, and the pooled transition counts against the pair posteriors made from the oracle's alpha, beta and emission
arrays, which the restatement's own rule has no part in.  Plus the change table, the uniform's range and the command's
refusals.  No GPU.

The bounds: a frequency over K independent draws has variance g (1 - g) / K; six standard errors, the variance floored at
4 / K so that a state the draws never visit is held to 12 / K.  Of the 0.3 M (state, gene) cells of the largest case the
chance that one exceeds six standard errors is about 1e-3 (2e-9 each, two-sided normal; the floor only lowers it)."""
import functools
import logging
import os

import numpy as np
import pytest

import grid_cases
import sim_geno_restate as restate

K = 4096
SEED = 20240229            # fixed: the restatement passes every bound below with it
STYLES = ("benign", "do")
FOUNDERS = (3, 8, 16)


@functools.lru_cache(maxsize=None)
def draws(H, style):
    """Per chromosome of the table's problem: K paths drawn by the restatement from the oracle's alpha."""
    res, _ = grid_cases.oracle_arrays(H, style, 0)
    p = grid_cases.problem(H, style)
    out = {}
    for ci, c in enumerate(p.chroms):
        paths, changes, margins, degenerate = restate.sample_paths(res[c]["alpha"], p.tprob[c], SEED, 0, ci, K)
        assert degenerate == 0
        paths.setflags(write=False)
        out[c] = paths
    return out


def standard_error(variance):
    return np.sqrt(np.maximum(variance, 4.0 / K) / K)


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", FOUNDERS)
def test_marginals_are_the_posterior(H, style):
    res, _ = grid_cases.oracle_arrays(H, style, 0)
    S = H * (H + 1) // 2
    worst = 0.0
    for c, paths in draws(H, style).items():
        gamma = res[c]["gamma"]                                                # (S x n)
        assert paths.shape == (K, gamma.shape[1]) and paths.max() < S
        freq = np.stack([(paths == k).mean(axis=0) for k in range(S)])
        z = np.abs(freq - gamma) / standard_error(gamma * (1.0 - gamma))
        worst = max(worst, float(z.max()))
    print(f"DEVIATION marginals H={H} {style}: worst {worst:.2f} standard errors (bound 6)")
    assert worst <= 6.0


def pair_posterior(res_c, T):
    """sum over i of xi_i(k, j), xi_i(k, j) ~ exp(alpha[k, i] + T[i][j, k] + eprob[i + 1][j] + beta[j, i + 1]) normalised
    per i: the posterior of (z_i = k, z_{i+1} = j) from the oracle's arrays."""
    alpha, beta, E = res_c["alpha"], res_c["beta"], res_c["eprob"]
    S, n = alpha.shape
    total = np.zeros((S, S))
    for i in range(n - 1):
        with np.errstate(divide="ignore"):
            lx = alpha[:, i][:, None] + T[i].T + (E[i + 1] + beta[:, i + 1])[None, :]      # [k, j]
        x = np.exp(lx - lx.max())
        total += x / x.sum()
    return total


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("H", FOUNDERS)
def test_pooled_transitions_are_the_pair_posterior(H, style):
    """Per chromosome the mean over the draws of N[k, j] = #{i : z_i = k, z_{i+1} = j} against sum_i xi_i(k, j), within six
    of the mean's own standard errors (the draws' variance of N[k, j], floored like the marginals').  With T[i]
    transposed the "benign" cases miss the bound by a factor of 20 (their tables are asymmetric; the "do" recipe's are
    symmetric), with T[i - 1] in place of T[i] both styles do (98 and 2048 standard errors at 8 founders)."""
    res, _ = grid_cases.oracle_arrays(H, style, 0)
    p = grid_cases.problem(H, style)
    S = H * (H + 1) // 2
    worst = 0.0
    for c, paths in draws(H, style).items():
        n = paths.shape[1]
        if n < 2:
            continue
        want = pair_posterior(res[c], p.tprob[c])
        pair = paths[:, :-1].astype(np.int64) * S + paths[:, 1:]
        s1, s2 = np.zeros(S * S), np.zeros(S * S)
        for lo in range(0, K, 256):                        # per-draw count matrices, 256 draws at a time
            block = pair[lo:lo + 256]
            rows = np.repeat(np.arange(len(block)), n - 1)
            counts = np.bincount(rows * (S * S) + block.ravel(), minlength=len(block) * S * S).reshape(len(block), S * S)
            s1 += counts.sum(axis=0)
            s2 += (counts.astype(np.float64) ** 2).sum(axis=0)
        mean = s1 / K
        variance = (s2 - K * mean ** 2) / (K - 1)
        z = np.abs(mean - want.ravel()) / standard_error(variance)
        worst = max(worst, float(z.max()))
    print(f"DEVIATION pooled transitions H={H} {style}: worst {worst:.2f} standard errors (bound 6)")
    assert worst <= 6.0


@pytest.mark.parametrize("H", range(1, 17))
def test_change_table(H):
    from gbrs_amd.hmm import change_table
    want = restate.change_table(H)
    got = change_table(H)
    assert got.dtype == np.uint8 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    if H >= 3:       # AA -> AB is 1, AB -> CC is 2 (states: AA AB AC .. BB ..)
        from itertools import combinations_with_replacement
        st = list(combinations_with_replacement(range(H), 2))
        assert got[st.index((0, 0)), st.index((0, 1))] == 1 and got[st.index((0, 1)), st.index((2, 2))] == 2


def test_viterbi_changes_skip_genes_without_a_call():
    from gbrs_amd.hmm import change_table, viterbi_changes
    tab = change_table(3)                   # AA AB AC BB BC CC
    assert viterbi_changes([0, 0, 1, 5], tab) == 0 + 1 + 2
    assert viterbi_changes([0, -1, 1, 5], tab) == 2          # 0 -> (none) -> 1 are not neighbours that both have a call
    assert viterbi_changes([3], tab) == 0 and viterbi_changes([], tab) == 0


def test_uniform_is_in_the_half_open_interval():
    assert restate.u_from_words(0, 0) == 0.0
    top = float(restate.u_from_words(0xFFFFFFFF, 0xFFFFFFFF))
    assert top == 1.0 - 2.0 ** -53 and top < 1.0
    assert float(restate.u_from_words(1 << 5, 0)) == 2.0 ** -27 and float(restate.u_from_words(0, 1 << 6)) == 2.0 ** -53
    u = restate.uniforms(SEED, 3, 2, 7, 5)
    assert u.shape == (5, 7) and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 35
    # a draw's uniforms do not depend on how many draws or genes are asked for beside it
    np.testing.assert_array_equal(restate.uniforms(SEED, 3, 2, 4, 2), u[:2, :4])


def test_threshold_rounded_up_to_the_total():
    """u * c_{S-1} = c_{S-1} happens for a subnormal total: no c_k is above t, and the largest k with w_k > 0 is taken;
    a total of 0 takes the first argmax and is counted."""
    tiny = np.log(5e-324)
    logw = np.array([[-np.inf, tiny, -np.inf], [-np.inf, -np.inf, -np.inf], [-800.0, -790.0, -790.0]])
    u = np.array([1.0 - 2.0 ** -53, 0.5, 0.5])
    assert u[0] * 5e-324 == 5e-324
    z, margin, degenerate = restate.pick(logw, u)
    assert list(z) == [1, 0, 1] and list(degenerate) == [False, True, True]
    z, _, degenerate = restate.pick(np.log(np.array([[0.25, 0.5, 0.25]])), np.array([0.75]))
    assert list(z) == [2] and not degenerate[0]             # c_1 = 0.75 is not above t = 0.75


def test_comparable_cuts_a_draw_at_its_first_close_decision():
    m = np.full((3, 5), 1.0)
    m[1, 2] = 1e-13
    m[2, 4] = 0.0
    genes, whole = restate.comparable(m)
    assert list(whole) == [True, False, False]
    assert genes[0].all() and list(genes[1]) == [False, False, False, True, True] and not genes[2].any()


@pytest.mark.parametrize("value", [0, -3])
def test_command_refuses_a_bad_count_before_reading_a_file(tmp_path, caplog, value):
    """K < 1 ends in the catch-all's logged error; the inputs (empty files here) are never opened and nothing is written."""
    from gbrs_amd import cli
    tpm, tprob = tmp_path / "s.genes.tpm", tmp_path / "tprob.npz"
    tpm.write_text("")
    tprob.write_bytes(b"")
    out = tmp_path / "out"
    with caplog.at_level(logging.ERROR, logger="gbrs"):
        assert cli.main(["reconstruct", "-e", str(tpm), "-t", str(tprob), "-o", str(out), "--sim-geno", str(value)]) == 0
    assert any("--sim-geno must be at least 1" in r.getMessage() for r in caplog.records)
    assert sorted(os.listdir(tmp_path)) == ["s.genes.tpm", "tprob.npz"]


def test_functions_refuse_bad_arguments():
    from gbrs_amd.hmm import check_sim_geno_args, reconstruct, reconstruct_many
    check_sim_geno_args(None)
    check_sim_geno_args(1, 2 ** 64 - 1)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(RuntimeError, match="--sim-geno must be at least 1"):
            check_sim_geno_args(bad)
    for seed in (-1, 2 ** 64):
        with pytest.raises(RuntimeError, match="--sim-geno-seed"):
            check_sim_geno_args(4, seed)
    with pytest.raises(RuntimeError, match="--sim-geno must be at least 1"):
        reconstruct("missing.tpm", "missing.npz", sim_geno=0)
    with pytest.raises(RuntimeError, match="--sim-geno must be at least 1"):
        reconstruct_many(["missing.tpm"], ["out"], "missing.npz", sim_geno=0)


def test_parser_takes_the_two_options():
    from gbrs_amd import cli
    here = os.path.abspath(__file__)
    args = cli.build_parser().parse_args(["reconstruct", "-e", here, "-t", here, "--sim-geno", "8", "--sim-geno-seed", "5"])
    assert (args.sim_geno, args.sim_geno_seed) == (8, 5)
    args = cli.build_parser().parse_args(["reconstruct", "-e", here, "-t", here])
    assert (args.sim_geno, args.sim_geno_seed) == (None, 0)


def test_files_of_a_sample(tmp_path):
    """The two files' names and contents from given draws: the (K x n_c) arrays, the state names, seed and stream; one
    line per chromosome in handle order with %.6f mean and sd (ddof 1), nan at K = 1."""
    import types
    from gbrs_amd.hmm import _save_sim_geno
    ctx = types.SimpleNamespace(chroms=["2", "1"])
    paths = [np.array([[0, 1, 2], [2, 2, 2], [1, 1, 0]], dtype=np.uint8), np.array([[1], [0], [2]], dtype=np.uint8)]
    changes = np.array([[2, 0], [0, 0], [1, 0]], dtype=np.int32)
    stem = str(tmp_path / "s")
    _save_sim_geno(stem, ctx, ["AA", "AB", "BB"], (paths, changes, [1, 0]), seed=2 ** 63 + 1, stream=7)
    assert sorted(os.listdir(tmp_path)) == ["s.sim_geno.crossovers.tsv", "s.sim_geno.npz"]
    z = np.load(stem + ".sim_geno.npz")
    assert sorted(z.files) == ["1", "2", "diplotypes", "seed", "stream"]
    np.testing.assert_array_equal(z["2"], paths[0])
    np.testing.assert_array_equal(z["1"], paths[1])
    assert z["2"].dtype == np.uint8 and list(z["diplotypes"]) == ["AA", "AB", "BB"]
    assert int(z["seed"]) == 2 ** 63 + 1 and int(z["stream"]) == 7
    lines = open(stem + ".sim_geno.crossovers.tsv").read().splitlines()
    assert lines == ["#Chromosome\tGenes\tViterbi\tMean\tSD\tMin\tMax",
                     "2\t3\t1\t1.000000\t1.000000\t0\t2", "1\t1\t0\t0.000000\t0.000000\t0\t0"]
    _save_sim_geno(stem, ctx, ["AA", "AB", "BB"], ([q[:1] for q in paths], changes[:1], [1, 0]), seed=0, stream=0)
    assert open(stem + ".sim_geno.crossovers.tsv").read().splitlines()[1] == "2\t3\t1\t2.000000\tnan\t2\t2"
