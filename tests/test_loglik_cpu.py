"""Host side of the log-likelihood pass (`gbrs reconstruct --loglik / --alt-tprob-file / --model-report`):
the restatement against the oracle's own scaler, choose_tables, the argument checks, the parser, the two writers, the
checks of the alternative files, and the margins of the fixtures whose selection tests/test_loglik_gpu.py asserts."""
import os

import numpy as np
import pytest

import grid_cases
import loglik_cases as cases
import loglik_restate as restate
from gbrs_amd.hmm import (ReconstructContext, check_loglik_args, choose_tables, loglik_totals, write_loglik_table,
                          write_model_report)


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("H", cases.HS)
def test_restatement_is_the_oracles_scaler(H, style):
    """-forward(T, E, init)[1].sum() on the base tables is -scaler.sum() of reconstruct_arrays, chromosome by chromosome;
    a one-gene chromosome's value is the log of its first normaliser."""
    res, _ = grid_cases.oracle_arrays(H, style, 0)
    got = restate.per_chromosome(H, style, 0)
    want = np.array([-res[c]["scaler"].sum() for c in grid_cases.CHROMS])
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(got).all() and (got <= 0).all()
    assert got[0] == -res["1"]["scaler"][0]
    assert choose_tables(got[None].T.sum(axis=0, keepdims=True))[0].tolist() == [0]


def test_choose_tables_by_hand():
    inf, nan = np.inf, np.nan
    total = np.array([[-10.0, -5.0, -7.0, nan, -inf, -3.0, nan],
                      [-10.0, -4.0, -9.0, -8.0, -inf, nan, nan],
                      [-12.0, -4.0, -7.0, -9.0, -inf, -inf, nan]])
    best, margin = choose_tables(total)
    assert best.tolist() == [0, 1, 0, 1, 0, 0, 0]                       # ties: the first listed wins
    assert margin.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, inf, 0.0]       # NaN counts as -inf; all -inf: 0.0
    one, m1 = choose_tables(np.array([[-3.0, nan, -inf]]))
    assert one.tolist() == [0, 0, 0] and m1.tolist() == [inf, inf, inf]
    b2, m2 = choose_tables(np.array([[-5.0, -1.0], [-2.0, -4.0]]))
    assert b2.tolist() == [1, 0] and m2.tolist() == [3.0, 3.0]
    assert choose_tables(np.zeros((2, 0)))[0].shape == (0,)
    with pytest.raises(ValueError):
        choose_tables(np.zeros(3))
    rng = np.random.default_rng(5)
    for _ in range(20):
        t = rng.normal(size=(4, 9)).round(1)
        t[rng.random(t.shape) < 0.2] = nan
        t[rng.random(t.shape) < 0.2] = -inf
        got, want = choose_tables(t), restate.choose(t)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_totals_add_in_handle_order():
    per = np.array([[[1e16, 1.0, -1e16, 1.0]], [[1.0, 1.0, 1e16, -1e16]]])
    assert loglik_totals(per).tolist() == [[1.0], [2.0]]      # left to right: 1e16 + 1.0 is 1e16
    assert loglik_totals(per[:, 0, :]).tolist() == [1.0, 2.0]
    assert loglik_totals(np.zeros((2, 3, 0))).tolist() == [[0.0] * 3] * 2


def test_argument_checks(tmp_path):
    a, b, t = (str(tmp_path / f"{k}.npz") for k in "abt")
    check_loglik_args()
    check_loglik_args(True, None, None, False, tprob_file=t)
    check_loglik_args(False, [a, b], None, False, tprob_file=t)
    check_loglik_args(False, [a], str(tmp_path / "r.tsv"), True, tprob_file=t)
    for alts, cohort in (([a], False), (None, True), ([], True)):
        with pytest.raises(RuntimeError, match="--model-report needs --sample-file and at least one --alt-tprob-file"):
            check_loglik_args(True, alts, "r.tsv", cohort, tprob_file=t)
    with pytest.raises(RuntimeError, match="same file as -t"):
        check_loglik_args(False, [a, t], None, False, tprob_file=t)
    with pytest.raises(RuntimeError, match="same file as --alt-tprob-file"):
        check_loglik_args(False, [a, b, str(tmp_path / "." / "a.npz")], None, False, tprob_file=t)
    os.symlink(t, tmp_path / "link.npz")
    with pytest.raises(RuntimeError, match="same file as -t"):
        check_loglik_args(False, [str(tmp_path / "link.npz")], None, True, tprob_file=t)


def test_parser(tmp_path):
    from gbrs_amd import cli
    files = {}
    for k in ("e", "t", "a", "b"):
        files[k] = str(tmp_path / k)
        open(files[k], "w").close()
    parse = cli.build_parser().parse_args
    args = parse(["reconstruct", "-e", files["e"], "-t", files["t"]])
    assert args.loglik is False and args.alt_tprob_file is None and args.model_report is None
    args = parse(["reconstruct", "-e", files["e"], "-t", files["t"], "--loglik"])
    assert args.loglik is True and args.alt_tprob_file is None
    args = parse(["reconstruct", "-e", files["e"], "-t", files["t"], "--alt-tprob-file", files["a"], "--alt-tprob-file",
                  files["b"], "--model-report", "r.tsv"])
    assert args.alt_tprob_file == [files["a"], files["b"]] and args.model_report == "r.tsv" and args.tprob_file == files["t"]
    with pytest.raises(SystemExit):
        parse(["reconstruct", "-e", files["e"], "-t", files["t"], "--alt-tprob-file", str(tmp_path / "missing")])
    with pytest.raises(SystemExit):                                      # -t stays single and required
        parse(["reconstruct", "-e", files["e"], "--alt-tprob-file", files["a"]])


def test_the_two_writers(tmp_path):
    per = np.array([[-1.5, -0.1, -2.0 / 3.0], [-np.inf, -0.25, -1e-300]])
    write_loglik_table(tmp_path / "s.loglik.tsv", ["1", "2", "X"], [4, 1, 7], ["dir/F.npz", "M.npz"], per, 0)
    assert open(tmp_path / "s.loglik.tsv").read().splitlines() == [
        "chromosome\tgenes\tdir/F.npz\tM.npz",
        "1\t4\t-1.5\t-inf",
        "2\t1\t-0.1\t-0.25",
        f"X\t7\t{-2.0 / 3.0!r}\t-1e-300",
        f"total\t12\t{(-1.5 + -0.1) + -2.0 / 3.0!r}\t-inf",
        "# selected: dir/F.npz"]
    write_loglik_table(tmp_path / "one.tsv", ["7"], [3], ["t.npz"], np.array([[-4.0]]), 0)
    assert open(tmp_path / "one.tsv").read() == "chromosome\tgenes\tt.npz\n7\t3\t-4.0\ntotal\t3\t-4.0\n# selected: t.npz\n"
    write_loglik_table(tmp_path / "none.tsv", [], [], ["t.npz", "u.npz"], np.zeros((2, 0)), 1)
    assert open(tmp_path / "none.tsv").read() == "chromosome\tgenes\tt.npz\tu.npz\ntotal\t0\t0.0\t0.0\n# selected: u.npz\n"
    write_model_report(tmp_path / "r.tsv", ["F.npz", "M.npz"],
                       [("out/a", 0, 12.5, np.array([-100.0, -112.5])), ("out/b", 1, np.inf, np.array([-np.inf, -3.0]))])
    assert open(tmp_path / "r.tsv").read().splitlines() == [
        "#outbase\tselected\tmargin\tF.npz\tM.npz", "out/a\tF.npz\t12.5\t-100.0\t-112.5", "out/b\tM.npz\tinf\t-inf\t-3.0"]
    write_model_report(tmp_path / "empty.tsv", ["F.npz", "M.npz"], [])
    assert open(tmp_path / "empty.tsv").read() == "#outbase\tselected\tmargin\tF.npz\tM.npz\n"


def test_alternative_files_are_checked_before_any_sample_runs(tmp_path, monkeypatch):
    """A missing chromosome, one the base lacks, another state count and too few blocks: RuntimeErrors that name the file
    and the chromosome, from load() and alt_tables() - no device is touched."""
    H = 3
    p0 = grid_cases.problem(H, "benign")
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    paths = grid_cases.write_tables(tmp_path, p0, grid_cases.gene_positions())
    base = dict(zip(p0.chroms, cases.candidate(H, "benign", "base")))

    def context(name, tables):
        f = str(tmp_path / f"{name}.npz")
        np.savez(f, **tables)
        return f, ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"], alt_tprob_files=[f])

    f, ctx = context("missing", {c: t for c, t in base.items() if c != "3"})
    with pytest.raises(RuntimeError) as e:
        ctx.load()
    assert f in str(e.value) and "chromosome 3" in str(e.value)
    f, ctx = context("extra", dict(base, MT=base["2"]))
    with pytest.raises(RuntimeError) as e:
        ctx.load()
    assert f in str(e.value) and "chromosome MT" in str(e.value)
    f, ctx = context("states", dict(base, X=cases.candidate(2, "benign", "base")[4]))
    ctx.load()
    with pytest.raises(RuntimeError) as e:
        ctx.alt_tables(H)
    assert f in str(e.value) and "chromosome X" in str(e.value) and "(n, 6, 6)" in str(e.value)
    f, ctx = context("blocks", dict(base, X=base["X"][:198]))
    ctx.load()
    with pytest.raises(RuntimeError) as e:
        ctx.alt_tables(H)
    assert f in str(e.value) and "chromosome X" in str(e.value) and "198 blocks for 200 genes" in str(e.value)
    # files that fit: n - 1 blocks are enough, none for the one-gene chromosome; equal tables are found equal
    f, ctx = context("fits", dict(base, X=base["X"][:199], **{"1": base["1"][:0], "4": base["4"] + 0.0}))
    ctx.load()
    tabs = ctx.alt_tables(H)
    assert len(tabs) == 1 and [t.shape[0] for t in tabs[0]] == [0, 2, 3, 65, 199]
    assert ctx.alt_same == [[False, True, True, True, False]]
    assert ctx.loglik_launches == 0


@pytest.mark.parametrize("H,style,alts,samples", [
    (cases.COMMAND_H, cases.COMMAND_STYLE, cases.COMMAND_ALTS, cases.COMMAND_SAMPLES),
    (cases.SINGLE_H, cases.SINGLE_STYLE, cases.SINGLE_ALTS, 1),
    (cases.TIE_H, "do", ("other", "x_only"), 2),
])
def test_selection_fixtures_are_decided_or_exact_ties(H, style, alts, samples):
    """The cohorts whose selected model the GPU tests assert: the oracle's own margin is above 1e-6, or - one founder, every
    table log(1) - the totals tie exactly and the first listed candidate wins."""
    total = restate.totals(H, style, range(samples), ("base",) + tuple(alts))
    best, margin = choose_tables(total)
    np.testing.assert_array_equal(best, restate.choose(total)[0])
    if H == 1:
        assert (total == total[0]).all() and (best == 0).all() and (margin == 0.0).all()
    else:
        assert (margin > 1e-6).all(), margin
    print(f"selection H={H} {style}: {best.tolist()}, smallest margin {margin.min():.3g}")


def test_the_command_cohort_has_samples_that_stay_and_samples_that_move():
    total = restate.totals(cases.COMMAND_H, cases.COMMAND_STYLE, range(cases.COMMAND_SAMPLES), ("base",) + cases.COMMAND_ALTS)
    best = choose_tables(total)[0]
    assert (best == 0).any() and (best != 0).any()
