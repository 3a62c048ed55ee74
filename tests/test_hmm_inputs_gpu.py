"""`gbrs get-transition-prob` / `gbrs get-alignment-spec` on the device (needs an MI355X): the fixtures made by the
reference through the Python functions and through cli.main, shapes the fixtures do not reach against the numpy
restatement, the statuses of the two ABI calls, and the chain the commands exist for - both commands, then
`gbrs reconstruct` on the files they wrote.

Bounds.  Tables: rtol 1e-12, atol 0 - every entry is two logarithms of operands computed identically on both sides
and a subtraction that cannot cancel (first term <= 0, log(1 + gamma) > 0), so the sides differ by the two libraries'
rounding of log only.  axes, ases: equal (adds and one divide in the reference's order).  avecs: rtol 1e-12 (the
norm's sum of squares is added in another order than the BLAS dot product of numpy).  Each test prints the worst
difference it saw before it asserts."""
import os

import numpy as np
import pytest

from conftest import golden_files, load_golden, viterbi_decision_margins
import hmm_inputs_restate as hr

pytestmark = pytest.mark.gpu

TRANPROB = golden_files("tranprob")
ALNSPEC = golden_files("alnspec")
RTOL = 1e-12


def name_of(path):
    return os.path.basename(path)[:-4]


def npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def file_bytes(*paths):
    return [open(p, "rb").read() for p in paths]


# ---- get-transition-prob -----------------------------------------------------------------------------------------------
def run_transition_prob(g, data_dir, tmp_path, how):
    from gbrs_amd import cli, hmm_inputs
    p = hr.tranprob_params(g)
    markers = tmp_path / "markers.tsv"
    markers.write_text(str(g["marker_text"]))
    if how == "function":
        hmm_inputs.get_transition_prob(str(markers), haplotypes=p["haplotypes"], mating_scheme=p["mating_scheme"],
                                       gamma_scale=p["gamma_scale"], epsilon=p["epsilon"], output_file="tables.npz")
    else:
        assert cli.main(["get-transition-prob", "-i", str(markers), "-s", p["haplotypes"], "-m", p["mating_scheme"],
                         "-g", repr(p["gamma_scale"]), "-e", repr(p["epsilon"]), "-o", "tables.npz"]) == 0
    return os.path.join(data_dir, "tables.npz"), os.path.join(data_dir, "ref.gene_pos.ordered.npz")


@pytest.mark.parametrize("how", ["function", "cli"])
@pytest.mark.parametrize("path", TRANPROB, ids=name_of)
def test_transition_prob_fixture(path, how, tmp_path, monkeypatch):
    g = load_golden(path)
    data = tmp_path / "data"
    data.mkdir()
    monkeypatch.setenv("GBRS_DATA", str(data))
    out, gpos_file = run_transition_prob(g, str(data), tmp_path, how)
    assert sorted(os.listdir(data)) == ["ref.gene_pos.ordered.npz", "tables.npz"]
    got, gpos = npz(out), npz(gpos_file)
    want, want_gpos = hr.keyed(g, "tprob"), hr.keyed(g, "gpos")
    assert list(got) == list(want) and list(gpos) == list(want_gpos)        # the reference's member order
    worst = max(hr.max_rel(got[c], want[c]) for c in want)
    print(f"{name_of(path)} [{how}]: worst relative difference of the tables {worst:.3e}")
    for c in want:
        assert got[c].dtype == np.float64 and got[c].shape == want[c].shape, c      # (0, 3, 3) members included
        np.testing.assert_allclose(got[c], want[c], rtol=RTOL, atol=0, err_msg=c)
        assert np.array_equal(gpos[c].astype(str), want_gpos[c].astype(str)), c
    first = file_bytes(out, gpos_file)
    run_transition_prob(g, str(data), tmp_path, how)
    assert [np.array_equal(a, b) for a, b in zip(npz(out).values(), got.values())] == [True] * len(got)
    assert file_bytes(out)[0] == first[0]


def test_transition_prob_absolute_output_path_wins(tmp_path, monkeypatch):
    from gbrs_amd import hmm_inputs
    data = tmp_path / "data"
    data.mkdir()
    monkeypatch.setenv("GBRS_DATA", str(data))
    markers = tmp_path / "m.tsv"
    markers.write_text("g0\t1\t5\t0.5\ng1\t1\t9\t0.75\ng2\tX\t9\t0.75\n")
    hmm_inputs.get_transition_prob(str(markers), output_file=str(tmp_path / "elsewhere.npz"))
    assert os.listdir(data) == ["ref.gene_pos.ordered.npz"]
    t = npz(tmp_path / "elsewhere.npz")
    assert [(c, a.shape) for c, a in t.items()] == [("1", (1, 3, 3)), ("X", (0, 3, 3))]


def big_positions(rng, n):
    steps = rng.uniform(0.0, 0.01, size=n)
    steps[rng.integers(0, n, size=n // 50)] = 0.0                          # zero and sub-epsilon steps throughout
    steps[rng.integers(0, n, size=n // 50)] = 2e-7
    steps[rng.integers(0, n, size=n // 100)] = -0.5
    return np.cumsum(steps)


def test_transition_tables_grid_stride_wraps():
    """1,100,000 intervals (9.9 million doubles, more than the capped grid holds lanes) on an autosome and an X"""
    from gbrs_amd import hmm_inputs
    rng = np.random.default_rng(41)
    positions = [big_positions(rng, 600_001), big_positions(rng, 500_001)]
    got = hmm_inputs.ri_transition_tables(positions, [False, True], 0.01, 1e-6)
    assert [len(t) for t in got] == [600_000, 500_000]
    worst = 0.0
    for t, p, x in zip(got, positions, (False, True)):
        want = hr.ri_table(p, x, 0.01, 1e-6, scalar_logs=False)
        worst = max(worst, hr.max_rel(t, want))
        np.testing.assert_allclose(t, want, rtol=RTOL, atol=0)
    print(f"1.1 million intervals: worst relative difference of the tables {worst:.3e}")
    again = hmm_inputs.ri_transition_tables(positions, [False, True], 0.01, 1e-6)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_transition_tables_without_intervals(hip_lib):
    from gbrs_amd import _lib, hmm_inputs
    assert hmm_inputs.ri_transition_tables([], [], 0.01, 1e-6) == []
    got = hmm_inputs.ri_transition_tables([np.array([1.0]), np.array([2.0]), np.array([0.5])], [False, True, False], 0.01, 1e-6)
    assert [t.shape for t in got] == [(0, 3, 3)] * 3
    # chromosomes without a marker between chromosomes with intervals: nothing is read across a boundary
    parts = [np.array([0.0, 1.0, 3.0]), np.zeros(0), np.array([7.0]), np.array([100.0, 100.5])]
    got = hmm_inputs.ri_transition_tables(parts, [False, False, True, True], 0.01, 1e-6)
    assert [len(t) for t in got] == [2, 0, 0, 1]
    np.testing.assert_allclose(got[0], hr.ri_table(parts[0], False, 0.01, 1e-6), rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[3], hr.ri_table(parts[3], True, 0.01, 1e-6), rtol=RTOL, atol=0)
    zero = np.zeros(1, dtype=np.int64)
    assert hip_lib.gbrs_ri_transition_tables(None, _lib.ptr(zero), None, 0, 0.01, 1e-6, 0, None) == _lib.GBRS_OK


# ---- get-alignment-spec ------------------------------------------------------------------------------------------------
def run_alignment_spec(g, data, how, capsys):
    from gbrs_amd import cli, hmm_inputs
    sample_file, strains, min_expr, missing = hr.alnspec_write_inputs(g, data)
    capsys.readouterr()
    if how == "function":
        hmm_inputs.get_alignment_spec(sample_file, strains, min_expr=min_expr)
    else:
        argv = ["get-alignment-spec", "-i", sample_file, "-s", ",".join(strains[:2])]
        for s in strains[2:]:
            argv += ["-s", s]
        assert cli.main(argv + ["-m", repr(min_expr)]) == 0
    assert capsys.readouterr().out == "".join(f"File {p} does not exist.\n" for p in missing)
    return [os.path.join(str(data), f"{k}.npz") for k in ("axes", "ases", "avecs")]


@pytest.mark.parametrize("how", ["function", "cli"])
@pytest.mark.parametrize("path", ALNSPEC, ids=name_of)
def test_alignment_spec_fixture(path, how, tmp_path, monkeypatch, capsys):
    g = load_golden(path)
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    files = run_alignment_spec(g, tmp_path, how, capsys)
    axes, ases, avecs = (npz(f) for f in files)
    want_axes, want_ases, want_avecs = hr.keyed(g, "axes"), hr.keyed(g, "ases"), hr.keyed(g, "avecs")
    assert list(axes) == list(want_axes) and list(ases) == list(want_ases)
    assert list(avecs) == list(want_avecs)                                  # the key set, in the gene list's order
    worst = max(hr.max_rel(avecs[k], want_avecs[k]) for k in want_avecs)
    with capsys.disabled():
        print(f"{name_of(path)} [{how}]: worst relative difference of avecs {worst:.3e}")
    for k in want_axes:
        assert axes[k].shape == want_axes[k].shape and np.array_equal(axes[k], want_axes[k]), k
        assert ases[k].shape == want_ases[k].shape and np.array_equal(ases[k], want_ases[k]), k
    for k in want_avecs:
        np.testing.assert_allclose(avecs[k], want_avecs[k], rtol=RTOL, atol=0, err_msg=k)
    first = file_bytes(*files)
    run_alignment_spec(g, tmp_path, how, capsys)
    assert file_bytes(*files) == first


def test_alignment_spec_strain_without_a_line(tmp_path, monkeypatch, capsys):
    from gbrs_amd import hmm_inputs
    g = load_golden([p for p in ALNSPEC if p.endswith("alnspec_s2.npz")][0])
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    sample_file, strains, min_expr, _ = hr.alnspec_write_inputs(g, tmp_path)
    with pytest.raises(KeyError):
        hmm_inputs.get_alignment_spec(sample_file, [strains[0], "Z"], min_expr=min_expr)


def random_spec_case(S, G, seed):
    """files per strain 1-3 (strain 0 one file, one strain with a listed file that is missing when S > 1), values that are
    exact in binary thirds apart so that sums in another order would show, some rows at the branch points"""
    rng = np.random.default_rng(seed)
    tables, divisors = [], []
    for i in range(S):
        n = 1 if i == 0 else int(rng.integers(1, 4))
        mine = [np.round(rng.lognormal(0.0, 1.5, size=(G, S)) * (rng.random((G, S)) < 0.7), 3) for _ in range(n)]
        for t in mine:
            t[3] = 0.0                                                      # a gene nobody expresses
            t[5] = rng.uniform(0.0, 1.9 / S, size=S)                        # below min_expr everywhere
        tables.append(mine)
        divisors.append(n + (1 if i == S - 1 and S > 1 else 0))
    tables[0][0][7] = 0.0
    tables[0][0][7, 0] = 7e-7                                               # 0 < sum <= 1e-6
    tables[0][0][9] = 0.0
    tables[0][0][9, -1] = 2.0                                               # a row sum equal to min_expr
    for i in range(1, S):
        for t in tables[i]:
            t[9] = 0.0
    return tables, divisors


@pytest.mark.parametrize("S", [1, 3, 5, 16, 32])
def test_alignment_spec_other_strain_counts(S):
    """every template width, and counts that do not fill theirs; 70 genes"""
    from gbrs_amd import hmm_inputs
    G = 70
    tables, divisors = random_spec_case(S, G, 500 + S)
    want_axes, want_ases, want_avecs, want_has = hr.spec_from_tables(tables, divisors, 2.0)
    ptr = np.concatenate(([0], np.cumsum([len(t) for t in tables])))
    stacked = np.stack([t for mine in tables for t in mine])
    axes, ases, avecs, has = hmm_inputs.alignment_spec_arrays(stacked, ptr, divisors, G, S, 2.0)
    assert np.array_equal(has.astype(bool), want_has) and not want_has[[3, 5, 9]].any() and want_has.sum() > 5
    assert np.array_equal(axes, want_axes) and np.array_equal(ases, want_ases)
    print(f"S={S}: worst relative difference of avecs {hr.max_rel(avecs[want_has], want_avecs[want_has]):.3e}")
    np.testing.assert_allclose(avecs[want_has], want_avecs[want_has], rtol=RTOL, atol=0)
    assert np.array_equal(avecs[7, 0], axes[7, 0]) and axes[7, 0, 0] == 7e-7
    again = hmm_inputs.alignment_spec_arrays(stacked, ptr, divisors, G, S, 2.0)
    assert all(np.array_equal(a, b) for a, b in zip((axes, ases, avecs, has), again))


# ---- the two ABI calls ---------------------------------------------------------------------------------------------------
def test_abi_statuses(hip_lib):
    from gbrs_amd import _lib, hmm_inputs
    lib, p = hip_lib, _lib.ptr
    cm = np.array([0.0, 1.0, 2.0, 0.5, 0.75])
    ptr = np.array([0, 3, 5], dtype=np.int64)
    x = np.array([0, 1], dtype=np.uint8)
    out = np.empty((3, 3, 3))
    good = lambda: lib.gbrs_ri_transition_tables(p(cm), p(ptr), p(x), 2, 0.01, 1e-6, 0, p(out))       # noqa: E731
    assert good() == _lib.GBRS_OK
    for args in ((None, p(ptr), p(x), 2, 0.01, 1e-6, 0, p(out)), (p(cm), None, p(x), 2, 0.01, 1e-6, 0, p(out)),
                 (p(cm), p(ptr), None, 2, 0.01, 1e-6, 0, p(out)), (p(cm), p(ptr), p(x), 2, 0.01, 1e-6, 0, None),
                 (p(cm), p(ptr), p(x), -1, 0.01, 1e-6, 0, p(out)),
                 (p(cm), p(np.array([0, 3, 2], dtype=np.int64)), p(x), 2, 0.01, 1e-6, 0, p(out)),          # decreasing
                 (p(cm), p(np.array([1, 3, 5], dtype=np.int64)), p(x), 2, 0.01, 1e-6, 0, p(out))):
        assert lib.gbrs_ri_transition_tables(*args) == _lib.GBRS_ERR_INVALID
        assert lib.gbrs_last_error()
    with pytest.raises(_lib.GbrsHipError, match="chrom_ptr decreases"):
        _lib.check(lib.gbrs_ri_transition_tables(p(cm), p(np.array([0, 3, 2], dtype=np.int64)), p(x), 2, 0.01, 1e-6, 0, p(out)))
    first = out.copy()
    assert good() == _lib.GBRS_OK and np.array_equal(out, first)

    G, S = 4, 2
    tables = np.ones((2, G, S))
    sp, sd = np.array([0, 1, 2], dtype=np.int64), np.array([1, 1], dtype=np.int64)
    axes, ases, avecs, has = np.empty((G, S, S)), np.empty((G, S)), np.empty((G, S, S)), np.zeros(G, dtype=np.uint8)
    spec = lambda *a: lib.gbrs_alignment_spec(*a)                                                       # noqa: E731
    ok = (p(tables), p(sp), p(sd), G, S, 2.0, 0, p(axes), p(ases), p(avecs), p(has))
    assert spec(*ok) == _lib.GBRS_OK
    for k in (0, 1, 2, 7, 8, 9, 10):
        bad = list(ok)
        bad[k] = None
        assert spec(*bad) == _lib.GBRS_ERR_INVALID, k
        assert lib.gbrs_last_error()
    for n in (0, 33, -1):
        bad = list(ok)
        bad[4] = n
        assert spec(*bad) == _lib.GBRS_ERR_UNSUPPORTED
    bad = list(ok)
    bad[1] = p(np.array([0, 2, 1], dtype=np.int64))
    assert spec(*bad) == _lib.GBRS_ERR_INVALID
    bad = list(ok)
    bad[2] = p(np.array([1, 0], dtype=np.int64))
    assert spec(*bad) == _lib.GBRS_ERR_INVALID
    bad = list(ok)
    bad[3] = -1
    assert spec(*bad) == _lib.GBRS_ERR_INVALID
    bad = list(ok)
    bad[3] = 0
    assert spec(*bad) == _lib.GBRS_OK                                        # no gene: nothing to do
    first = [a.copy() for a in (axes, ases, avecs, has)]
    assert spec(*ok) == _lib.GBRS_OK
    assert all(np.array_equal(a, b) for a, b in zip(first, (axes, ases, avecs, has)))
    assert np.array_equal(ases, np.full((G, S), 2.0)) and not has.any()      # 2.0 is not above min_expr
    with pytest.raises(_lib.GbrsHipError):
        hmm_inputs.alignment_spec_arrays(np.ones((1, 2, 33)), np.zeros(34, dtype=np.int64), np.ones(33, dtype=np.int64),
                                         2, 33, 2.0)


# ---- the loop the commands exist for -------------------------------------------------------------------------------------
# the seed was fixed on the CPU, with the restatement's tables and blocks in the oracle: the smallest decision margins are
# 0.126 (1), 0.073 (2) and 1.50 (X), and every chromosome is called AA in places and BB in others
CROSS_SEED = 7
CROSS_CHROMS = (("1", 170), ("2", 100), ("X", 30))


def cross_inputs(g, seed=CROSS_SEED):
    """A two-founder recombinant inbred sample over the 300 genes of alnspec_s2: (marker text, ref.fa.fai text, genes.tpm
    text).  Every chromosome is a mosaic of AA and BB stretches; a gene's TPMs are its founder's mean row with 10 % noise."""
    rng = np.random.default_rng(seed)
    genes = [str(k) for k in g["axes_keys"]]
    axes = hr.keyed(g, "axes")
    assert len(genes) == sum(n for _, n in CROSS_CHROMS)
    markers, expr, k = [], ["locus\tA\tB\ttotal\n"], 0
    for chrom, n in CROSS_CHROMS:
        cm, bp, founder = 0.0, 3_000_000, int(rng.integers(0, 2))
        for _ in range(n):
            cm = round(cm + float(rng.uniform(0.05, 1.5)), 4)
            bp += int(rng.integers(10_000, 900_000))
            if rng.random() < 0.03:
                founder = 1 - founder
            v = np.round(axes[genes[k]][founder] * rng.lognormal(0.0, 0.1, size=2), 3)
            markers.append(f"{genes[k]}\t{chrom}\t{bp}\t{cm!r}\n")
            expr.append(f"{genes[k]}\t{float(v[0])!r}\t{float(v[1])!r}\t{float(v.sum())!r}\n")
            k += 1
    fai = "".join(f"{c}\t{200_000_000 - 10_000_000 * i}\t{100 * i + 3}\t60\t61\n" for i, (c, _) in enumerate(CROSS_CHROMS))
    return "".join(markers), fai, "".join(expr)


def test_both_commands_then_reconstruct(tmp_path, monkeypatch, capsys):
    """quantified founders -> get-alignment-spec, a marker file -> get-transition-prob, then reconstruct with no -x / -g:
    it finds avecs.npz and ref.gene_pos.ordered.npz where the two commands left them."""
    from gbrs_amd import cli
    from oracle import hmm_oracle
    g = load_golden([p for p in ALNSPEC if p.endswith("alnspec_s2.npz")][0])
    data = tmp_path / "data"
    data.mkdir()
    monkeypatch.setenv("GBRS_DATA", str(data))
    marker_text, fai_text, expr_text = cross_inputs(g)
    sample_file, strains, min_expr, _ = hr.alnspec_write_inputs(g, data)
    (data / "ref.fa.fai").write_text(fai_text)
    markers, expr_file = tmp_path / "markers.tsv", tmp_path / "sample.genes.tpm"
    markers.write_text(marker_text)
    expr_file.write_text(expr_text)
    assert cli.main(["get-alignment-spec", "-i", sample_file, "-s", ",".join(strains)]) == 0
    assert cli.main(["get-transition-prob", "-i", str(markers)]) == 0
    for name in ("avecs.npz", "tranprob.npz", "ref.gene_pos.ordered.npz"):
        assert (data / name).is_file(), name
    outbase = str(tmp_path / "sample")
    assert cli.main(["reconstruct", "-e", str(expr_file), "-t", str(data / "tranprob.npz"), "-o", outbase]) == 0

    tprob, avecs = npz(data / "tranprob.npz"), npz(data / "avecs.npz")
    gene_ids = {c: [str(r[0]) for r in a] for c, a in npz(data / "ref.gene_pos.ordered.npz").items()}
    chroms = [c for c, _ in CROSS_CHROMS]
    assert list(tprob) == chroms and [len(gene_ids[c]) for c in chroms] == [n for _, n in CROSS_CHROMS]
    expr = {}
    for line in expr_text.splitlines()[1:]:
        item = line.split("\t")
        expr[item[0]] = np.array([float(item[1]), float(item[2])])
    ref = hmm_oracle.reconstruct_arrays(strains, chroms, gene_ids, tprob, expr, avecs)
    names = ["AA", "AB", "BB"]
    gamma, path = npz(outbase + ".genoprobs.npz"), npz(outbase + ".genotypes.npz")
    calls = dict(line.split("\t") for line in open(outbase + ".genotypes.tsv").read().splitlines()[1:])
    want_calls = {}
    for c in chroms:
        margin = viterbi_decision_margins(tprob[c], ref[c]["delta"]).min()
        print(f"chromosome {c}: smallest Viterbi decision margin {margin:.3e}, "
              f"worst relative difference of gamma {hr.max_rel(gamma[c], ref[c]['gamma']):.3e}")
        assert margin > 1e-6, (c, margin)                                   # no tie can hide as a pass
        assert [str(s) for s in path[c]] == [names[s] for s in ref[c]["states"]], c
        want_calls.update((gid, names[s]) for gid, s in zip(gene_ids[c], ref[c]["calls"]) if s >= 0)
        np.testing.assert_allclose(gamma[c], ref[c]["gamma"], rtol=1e-8, atol=1e-300, err_msg=c)
        assert {0, 2} <= set(ref[c]["calls"].tolist()), c                   # the mosaic is really called: AA and BB
    assert calls == want_calls and len(calls) == 300 - len(chroms)            # a chromosome's last gene gets no call
