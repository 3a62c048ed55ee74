"""`gbrs get-transition-prob` / `gbrs get-alignment-spec` without a device: the numpy restatement against the
tranprob_*.npz / alnspec_*.npz fixtures (made by running the reference, scripts/gen_golden_hmm_inputs.py), the parser
flags, the signatures, the refusals and the text parsers of gbrs_amd.hmm_inputs."""
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT, golden_files, load_golden
import hmm_inputs_restate as hr

TRANPROB = golden_files("tranprob")
ALNSPEC = golden_files("alnspec")


def name_of(path):
    return os.path.basename(path)[:-4]


def test_fixture_set():
    assert [name_of(p) for p in TRANPROB] == ["tranprob_main", "tranprob_params"]
    assert [name_of(p) for p in ALNSPEC] == ["alnspec_s2", "alnspec_s8"]
    for p in TRANPROB + ALNSPEC:
        assert os.path.getsize(p) < 200_000
    for prefix in ("em", "emmodel", "hmm", "hmmtie", "tensor", "matops", "counts", "compress", "posterior", "postproc",
                   "sharedreads"):
        assert not set(golden_files(prefix)) & set(TRANPROB + ALNSPEC)


@pytest.mark.parametrize("path", TRANPROB, ids=name_of)
def test_transition_restatement_matches_reference(path):
    g = load_golden(path)
    p = hr.tranprob_params(g)
    tables, gpos = hr.transition_prob(str(g["marker_text"]), p["gamma_scale"], p["epsilon"])
    ref_t, ref_g = hr.keyed(g, "tprob"), hr.keyed(g, "gpos")
    assert list(tables) == list(ref_t) == list(gpos) == list(ref_g)          # order of first appearance
    for c in ref_t:
        assert tables[c].shape == ref_t[c].shape and ref_t[c].dtype == np.float64
        assert np.array_equal(tables[c], ref_t[c]), c
        assert np.array_equal(gpos[c], ref_g[c].astype(str)), c


def test_transition_fixtures_hold_what_the_kernel_can_get_wrong():
    g = load_golden([p for p in TRANPROB if p.endswith("tranprob_main.npz")][0])
    t = hr.keyed(g, "tprob")
    assert [(c, len(a)) for c, a in t.items()] == [("1", 69), ("X", 4), ("2", 300), ("x", 2), ("Y", 1), ("MT", 0)]
    assert t["MT"].shape == (0, 3, 3)
    markers = hr.parse_markers(str(g["marker_text"]))
    chrom_of_line = [line.split("\t")[1] for line in str(g["marker_text"]).splitlines()]
    first, last = chrom_of_line.index("1"), len(chrom_of_line) - 1 - chrom_of_line[::-1].index("1")
    assert "X" in chrom_of_line[first:last]                                # `1` is not contiguous in the file
    eps = float(g["epsilon"])
    d = np.diff(markers["1"][2])
    assert (d == 0).any() and (d < 0).any() and ((d > 0) & (d < eps)).any() and (np.abs(d - 50.0) < 1e-6).any()
    dx = np.diff(markers["X"][2])
    assert (dx == 0).any() and ((dx > 0) & (dx < eps)).any() and (np.abs(dx - 50.0) < 1e-6).any()
    # X and the autosome `x` take different formulas: row 2 is not row 0 mirrored on X
    assert not np.array_equal(t["X"][:, 2, ::-1], t["X"][:, 0]) and np.array_equal(t["x"][:, 2, ::-1], t["x"][:, 0])
    for a in t.values():
        assert np.isfinite(a).all()
        assert np.array_equal(a[:, 1], np.full((len(a), 3), np.log(1 / 3.0)))
    g = load_golden([p for p in TRANPROB if p.endswith("tranprob_params.npz")][0])
    assert (float(g["gamma_scale"]), float(g["epsilon"])) == (0.25, 1e-3) and len(hr.keyed(g, "tprob")) == 2


@pytest.mark.parametrize("path", ALNSPEC, ids=name_of)
def test_alignment_spec_restatement_matches_reference(path):
    g = load_golden(path)
    strains = [str(s) for s in g["strains"]]
    axes, ases, avecs, missing = hr.alignment_spec(str(g["gene_text"]), str(g["sample_text"]), hr.alnspec_reports(g),
                                                   strains, float(g["min_expr"]))
    assert missing == [str(p) for p in g["missing_paths"]]
    ref_axes, ref_ases, ref_avecs = hr.keyed(g, "axes"), hr.keyed(g, "ases"), hr.keyed(g, "avecs")
    assert list(axes) == list(ref_axes) and list(ases) == list(ref_ases)
    assert list(avecs) == list(ref_avecs)                                  # the key set, in the gene list's order
    S = len(strains)
    for k in ref_axes:
        assert axes[k].shape == (S, S) and np.array_equal(axes[k], ref_axes[k]), k
        assert ases[k].shape == (1, S) and np.array_equal(ases[k], ref_ases[k]), k
    for k in ref_avecs:
        np.testing.assert_allclose(avecs[k], ref_avecs[k], rtol=1e-15, atol=0, err_msg=k)


@pytest.mark.parametrize("path", ALNSPEC, ids=name_of)
def test_alignment_spec_fixtures_hold_what_the_kernel_can_get_wrong(path):
    g = load_golden(path)
    sp = dict(zip((str(x) for x in g["special_names"]), (str(x) for x in g["special_genes"])))
    assert set(sp) == {"absent", "twice", "nofile", "low", "one", "zero", "tiny", "exact"}
    S, min_expr = len(g["strains"]), float(g["min_expr"])
    axes, ases, avecs = hr.keyed(g, "axes"), hr.keyed(g, "ases"), hr.keyed(g, "avecs")
    texts = [str(t) for t in g["report_texts"]]
    count = [sum(line.startswith(sp["twice"] + "\t") for line in t.splitlines()) for t in texts]
    assert 2 in count
    assert 0 in [sum(line.startswith(sp["absent"] + "\t") for line in t.splitlines()) for t in texts]
    assert not any(sp["nofile"] + "\t" in t for t in texts) and not axes[sp["nofile"]].any()
    assert any("ENSMUSG_NOT_LISTED\t" in t for t in texts) and "ENSMUSG_NOT_LISTED" not in axes
    assert sp["low"] not in avecs and ases[sp["low"]].max() <= min_expr
    assert sp["exact"] not in avecs and ases[sp["exact"]].max() == min_expr
    assert (ases[sp["one"]][0] > min_expr).sum() == 1 and sp["one"] in avecs
    assert not axes[sp["zero"]][0].any() and sp["zero"] in avecs
    assert 0 < ases[sp["tiny"]][0, 0] <= 1e-6 and np.array_equal(avecs[sp["tiny"]][0], axes[sp["tiny"]][0])
    assert len(avecs) < len(axes)
    listed = [line.split("\t")[0] for line in str(g["sample_text"]).splitlines()]
    per_strain = sorted({listed.count(str(s)) for s in g["strains"]})
    if S == 2:
        assert (len(axes), per_strain, len(g["missing_paths"])) == (300, [1, 3], 1)
    else:
        assert (S, len(axes), per_strain) == (8, 130, [1, 2, 3])


# ---- the command line and the Python functions -----------------------------------------------------------------------------
def subparser(name):
    from gbrs_amd.cli import build_parser
    return build_parser()._subparsers._group_actions[0].choices[name]


def flags_of(parser):
    return {tuple(a.option_strings): a for a in parser._actions}


def test_get_transition_prob_flags_match_the_reference(tmp_path):
    """gbrs/commands.py:282-291"""
    from gbrs_amd.cli import build_parser
    f = flags_of(subparser("get-transition-prob"))
    assert {("-i", "--marker-file"), ("-s", "--haplotypes"), ("-m", "--mating-scheme"), ("-g", "--gamma-scale"),
            ("-e", "--epsilon"), ("-o", "--output"), ("-v", "--verbose"), ("--device",)} <= set(f)
    assert f[("-i", "--marker-file")].required
    markers = tmp_path / "m.tsv"
    markers.write_text("g\t1\t5\t0.5\n")
    a = build_parser().parse_args(["get-transition-prob", "-i", str(markers)])
    assert (a.haplotypes, a.mating_scheme, a.gamma_scale, a.epsilon, a.output_file, a.verbose, a.device) == \
        ("A,B", "RI", 0.01, 0.000001, "tranprob.npz", 0, 0)
    assert a.marker_file == os.path.realpath(markers)
    a = build_parser().parse_args(["get-transition-prob", "-i", str(markers), "-s", "C,D", "-m", "F2", "-g", "0.5", "-e", "1e-3",
                                   "-o", "t.npz", "-vv", "--device", "1"])
    assert (a.haplotypes, a.mating_scheme, a.gamma_scale, a.epsilon, a.output_file, a.verbose, a.device) == \
        ("C,D", "F2", 0.5, 1e-3, "t.npz", 2, 1)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["get-transition-prob", "-i", str(tmp_path / "none.tsv")])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["get-transition-prob"])


def test_get_alignment_spec_flags_match_the_reference(tmp_path):
    """gbrs/commands.py:312-318"""
    from gbrs_amd.cli import build_parser
    f = flags_of(subparser("get-alignment-spec"))
    assert {("-i", "--sample-file"), ("-s", "--parental-strains"), ("-m", "--min-expr"), ("-v", "--verbose"),
            ("--device",)} <= set(f)
    assert f[("-i", "--sample-file")].required and f[("-s", "--parental-strains")].required
    samples = tmp_path / "s.tsv"
    samples.write_text("A\tx\n")
    a = build_parser().parse_args(["get-alignment-spec", "-i", str(samples), "-s", "A,B", "-s", "C"])
    assert (a.haplotypes, a.min_expr, a.verbose, a.device) == (["A,B", "C"], 2.0, 0, 0)
    a = build_parser().parse_args(["get-alignment-spec", "-i", str(samples), "-s", "A", "-m", "0.5"])
    assert a.min_expr == 0.5
    with pytest.raises(SystemExit):
        build_parser().parse_args(["get-alignment-spec", "-i", str(samples)])


def test_function_signatures():
    from gbrs_amd import hmm_inputs
    p = inspect.signature(hmm_inputs.get_transition_prob).parameters
    assert list(p)[:7] == ["marker_file", "haplotypes", "mating_scheme", "gamma_scale", "epsilon", "output_file", "device"]
    assert [p[k].default for k in list(p)[1:7]] == ["A,B", "RI", 0.01, 0.000001, "tranprob.npz", 0]
    assert p["marker_file"].default is inspect.Parameter.empty
    p = inspect.signature(hmm_inputs.get_alignment_spec).parameters
    assert list(p)[:4] == ["sample_file", "haplotypes", "min_expr", "device"]
    assert (p["min_expr"].default, p["device"].default) == (2.0, 0)
    assert p["sample_file"].default is inspect.Parameter.empty and p["haplotypes"].default is inspect.Parameter.empty


@pytest.mark.parametrize("kw, error, text", [
    (dict(haplotypes="A,B,C"), RuntimeError, "two haplotypes"),
    (dict(haplotypes="A"), RuntimeError, "two haplotypes"),
    (dict(mating_scheme="F2"), NotImplementedError, "F2"),
    (dict(mating_scheme="CC"), NotImplementedError, "CC"),
    (dict(mating_scheme="DO"), NotImplementedError, "DO"),
    (dict(mating_scheme="ri"), ValueError, "Unknown mating scheme: ri"),
])
def test_refusals_come_before_any_file(tmp_path, monkeypatch, kw, error, text):
    from gbrs_amd import hmm_inputs
    monkeypatch.setenv("GBRS_DATA", str(tmp_path / "data"))
    (tmp_path / "data").mkdir()
    markers = tmp_path / "m.tsv"
    markers.write_text("g0\t1\t5\t0.5\ng1\t1\t9\t0.75\n")
    with pytest.raises(error, match=text) as e:
        hmm_inputs.get_transition_prob(str(markers), output_file="out.npz", **kw)
    assert type(e.value) is error                                          # NotImplementedError is a RuntimeError
    assert os.listdir(tmp_path / "data") == []


@pytest.mark.parametrize("path", TRANPROB, ids=name_of)
def test_marker_parser(path):
    from gbrs_amd import hmm_inputs
    g = load_golden(path)
    locs, gpos = hmm_inputs.parse_marker_text(str(g["marker_text"]))
    want = hr.parse_markers(str(g["marker_text"]))
    assert list(locs) == list(gpos) == list(want)
    for c, (ids, pos, cm) in want.items():
        assert locs[c] == list(zip(ids, cm)) and gpos[c] == list(zip(ids, pos))
        assert np.array_equal(np.asanyarray(gpos[c]), hr.keyed(g, "gpos")[c].astype(str))   # what savez stores
    for bad, error in (("g\t1\tfive\t0.5\n", ValueError), ("g\t1\t5\thalf\n", ValueError), ("g\t1\t5\n", IndexError),
                       ("g\t1\t5.5\t0.5\n", ValueError), ("\n", IndexError)):
        with pytest.raises(error):
            hmm_inputs.parse_marker_text("a\t1\t1\t0.0\n" + bad)


@pytest.mark.parametrize("path", ALNSPEC, ids=name_of)
def test_sample_list_and_report_parsers(path, tmp_path, hip_lib):
    """The host side of get-alignment-spec on the fixture's texts: which files a strain lists, and the table every
    report contributes, through the library's number parser and line by line."""
    from gbrs_amd import hmm_inputs
    g = load_golden(path)
    sample_file, strains, min_expr, missing = hr.alnspec_write_inputs(g, tmp_path)
    flist = hmm_inputs.read_sample_list(open(sample_file).read())
    assert list(flist) == strains
    assert [p for st in strains for p in flist[st] if not os.path.isfile(p)] == missing
    genes = [str(k) for k in g["axes_keys"]]
    gid = {k: i for i, k in enumerate(genes)}
    S = len(strains)
    for p, text in hr.alnspec_reports(g, str(tmp_path)).items():
        want = np.zeros((len(genes), S))
        for line in text.splitlines()[1:]:
            item = line.split("\t")
            if item[0] in gid:
                want[gid[item[0]]] = [float(x) for x in item[1:S + 1]]
        assert np.array_equal(hmm_inputs.read_report_table(p, gid, len(genes), S), want)
        # a notes column makes the table not plain: the line-by-line reader gives the same numbers
        noted = tmp_path / "noted.tpm"
        noted.write_text("\n".join(line + "\tnote" for line in text.splitlines()) + "\n")
        assert np.array_equal(hmm_inputs.read_report_table(str(noted), gid, len(genes), S), want)
    with pytest.raises(IndexError):
        hmm_inputs.read_sample_list("A\tx\nB\n")


def test_no_cpu_fallback():
    """The library calls are the only route to numbers: the module holds no logarithm, square root or norm of its own,
    and without a device the calls fail instead of computing."""
    from gbrs_amd import _lib, hmm_inputs
    src = open(os.path.join(ROOT, "gbrs_amd", "hmm_inputs.py")).read()
    code = src.split('"""', 2)[2]
    for word in ("np.log", "np.sqrt", "linalg", "np.diff", "math.", "hmm_oracle", "restate"):
        assert word not in code, word
    assert "gbrs_ri_transition_tables" in code and "gbrs_alignment_spec" in code
    lib = _lib.load()
    if lib.gbrs_device_count() > 0:
        return
    with pytest.raises(_lib.GbrsHipError) as e:
        hmm_inputs.ri_transition_tables([np.array([0.0, 1.0, 2.5])], [False], 0.01, 1e-6)
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
    with pytest.raises(_lib.GbrsHipError) as e:
        hmm_inputs.alignment_spec_arrays(np.ones((1, 2, 2)), [0, 1, 1], [1, 1], 2, 2, 2.0)
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE


def test_commands_fail_loudly_without_a_device(tmp_path, monkeypatch, hip_lib):
    """Through cli.main the failure is logged and nothing is written (exit code 0, as every command here)."""
    if hip_lib.gbrs_device_count() > 0:
        return
    from gbrs_amd import cli
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    markers = tmp_path / "m.tsv"
    markers.write_text("g0\t1\t5\t0.5\ng1\t1\t9\t0.75\n")
    assert cli.main(["get-transition-prob", "-i", str(markers)]) == 0
    assert sorted(os.listdir(tmp_path)) == ["m.tsv"]
