"""The host side of `gbrs reconstruct --match-panel`: the options and their refusals, the panel and label
readers, match_scores, rank_matches and the writers.  No GPU; the device's sums are tests/test_match_gpu.py's."""
import types

import numpy as np
import pytest

import grid_cases
import match_cases as cases
from gbrs_amd import cli
from gbrs_amd import hmm as H


# ---- options ---------------------------------------------------------------------------------------------------------------

def parse(tmp_path, *more):
    for name in ("t.npz", "e.tpm", "s.txt", "g.txt", "p.txt", "l.txt"):
        (tmp_path / name).write_text("")
    argv = ["reconstruct", "-t", str(tmp_path / "t.npz")] + [str(tmp_path / x) if x.endswith(".txt") or x.endswith(".tpm") else x
                                                            for x in more]
    return cli.build_parser().parse_args(argv)


def check(args):
    H.check_match_args(args.match_panel, args.match_labels, args.match_expected, args.match_chromosomes, args.match_report,
                       args.match_matrix, args.grid_file, cohort=args.sample_file is not None)


def test_parser_flags(tmp_path):
    a = parse(tmp_path, "--sample-file", "s.txt", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-labels", "l.txt",
              "--match-chromosomes", "1,2", "--match-report", "r.tsv", "--match-matrix", "m.npz")
    assert a.match_panel.endswith("p.txt") and a.match_labels.endswith("l.txt") and a.match_chromosomes == "1,2"
    assert a.match_report == "r.tsv" and a.match_matrix == "m.npz" and a.match_expected is None
    check(a)
    b = parse(tmp_path, "-e", "e.tpm", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-expected", "animal3")
    assert b.match_expected == "animal3"
    check(b)
    plain = parse(tmp_path, "-e", "e.tpm")
    assert plain.match_panel is None
    check(plain)
    with pytest.raises(SystemExit):
        parse(tmp_path, "-e", "e.tpm", "--match-panel", "missing_panel_file")


@pytest.mark.parametrize("more,text", [
    (("-e", "e.tpm", "--match-panel", "p.txt"), "--match-panel needs --grid-file"),
    (("--sample-file", "s.txt", "--match-panel", "p.txt"), "--match-panel needs --grid-file"),
    (("-e", "e.tpm", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-labels", "l.txt"), "--match-labels needs --sample-file"),
    (("--sample-file", "s.txt", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-expected", "x"), "--match-expected belongs to -e"),
    (("-e", "e.tpm", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-report", "r.tsv"), "--match-report needs --sample-file"),
    (("-e", "e.tpm", "--grid-file", "g.txt", "--match-panel", "p.txt", "--match-matrix", "m.npz"), "--match-matrix needs --sample-file"),
    (("-e", "e.tpm", "--grid-file", "g.txt", "--match-expected", "x"), "--match-expected needs --match-panel"),
    (("-e", "e.tpm", "--grid-file", "g.txt", "--match-chromosomes", "1"), "--match-chromosomes needs --match-panel"),
    (("--sample-file", "s.txt", "--grid-file", "g.txt", "--match-report", "r.tsv"), "--match-report needs --match-panel"),
])
def test_refusals(tmp_path, caplog, more, text):
    args = parse(tmp_path, *more)
    with pytest.raises(RuntimeError, match=text):
        check(args)
    # the command refuses before it reads a file: the files here are empty, and the only error is the refusal
    argv = ["reconstruct", "-t", str(tmp_path / "t.npz")] + [str(tmp_path / x) if x.endswith((".txt", ".tpm")) else x for x in more]
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(argv) == 0
    errors = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(errors) == 1 and text in errors[0]


# ---- readers ---------------------------------------------------------------------------------------------------------------

HAPS = ["A", "B", "C"]


def context():
    """What the readers use of a ReconstructContext: handle chromosomes 1, 2, 3, X; the grid file lists X, then 2, then 1."""
    grid = {"X": np.arange(3.0), "2": np.arange(2.0), "1": np.arange(4.0)}
    return types.SimpleNamespace(chroms=["1", "2", "3", "X"], grid=grid, grid_slices={})


def table(seed, rows=9):
    return np.random.default_rng(seed).dirichlet(np.ones(len(HAPS)), size=rows)


def test_panel_reader(tmp_path):
    tables = [table(1), table(2)]
    path = cases.write_panel(tmp_path, ["m1", "m2"], tables, HAPS)
    assert open(path).read().startswith("# id\tpath\n\n")          # a comment and a blank line
    ctx = context()
    assert H.grid_layout(ctx) == {"1": (0, 0, 4), "2": (1, 4, 2), "X": (3, 6, 3)}
    ids, arrays = H.read_match_panel(path, ctx, HAPS)
    assert ids == ["m1", "m2"] and len(arrays) == 2
    for got, t in zip(arrays, tables):
        want = cases.rounded(t)
        # grid file order X (rows 0-2), 2 (3-4), 1 (5-8) -> handle order 1, 2, X
        np.testing.assert_array_equal(got, np.concatenate([want[5:9], want[3:5], want[0:3]]))
        assert got.flags.c_contiguous and got.dtype == np.float64


def test_panel_reader_refusals(tmp_path):
    ctx = context()
    good = cases.write_dosage_table(tmp_path / "good.tsv", table(1), HAPS)

    def panel(text):
        (tmp_path / "p.txt").write_text(text)
        return str(tmp_path / "p.txt")

    with pytest.raises(RuntimeError, match=r"line 3: panel id m1 is already on line 1"):
        H.read_match_panel(panel(f"m1\t{good}\n#\nm1\t{good}\n"), ctx, HAPS)
    with pytest.raises(RuntimeError, match="expected id<TAB>path"):
        H.read_match_panel(panel(f"m1 {good}\n"), ctx, HAPS)
    with pytest.raises(RuntimeError, match="no panel entries"):
        H.read_match_panel(panel("# nothing\n\n"), ctx, HAPS)
    with pytest.raises(RuntimeError, match="does not exist"):
        H.read_match_panel(panel(f"m1\t{tmp_path / 'absent.tsv'}\n"), ctx, HAPS)
    other = cases.write_dosage_table(tmp_path / "other.tsv", table(1), ["A", "B", "Z"])
    with pytest.raises(RuntimeError, match="other.tsv.*haplotypes"):
        H.read_match_panel(panel(f"m1\t{other}\n"), ctx, HAPS)
    short = cases.write_dosage_table(tmp_path / "short.tsv", table(1, rows=8), HAPS)
    with pytest.raises(RuntimeError, match="short.tsv: 8 rows for the 9 grid points"):
        H.read_match_panel(panel(f"m1\t{short}\n"), ctx, HAPS)
    rows = open(good).read().splitlines()
    rows[1] += "\t0.5"
    (tmp_path / "wide.tsv").write_text("\n".join(rows) + "\n")
    with pytest.raises(RuntimeError, match="wide.tsv, line 2: 4 columns for 3 haplotypes"):
        H.read_match_panel(panel(f"m1\t{tmp_path / 'wide.tsv'}\n"), ctx, HAPS)
    (tmp_path / "word.tsv").write_text(open(good).read().replace("0.", "x.", 1))
    with pytest.raises(RuntimeError, match="word.tsv"):
        H.read_match_panel(panel(f"m1\t{tmp_path / 'word.tsv'}\n"), ctx, HAPS)
    # a grid chromosome that is not on the handle: the error `--grid-file` alone raises only after the run
    ctx.grid["Z"] = np.arange(2.0)
    with pytest.raises(KeyError, match="Z"):
        H.read_match_panel(panel(f"m1\t{good}\n"), ctx, HAPS)


def test_label_reader(tmp_path):
    (tmp_path / "l.txt").write_text("# outbase\tid\n\nout/a\tm1\nout/b\tm7\n")
    assert H.read_match_labels(str(tmp_path / "l.txt")) == {"out/a": "m1", "out/b": "m7"}
    (tmp_path / "l.txt").write_text("out/a\tm1\nout/a\tm2\n")
    with pytest.raises(RuntimeError, match="line 2: outbase out/a is already on line 1"):
        H.read_match_labels(str(tmp_path / "l.txt"))
    (tmp_path / "l.txt").write_text("out/a\n")
    with pytest.raises(RuntimeError, match="expected outbase<TAB>panel id"):
        H.read_match_labels(str(tmp_path / "l.txt"))
    with pytest.raises(OSError):
        H.read_match_labels(str(tmp_path / "absent.txt"))


def test_chromosome_mask():
    chroms, points = ["1", "2", "3", "X"], [4, 2, 0, 3]
    assert H.match_chromosome_mask(chroms, points).tolist() == [True, True, False, True]
    assert H.match_chromosome_mask(chroms, points, "1,2").tolist() == [True, True, False, False]
    assert H.match_chromosome_mask(chroms, points, ["X", "3"]).tolist() == [False, False, False, True]
    with pytest.raises(RuntimeError, match="Y is not a chromosome"):
        H.match_chromosome_mask(chroms, points, "1,Y")
    with pytest.raises(RuntimeError, match="no grid points"):
        H.match_chromosome_mask(chroms, points, "3")
    with pytest.raises(RuntimeError, match="no grid points"):
        H.match_chromosome_mask(chroms, [0, 0, 0, 0])


# ---- scores ----------------------------------------------------------------------------------------------------------------

def small():
    rng = np.random.default_rng(5)
    points, offsets = [4, 2, 0, 3], [0, 4, 6, 6]
    a = rng.dirichlet(np.ones(3), size=(5, 9))
    panel = cases.random_panel(rng, 6, 9, 3)
    return a, panel, points, offsets


def test_match_scores_against_the_direct_difference():
    a, panel, points, offsets = small()
    cross, snorm, pnorm = cases.restate(a, panel, points, offsets)
    use = np.array([True, True, False, True])
    distance, similarity = H.match_scores(cross, snorm, pnorm, points, use)
    assert distance.shape == similarity.shape == (5, 6)
    b = np.stack(panel)
    direct = ((a[:, None] - b[None]) ** 2).sum(axis=(2, 3)) / 9
    np.testing.assert_allclose(distance, direct, rtol=1e-12, atol=0)
    cosine = (a[:, None] * b[None]).sum(axis=(2, 3)) / np.sqrt((a ** 2).sum(axis=(1, 2))[:, None] * (b ** 2).sum(axis=(1, 2))[None])
    np.testing.assert_allclose(similarity, cosine, rtol=1e-12, atol=0)
    assert (distance >= 0).all() and (distance <= 2).all()
    # one sample's arrays, without the leading axis
    d0, s0 = H.match_scores(cross[2], snorm[2], pnorm, points, use)
    np.testing.assert_array_equal(d0, distance[2])
    np.testing.assert_array_equal(s0, similarity[2])
    # the mask: chromosomes "2" and "X" alone
    use = np.array([False, True, False, True])
    distance, _ = H.match_scores(cross, snorm, pnorm, points, use)
    rows = np.r_[4:6, 6:9]
    np.testing.assert_allclose(distance, ((a[:, None, rows] - b[None, :, rows]) ** 2).sum(axis=(2, 3)) / 5, rtol=1e-12, atol=0)


def test_match_scores_adds_the_chromosomes_left_to_right():
    """Three chromosomes whose sums do not associate: (1 + 2^-53) + 2^-53 is 1.0 twice rounded, 1 + (2^-53 + 2^-53) is not."""
    tiny = 2.0 ** -53
    cross = np.array([[1.0], [tiny], [tiny]])
    snorm = np.array([1.0, tiny, tiny])
    pnorm = np.array([[4.0, 0.0, 0.0]])
    _, similarity = H.match_scores(cross, snorm, pnorm, [1, 1, 1], [True, True, True])
    assert similarity[0] == ((1.0 + tiny) + tiny) / np.sqrt(((1.0 + tiny) + tiny) * 4.0) == 0.5
    assert (1.0 + (tiny + tiny)) != 1.0
    distance, _ = H.match_scores(cross, snorm, pnorm, [1, 1, 1], [True, True, True])
    assert distance[0] == (1.0 + 4.0 - 2.0) / 3


def test_match_scores_edges():
    # the clamp: rounding can leave A + B - 2 X a little below zero for identical rows
    cross = np.array([[np.nextafter(1.0, 2.0)]])
    distance, similarity = H.match_scores(cross, np.array([1.0]), np.array([[1.0]]), [7], [True])
    assert distance[0] == 0.0 and similarity[0] > 1.0 - 1e-15
    # a zero norm: similarity 0.0, distance the other norm over n
    distance, similarity = H.match_scores(np.zeros((1, 2)), np.array([0.0]), np.array([[0.0], [3.0]]), [2], [True])
    assert similarity.tolist() == [0.0, 0.0] and distance.tolist() == [0.0, 1.5]
    with pytest.raises(RuntimeError, match="no grid points"):
        H.match_scores(np.zeros((2, 1)), np.zeros(2), np.zeros((1, 2)), [0, 5], [True, False])
    with pytest.raises(RuntimeError, match="no grid points"):
        H.match_scores(np.zeros((2, 1)), np.zeros(2), np.zeros((1, 2)), [3, 5], [False, False])


def test_rank_matches():
    ids = ["m0", "m1", "m2", "m3"]
    r = H.rank_matches(ids, [0.25, 0.125, 0.125, 0.5], "m1")
    assert r["order"].tolist() == [1, 2, 0, 3]                      # the tie keeps panel order
    assert (r["best"], r["second"], r["margin"], r["status"]) == ("m1", "m2", 0.0, "match")
    assert (r["expected"], r["expected_distance"], r["expected_rank"]) == ("m1", 0.125, 1)
    r = H.rank_matches(ids, [0.25, 0.125, 0.125, 0.5], "m2")
    assert (r["best"], r["status"], r["expected_rank"], r["expected_distance"]) == ("m1", "mismatch", 2, 0.125)
    r = H.rank_matches(ids, [0.25, 0.125, 0.0625, 0.5], "m3")
    assert (r["best"], r["second"], r["margin"], r["status"], r["expected_rank"]) == ("m2", "m1", 0.0625, "mismatch", 4)
    r = H.rank_matches(ids, [0.25, 0.125, 0.0625, 0.5])
    assert (r["status"], r["expected"], r["expected_rank"]) == ("unlabelled", "", 0) and np.isnan(r["expected_distance"])
    r = H.rank_matches(ids, [0.25, 0.125, 0.0625, 0.5], "m9")
    assert (r["status"], r["expected"], r["expected_rank"]) == ("unknown-label", "m9", 0) and np.isnan(r["expected_distance"])
    one = H.rank_matches(["only"], [0.5], "only")
    assert (one["best"], one["second"], one["status"], one["order"].tolist()) == ("only", "", "match", [0])
    assert np.isnan(one["second_distance"]) and np.isnan(one["margin"])


def test_writers(tmp_path):
    ids = ["m0", "m1", "m2"]
    distance, similarity = np.array([0.25, 1.0 / 3.0, 0.0]), np.array([0.5, 0.1, 1.0])
    r = H.rank_matches(ids, distance, "m0")
    H.write_match_table(str(tmp_path / "s.match.tsv"), ids, distance, similarity, r["order"])
    assert open(tmp_path / "s.match.tsv").read() == ("#panel_id\tdistance\tsimilarity\n"
                                                     "m2\t0.0\t1.0\n"
                                                     "m0\t0.25\t0.5\n"
                                                     "m1\t0.3333333333333333\t0.1\n")
    lines = [("out/a", r), ("out/b", H.rank_matches(ids, distance)), ("out/c", H.rank_matches(["m0"], [0.5], "zz"))]
    H.write_match_report(str(tmp_path / "report.tsv"), lines)
    assert open(tmp_path / "report.tsv").read() == (
        "#outbase\texpected\tstatus\tbest\tbest_distance\tsecond\tsecond_distance\tmargin\texpected_distance\texpected_rank\n"
        "out/a\tm0\tmismatch\tm2\t0.0\tm0\t0.25\t0.25\t0.25\t2\n"
        "out/b\t\tunlabelled\tm2\t0.0\tm0\t0.25\t0.25\tnan\t0\n"
        "out/c\tzz\tunknown-label\tm0\t0.5\t\tnan\tnan\tnan\t0\n")
    H.write_match_matrix(str(tmp_path / "m.npz"), ["out/a"], ids, ["1", "X"], [4, 0], distance[None], similarity[None],
                         np.ones((1, 2, 3)), np.ones((1, 2)), np.ones((3, 2)))
    z = np.load(tmp_path / "m.npz")
    assert sorted(z.files) == sorted(["distance", "similarity", "cross", "sample_norm", "panel_norm", "outbases", "panel_ids",
                                      "chromosomes", "points"])
    assert z["panel_ids"].tolist() == ids and z["chromosomes"].tolist() == ["1", "X"] and z["points"].tolist() == [4, 0]
    np.testing.assert_array_equal(z["distance"], distance[None])


def test_the_planted_cohort_is_separated_by_the_oracle():
    """The seed tests/test_match_gpu.py uses: the composed oracle's dosages put every sample's own entry first, at least
    twice the asserted margin ahead of the next."""
    seed = cases.planted_seed()
    p0 = grid_cases.problem(cases.PLANTED_H, cases.PLANTED_STYLE)
    grid = grid_cases.grids()[cases.PLANTED_GRID]
    points, offsets = cases.handle_points(p0.chroms, grid)
    own = np.stack([cases.to_handle_order(grid_cases.expected_for(cases.PLANTED_H, cases.PLANTED_STYLE, s, cases.PLANTED_GRID)[1],
                                          p0.chroms, grid) for s in range(cases.PLANTED_SAMPLES)])
    ids, arrays, where = cases.planted_panel(own, seed)
    best, margin, distance = cases.margins(own, arrays, points, offsets)
    assert best == where and min(margin) >= 2 * cases.PLANTED_MARGIN
    assert max(distance[s, where[s]] for s in range(len(where))) < cases.PLANTED_H * 0.5e-6 ** 2 * 4
    print(f"seed {seed}, margins {np.round(margin, 4).tolist()}")
