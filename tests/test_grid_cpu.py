"""The host side of the grid pass (`gbrs reconstruct --grid-file`, `--sample-file`): knot preparation, the parser, the
sample file, and the composed oracle of tests/grid_cases.py against the reference's goldens.  No GPU."""
import os

import numpy as np
import pytest

import grid_cases
import small_ops_cases as cases
from conftest import GOLD, hmm_case_inputs, load_golden


@pytest.mark.parametrize("name", list(cases.interp_positions()))
def test_knots_equal_the_oracles(name, hip_lib):
    """Sorted input: the knots are [0, genes..., last grid point + 1] as oracle.postproc_oracle.interpolate builds them,
    the two end knots carry the first and the last gene."""
    from gbrs_amd.hmm import grid_knots
    x_gene, x_grid = cases.interp_positions()[name]
    knots, gene = grid_knots(x_gene, x_grid)
    expected = np.append(np.append([0.0], np.asarray(x_gene, dtype=float)), [x_grid[-1] + 1.0])    # postproc_oracle.py:18-19
    np.testing.assert_array_equal(knots, expected)
    np.testing.assert_array_equal(gene, np.clip(np.arange(len(x_gene) + 2) - 1, 0, len(x_gene) - 1))


@pytest.mark.parametrize("x_gene,x_grid", [
    (np.array([1.0, 2.0, 50.0]), np.array([0.5, 3.0])),                   # a gene beyond the last grid point + 1
    (np.array([1.0, 5.0, 3.0, 4.0]), np.array([0.5, 9.0])),               # two genes out of order
    (np.array([4.0, 4.0, 1.0, 4.0, 10.0]), np.array([2.0, 4.0, 3.0])),    # ties keep their order; the grid's last point counts
], ids=["gene_past_the_grid", "out_of_order", "ties"])
def test_knots_of_unsorted_input_are_a_stable_argsort(x_gene, x_grid, hip_lib):
    from gbrs_amd.hmm import grid_knots
    knots, gene = grid_knots(x_gene, x_grid)
    raw = np.concatenate(([0.0], x_gene, [x_grid[-1] + 1.0]))
    order = np.argsort(raw, kind="stable")
    assert (np.diff(order) < 0).any()
    np.testing.assert_array_equal(knots, raw[order])
    np.testing.assert_array_equal(gene, np.clip(order - 1, 0, len(x_gene) - 1))


def test_knots_range_errors(hip_lib):
    from gbrs_amd.hmm import grid_knots
    x_gene = np.array([1.0, 2.0, 5.0])
    with pytest.raises(ValueError, match="below the interpolation range's minimum value"):
        grid_knots(x_gene, np.array([-1e-300, 2.0]))
    with pytest.raises(ValueError, match="above the interpolation range's maximum value"):
        grid_knots(x_gene, np.array([9.0, 3.0]))                            # the last knot is max(5, 3 + 1)
    with pytest.raises(IndexError):
        grid_knots(np.zeros(0), np.array([1.0]))                            # a grid chromosome without genes
    knots, _ = grid_knots(x_gene, np.array([6.0, 7.0, 9.0]))
    assert knots[-1] == 10.0


def test_parser_grid_and_sample_options(tmp_path):
    from gbrs_amd import cli
    f = tmp_path / "file"
    f.write_text("x\n")
    ap = cli.build_parser()
    base = ["reconstruct", "-t", str(f)]
    a = ap.parse_args(base + ["-e", str(f), "--grid-file", str(f), "--grid-genoprobs", "-g", str(f)])
    assert a.grid_file == os.path.realpath(f) and a.grid_genoprobs and a.gpos_file == os.path.realpath(f)
    assert a.sample_file is None
    a = ap.parse_args(base + ["-e", str(f)])
    assert a.grid_file is None and not a.grid_genoprobs and a.batch_size == 64
    a = ap.parse_args(base + ["--sample-file", str(f), "--batch-size", "7"])
    assert a.sample_file == os.path.realpath(f) and a.expression_file is None and a.batch_size == 7
    for bad in (base, base + ["-e", str(f), "--sample-file", str(f)]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_sample_file_lines(tmp_path):
    from gbrs_amd.hmm import read_sample_file
    f = tmp_path / "samples.txt"
    f.write_text("# cohort\n\na.genes.tpm\tout/a\n   \n#b.genes.tpm\tout/b\nc.genes.tpm\tout/c\n")
    assert read_sample_file(str(f)) == [("a.genes.tpm", "out/a"), ("c.genes.tpm", "out/c")]
    f.write_text("a.genes.tpm out/a\n")
    with pytest.raises(RuntimeError, match="line 1"):
        read_sample_file(str(f))


@pytest.mark.parametrize("name", ["h8", "h4"])
def test_composed_oracle_reproduces_the_reference(name):
    """grid_cases.expected on the inputs of the HMM golden that tests/golden/postproc_<name>.npz was made from gives that
    file's grid probabilities and dosages.  The golden's posteriors are the reference's and the oracle's are within 1e-10
    of them (tests/test_oracle_golden.py); an interpolated value is a convex combination of two of them, which keeps the
    relative error, plus four roundings of values in [0, 1]; a dosage adds at most S of those."""
    from gbrs_amd.synth import HmmProblem
    post = load_golden(os.path.join(GOLD, f"postproc_{name}.npz"))
    g = load_golden(os.path.join(GOLD, f"hmm_{name}_full.npz"))
    c = hmm_case_inputs(g)
    chroms = [str(x) for x in post["chroms"]]
    assert chroms == c["chroms"]
    H = c["H"]
    S = H * (H + 1) // 2
    expr = {str(gid): row for ch in chroms for gid, row in zip(c["genes"][ch], c["expr"][ch])}
    avecs = {str(gid): a for ch in chroms for gid, has, a in zip(c["genes"][ch], c["has_avec"][ch], c["avecs"][ch]) if has}
    p = HmmProblem([chr(65 + h) for h in range(H)], chroms, {ch: [str(x) for x in c["genes"][ch]] for ch in chroms},
                   c["tprob"], expr, avecs)
    grid = grid_cases.Grid({ch: post[f"xgene_{ch}"] for ch in chroms}, {ch: post[f"grid_{ch}"] for ch in chroms})
    on_grid, dosage = grid_cases.expected(p, grid)
    assert list(on_grid) == chroms
    for ch in chroms:
        np.testing.assert_allclose(on_grid[ch], post[f"interp_{ch}"], rtol=1e-10, atol=4 * 2.0 ** -53)
    np.testing.assert_allclose(dosage, post["dosage"], rtol=1e-10, atol=2 * S * 2.0 ** -53)


def test_grids_of_the_table_cover_what_they_claim():
    """The shapes the GPU tests rely on, checked where it is cheap."""
    grids = grid_cases.grids()
    w = grid_cases.gene_positions()
    assert sorted(len(x) for x in grids["a"].points.values()) == [1, 63, 64, 65] and "X" not in grids["a"].points
    assert sorted(len(x) for x in grids["b"].points.values()) == [1, 63, 65, 130] and "1" not in grids["b"].points
    for name in ("a", "b"):
        for c, x in grids[name].points.items():
            assert (np.diff(w[c]) >= 0).all() and x[-1] + 1.0 >= w[c][-1], (name, c)       # knots need no sorting
    a = grids["a"].points
    assert a["2"][0] == 0.0 and (a["2"] < w["2"][0]).sum() >= 2 and (a["2"] > w["2"][-1]).any()
    assert w["3"][1] == w["3"][2] and w["3"][1] in a["3"] and w["4"][10] == w["4"][12] and w["4"][10] in a["4"]
    assert np.isin(w["X"][[0, 100, 150]], grids["b"].points["X"]).all()
    u = grids["unsorted"]
    assert (np.diff(u.positions["3"]) < 0).any() and u.positions["4"][-1] > u.points["4"][-1] + 1.0


def test_dosage_table_is_savetxts_text(tmp_path):
    """`<outbase>.interpolated.genoprobs.tsv` is written by one format operation; the bytes are np.savetxt's, which is how
    `gbrs export` writes its table."""
    from gbrs_amd.hmm import write_dosage_table
    rng = np.random.default_rng(11)
    rows = rng.random((700, 8))
    rows[0] = [0.0, 1.0, 0.5, 0.9999995, 0.0000005, 1e-300, 0.1234565, 2.0 ** -53]
    rows[1, 0] = -1e-19
    names = list("ABCDEFGH")
    write_dosage_table(tmp_path / "mine.tsv", rows, names)
    np.savetxt(tmp_path / "numpy.tsv", rows, fmt="%.6f", delimiter="\t", header="\t".join(names))
    assert open(tmp_path / "mine.tsv", "rb").read() == open(tmp_path / "numpy.tsv", "rb").read()
    write_dosage_table(tmp_path / "empty.tsv", np.zeros((0, 3)), list("ABC"))
    np.savetxt(tmp_path / "empty_numpy.tsv", np.zeros((0, 3)), fmt="%.6f", delimiter="\t", header="A\tB\tC")
    assert open(tmp_path / "empty.tsv", "rb").read() == open(tmp_path / "empty_numpy.tsv", "rb").read()
