"""The rule of the imputation pass and its host side, without a GPU: tests/impute_cases.py's restatement
against the composed oracle on the oracle's posteriors, the SNP file reader, the argument checks and the parser."""
import logging

import numpy as np
import pytest

import grid_cases
import impute_cases

CASES = [(H, "benign") for H in (1, 2, 3, 8, 16)] + [(8, "do")]


def reassociation_atol(H):
    """Founders first and interpolation second against the 36-state interpolation first: both orders round at most
    2 S + H + 6 times on terms of magnitude <= 1, doubled by the final factor: 8 (S + H + 8) 2^-53."""
    S = H * (H + 1) // 2
    return 8 * (S + H + 8) * 2.0 ** -53


@pytest.mark.parametrize("H,style", CASES)
def test_restatement_equals_the_composed_oracle(H, style):
    p = grid_cases.sample_problem(H, style, 0)
    res = grid_cases.oracle_arrays(H, style, 0)[0]
    for name, snps in impute_cases.snp_sets().items():
        masks = impute_cases.masks_for(name, H)
        got = impute_cases.impute(list(snps.points), snps, masks, lambda c: res[c]["gamma"], H)
        want = impute_cases.composed(p, snps, masks, res, sorted_knots=name in impute_cases.NEEDS_SORTED_KNOTS)
        assert got.shape == want.shape == (sum(len(x) for x in snps.points.values()),)
        print(f"DEVIATION restatement against the composed oracle, H={H} {style} set {name}: "
              f"{np.abs(got - want).max():.3g} (bound {reassociation_atol(H):.3g})")
        np.testing.assert_allclose(got, want, rtol=0, atol=reassociation_atol(H), err_msg=f"set {name}")
        assert got.min() >= -reassociation_atol(H) and got.max() <= 2.0 + reassociation_atol(H)


@pytest.mark.parametrize("H", (1, 3, 8))
def test_zero_and_one_hot_patterns(H):
    """The all-zeros pattern gives exactly 0.0; a one-hot pattern gives 2 x the founder's dosage interpolated, the same
    bits (one term, added to +0.0); all ones gives 2 x the interpolated row sum."""
    res = grid_cases.oracle_arrays(H, "benign", 0)[0]
    snps = impute_cases.snp_sets()["b"]
    for c, x in snps.points.items():
        gamma = res[c]["gamma"]
        D = impute_cases.gene_dosage(gamma, H)
        zero = impute_cases.impute_chromosome(snps.positions[c], gamma, x, np.zeros(len(x), dtype=np.uint32), H)
        assert (zero == 0.0).all() and not np.signbit(zero).any()
        knots, knot_gene = impute_cases.knots_of(snps.positions[c], x)
        idx = np.clip(np.searchsorted(knots, x, side="left"), 1, len(knots) - 1)
        for h in range(H):
            one = impute_cases.impute_chromosome(snps.positions[c], gamma, x, np.full(len(x), 1 << h, dtype=np.uint32), H)
            d_lo, d_hi = D[knot_gene[idx - 1], h], D[knot_gene[idx], h]
            want = 2.0 * ((d_hi - d_lo) / (knots[idx] - knots[idx - 1]) * (x - knots[idx - 1]) + d_lo)
            np.testing.assert_array_equal(one, want)
        ones = impute_cases.impute_chromosome(snps.positions[c], gamma, x, np.full(len(x), (1 << H) - 1, dtype=np.uint32), H)
        np.testing.assert_allclose(ones, 2.0, rtol=0, atol=reassociation_atol(H))


def test_the_sets_hold_what_they_promise():
    sets = impute_cases.snp_sets()
    for count in (255, 256, 257):
        x = sets[f"n{count}"].points["X"]
        assert len(x) == count and x[100] == x[101]
        m = impute_cases.masks_for(f"n{count}", 8)["X"]
        assert m[100] != m[101]
    d = sets["descending"].points
    assert all((np.diff(x) < 0).all() for x in d.values())
    for H in (2, 8):
        every = np.concatenate([np.concatenate(list(impute_cases.masks_for(n, H).values())) for n in sets])
        assert {0, (1 << H) - 1} | {1 << h for h in range(H)} <= set(every.tolist())
        assert every.max() < 1 << H


# ---- read_snp_file ----------------------------------------------------------------------------------------------------------

HAPS = list("ABCDEFGH")


def write_lines(path, lines):
    with open(path, "w") as fh:
        fh.write("id\tchr\tbp\tcM\tpattern\n")
        fh.writelines(line + "\n" for line in lines)
    return str(path)


def test_read_snp_file_good(tmp_path):
    from gbrs_amd.hmm import read_snp_file, snp_dosage_in_file_order
    path = write_lines(tmp_path / "snps.tsv", [
        "rs1\t2\t1000\t1.5\t10000000",
        "rs2\t1\t2000\t0.25\t00000001",
        "rs3\t2\t500\t0.75\t11111111",
        "rs4\t1\tNA\t3.0\t00000000\tan extra column",
        "rs5\t2\t\t1.5\t01010101",
    ])
    s = read_snp_file(path, HAPS, ["1", "2", "X"])
    assert s["snp_id"].tolist() == ["rs1", "rs2", "rs3", "rs4", "rs5"]
    assert s["chrom"].tolist() == ["2", "1", "2", "1", "2"]
    np.testing.assert_array_equal(s["cM"], [1.5, 0.25, 0.75, 3.0, 1.5])
    np.testing.assert_array_equal(s["bp"], [1000.0, 2000.0, 500.0, np.nan, np.nan])
    assert s["mask"].dtype == np.uint32 and s["mask"].tolist() == [1, 128, 255, 0, 0b10101010]
    assert s["pattern"].tolist()[4] == "01010101"
    assert {c: v.tolist() for c, v in s["by_chrom"].items()} == {"1": [1, 3], "2": [0, 2, 4], "X": []}
    assert s["order"].tolist() == [1, 3, 0, 2, 4] and s["foreign"] == 0
    back = snp_dosage_in_file_order(s, np.array([[10.0, 11.0, 12.0, 13.0, 14.0]]))
    np.testing.assert_array_equal(back, [[12.0, 10.0, 13.0, 11.0, 14.0]])


@pytest.mark.parametrize("line,reason", [
    ("rs9\t1\t100\t1.0", "columns"),
    ("rs9\t1\t100\t1.0\t1010101", "7 characters for 8 haplotypes"),
    ("rs9\t1\t100\t1.0\t101010101", "9 characters for 8 haplotypes"),
    ("rs9\t1\t100\t1.0\t1010101A", "other than 0 and 1"),
    ("rs9\t1\t100\t1.0\t1010101 ", "other than 0 and 1"),
    ("rs9\t1\t100\tabc\t10101010", "not a number"),
    ("rs9\t1\tabc\t1.0\t10101010", "not a number"),
])
def test_read_snp_file_refuses_a_line_by_number(tmp_path, line, reason):
    from gbrs_amd.hmm import read_snp_file
    path = write_lines(tmp_path / "snps.tsv", ["rs1\t1\t100\t1.0\t10000000", "rs2\t1\t200\t2.0\t01000000", line])
    with pytest.raises(ValueError, match=f"line 4: .*{reason}"):
        read_snp_file(path, HAPS, ["1"])


def test_read_snp_file_fills_positions_from_the_grid_file(tmp_path):
    from gbrs_amd.hmm import read_snp_file
    grid = tmp_path / "grid.txt"
    with open(grid, "w") as fh:
        fh.write("marker\tchr\tbp\tcM\n")
        fh.write("m0\t1\t3000000\t1.75\nm1\t1\t1000000\t0.5\nm2\t2\t500\t9.0\nm3\t1\t2000000\t1.25\nm4\t2\t100\t4.0\n")
    path = write_lines(tmp_path / "snps.tsv", [
        "rs1\t1\t1500000\tNA\t10000000",
        "rs2\t1\t2500000\t\t10000000",
        "rs3\t1\t10\tNA\t10000000",            # before the first grid row: clamped
        "rs4\t1\t9000000\tNA\t10000000",       # behind the last
        "rs5\t2\t300\tNA\t10000000",
        "rs6\t2\t300\t7.0\t10000000",          # a given position stays
    ])
    s = read_snp_file(path, HAPS, ["1", "2"], grid_file=str(grid))
    bp1, cm1 = np.array([1e6, 2e6, 3e6]), np.array([0.5, 1.25, 1.75])
    want = list(np.interp([1.5e6, 2.5e6, 10.0, 9e6], bp1, cm1)) + [float(np.interp(300.0, [100.0, 500.0], [4.0, 9.0])), 7.0]
    np.testing.assert_array_equal(s["cM"], want)
    with pytest.raises(ValueError, match="line 2: .*--grid-file"):
        read_snp_file(path, HAPS, ["1", "2"])
    other = write_lines(tmp_path / "other.tsv", ["rs1\t1\t100\t1.0\t10000000", "rs2\t7\t100\tNA\t10000000"])
    with pytest.raises(ValueError, match="line 3: .*chromosome 7"):
        read_snp_file(other, HAPS, ["1"], grid_file=str(grid))
    neither = write_lines(tmp_path / "neither.tsv", ["rs1\t1\tNA\tNA\t10000000"])
    with pytest.raises(ValueError, match="line 2: "):
        read_snp_file(neither, HAPS, ["1"], grid_file=str(grid))


def test_read_snp_file_foreign_chromosomes(tmp_path, caplog):
    from gbrs_amd.hmm import read_snp_file, snp_dosage_in_file_order
    path = write_lines(tmp_path / "snps.tsv", [
        "rs1\tMT\t100\t1.0\t10000000",
        "rs2\t1\t100\t1.0\t10000000",
        "rs3\tY\t100\t1.0\t10000000",
        "rs4\t1\t100\t2.0\t01000000",
    ])
    with caplog.at_level(logging.WARNING, logger="gbrs"):
        s = read_snp_file(path, HAPS, ["1", "2"])
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "2 SNPs" in warnings[0].getMessage()
    assert s["foreign"] == 2 and s["order"].tolist() == [1, 3]
    out = snp_dosage_in_file_order(s, np.array([0.5, 1.5]))
    np.testing.assert_array_equal(out, [np.nan, 0.5, np.nan, 1.5])


# ---- arguments ------------------------------------------------------------------------------------------------------------

def test_check_snp_args():
    from gbrs_amd.hmm import check_snp_args
    check_snp_args()
    check_snp_args("snps.tsv", None, cohort=False)
    check_snp_args("snps.tsv", None, cohort=True)
    check_snp_args("snps.tsv", "all.npz", cohort=True)
    with pytest.raises(RuntimeError, match="--snp-matrix needs --snp-file"):
        check_snp_args(None, "all.npz", cohort=True)
    with pytest.raises(RuntimeError, match="--snp-matrix needs --sample-file"):
        check_snp_args("snps.tsv", "all.npz", cohort=False)


def test_the_parser_knows_the_flags(tmp_path, capsys, caplog):
    from gbrs_amd import cli
    for name in ("snps.tsv", "t.npz", "s.tpm"):
        (tmp_path / name).write_text("x\n")
    args = cli.build_parser().parse_args(["reconstruct", "-e", str(tmp_path / "s.tpm"), "-t", str(tmp_path / "t.npz"),
                                          "--snp-file", str(tmp_path / "snps.tsv"), "--snp-matrix", "all.npz"])
    assert args.snp_file == str(tmp_path / "snps.tsv") and args.snp_matrix == "all.npz"
    plain = cli.build_parser().parse_args(["reconstruct", "-e", str(tmp_path / "s.tpm"), "-t", str(tmp_path / "t.npz")])
    assert plain.snp_file is None and plain.snp_matrix is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["reconstruct", "--help"])
    text = capsys.readouterr().out
    assert "--snp-file" in text and "--snp-matrix" in text
    # the matrix without the SNP file or without a cohort is an argument error, logged like the command's other errors
    # before any file is read (the files here are no tables) or a device is opened
    with caplog.at_level(logging.ERROR, logger="gbrs"):
        cli.main(["reconstruct", "-e", str(tmp_path / "s.tpm"), "-t", str(tmp_path / "t.npz"), "--snp-matrix", "all.npz"])
        cli.main(["reconstruct", "-e", str(tmp_path / "s.tpm"), "-t", str(tmp_path / "t.npz"),
                  "--snp-file", str(tmp_path / "snps.tsv"), "--snp-matrix", "all.npz"])
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert errors == ["--snp-matrix needs --snp-file", "--snp-matrix needs --sample-file"]
    assert not (tmp_path / "all.npz").exists()
