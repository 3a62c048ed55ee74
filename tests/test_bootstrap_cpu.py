"""`gbrs quantify --bootstrap`, the parts that need no GPU: the draw's restatement against known answers, and the
command-line plumbing and refusals."""
import argparse
import os

import numpy as np
import pytest

import bootstrap_restate as br
from conftest import GOLD, em_case_inputs, load_golden


def _hex(words):
    return " ".join("%08x" % int(np.asarray(w).ravel()[0]) for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """The Random123 vectors of Philox4x32-10."""
    assert _hex(br.philox4x32_10([np.array([c]) for c in counter], key)) == want


def test_threshold_table_is_the_formula():
    """T[j] = floor(2^32 * sum_{i <= j} e^-1 / i!), with 60-digit decimals (and the same at 50 and 80)."""
    want = [1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
            4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295]
    assert br.THRESHOLDS.tolist() == want
    for digits in (50, 60, 80):
        assert br.thresholds_from_formula(digits) == want
    assert br.poisson1(np.array([0, 1580030167, 1580030168, 4294967294, 4294967295])).tolist() == [0, 0, 1, 12, 13]


def test_weight_known_answers():
    assert br.weights(0, 0, 8).tolist() == [1, 3, 0, 2, 3, 1, 1, 1]
    assert br.weights(2 ** 63 + 5, 7, 4, [3, 0, 10000, 1]).tolist() == [1, 0, 9928, 2]


def test_weights_depend_on_seed_replicate_row_and_count_only():
    """Row r's weight is the same whatever the other rows are, and a count of c is the sum of the first c draws."""
    w = br.weights(11, 3, 40, np.arange(40) % 7)
    for r in (0, 5, 13, 39):
        alone = np.zeros(r + 1, dtype=np.int64)
        alone[r] = r % 7
        assert br.weights(11, 3, r + 1, alone)[r] == w[r]
    by_count = [int(br.weights(11, 3, 6, np.full(6, c))[5]) for c in range(10)]
    assert by_count[0] == 0 and all(b >= a for a, b in zip(by_count, by_count[1:]))
    assert not np.array_equal(br.weights(11, 4, 40, np.arange(40) % 7), w)
    assert not np.array_equal(br.weights(12, 3, 40, np.arange(40) % 7), w)
    # Poisson(1): mean and variance of 200,000 draws within five standard errors
    big = br.weights(5, 0, 200_000)
    assert abs(big.mean() - 1.0) < 5 / np.sqrt(200_000) and abs(big.var() - 1.0) < 5 * np.sqrt(3.0 / 200_000)


def test_restated_input_is_the_file_with_repeated_rows():
    g = load_golden(os.path.join(GOLD, "em_h8_count_len.npz"))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    w = br.weights(2024, 0, R, count)
    assert (w == 0).any() and (w > 0).any()
    ptr, idx, cnt = br.restate_input(indptr, indices, w)
    assert np.array_equal(cnt, w.astype(np.float64))
    for h in range(H):
        assert ptr[h][0] == 0 and ptr[h][-1] == len(idx[h]) and (w[idx[h].astype(np.int64)] > 0).all()
        old = np.repeat(np.arange(L), np.diff(indptr[h].astype(np.int64)))
        keep = w[indices[h].astype(np.int64)] > 0
        assert np.array_equal(np.repeat(np.arange(L), np.diff(ptr[h].astype(np.int64))), old[keep])
        assert np.array_equal(idx[h], indices[h][keep])


def test_parser_accepts_the_bootstrap_options(tmp_path):
    from gbrs_amd.cli import build_parser
    aln = tmp_path / "a.npz"
    aln.write_bytes(b"")
    args = build_parser().parse_args(["quantify", "-i", str(aln)])
    assert args.bootstrap is None and args.bootstrap_seed == 0 and args.keep_replicates is False
    args = build_parser().parse_args(["quantify", "-i", str(aln), "--bootstrap", "100", "--bootstrap-seed", "7",
                                      "--keep-replicates"])
    assert args.bootstrap == 100 and args.bootstrap_seed == 7 and args.keep_replicates is True
    text = build_parser()._subparsers._group_actions[0].choices["quantify"].format_help()
    assert "--bootstrap" in text and "--bootstrap-seed" in text and "--keep-replicates" in text


@pytest.fixture
def no_device(monkeypatch):
    from gbrs_amd import _lib

    def touched(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "warm_up_device_async", touched)


@pytest.mark.parametrize("kw,match", [
    (dict(bootstrap=1), r"--bootstrap needs at least 2"),
    (dict(bootstrap=0), r"--bootstrap needs at least 2"),
    (dict(bootstrap=10, merge_identical_rows=True), r"--bootstrap.*--merge-identical-rows"),
])
def test_quantify_refuses_before_any_file_or_device(tmp_path, monkeypatch, no_device, kw, match):
    from gbrs_amd import quantify as q
    monkeypatch.setattr(q, "load_alignment", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the file was read")))
    with pytest.raises(RuntimeError, match=match):
        q.quantify(str(tmp_path / "missing.npz"), outbase=str(tmp_path / "out"), **kw)
    assert os.listdir(tmp_path) == []


def test_quantify_refuses_a_file_with_values_before_any_device_call(tmp_path, no_device):
    from conftest import em_case_values
    from gbrs_amd import quantify as q
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    g = load_golden(os.path.join(GOLD, "em_h8_values.npz"))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)], values=em_case_values(g))
    aln, grp, lens = str(tmp_path / "values.npz"), str(tmp_path / "g2t.tsv"), str(tmp_path / "len.tsv")
    apm.save(aln)
    with open(grp, "w") as fh:
        for i, mem in enumerate(groups):
            fh.write(f"G{i:07d}\t" + "\t".join(apm.lname[m] for m in mem) + "\n")
    with open(lens, "w") as fh:
        for name in apm.lname:
            for h in apm.hname:
                fh.write(f"{name}_{h}\t1000\n")
    with pytest.raises(RuntimeError, match=r"--bootstrap.*stored alignment values"):
        q.quantify(aln, group_file=grp, length_file=lens, outbase=str(tmp_path / "out"), bootstrap=4)
    assert sorted(os.listdir(tmp_path)) == ["g2t.tsv", "len.tsv", "values.npz"]


def test_cli_refusals_are_logged_without_a_device(tmp_path, no_device, caplog):
    from gbrs_amd import cli
    aln = tmp_path / "a.npz"
    aln.write_bytes(b"")
    for extra, text in ((["--bootstrap", "1"], "at least 2"),
                        (["--bootstrap", "5", "--merge-identical-rows"], "--merge-identical-rows"),
                        (["--bootstrap", "5", "--gpus", "2"], "--gpus")):
        caplog.clear()
        assert cli.main(["quantify", "-i", str(aln), "-o", str(tmp_path / "out")] + extra) == 0
        assert any(text in r.getMessage() and "--bootstrap" in r.getMessage() for r in caplog.records), extra
    assert sorted(os.listdir(tmp_path)) == ["a.npz"]


def test_sharded_launcher_refuses_bootstrap():
    from gbrs_amd.sharded import check_args
    base = dict(gpus=2, multiread_model=4, report_posterior=False, merge_identical_rows=False, devices=None, device=0,
                dist_backend="nccl", posterior_values=False)
    with pytest.raises(RuntimeError, match=r"--gpus.*--bootstrap"):
        check_args(argparse.Namespace(**base, bootstrap=10))
    assert check_args(argparse.Namespace(**base, bootstrap=None)) == [0, 1]
    assert check_args(argparse.Namespace(**base)) == [0, 1]
