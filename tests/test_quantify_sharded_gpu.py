"""`python -m gbrs_amd quantify --gpus N` end to end, every command a fresh process under a time limit: the reports of the
single-GPU command (the goldens' numbers within 1e-9, the golden's iteration count, `-a` byte for byte), the path the
ranks took (GBRS_STAGE_TIMES), one-rank and two-rank RCCL groups, a 2M-read sample, and a rank that fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from sharded_cases import check_reports_against_golden, check_reports_close, write_case

pytestmark = pytest.mark.gpu

TIME_LIMIT_S = 300


def _run(argv, tmp_path, tag):
    env = dict(os.environ, GBRS_STAGE_TIMES=str(tmp_path / f"{tag}.json"))
    p = subprocess.run(["timeout", "-k", "10", str(TIME_LIMIT_S), sys.executable, "-m", "gbrs_amd"] + argv, cwd=ROOT,
                       env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    with open(tmp_path / f"{tag}.json") as fh:
        return json.load(fh), p.stderr


def _outputs(tmp_path, tag):
    return sorted(f[len(tag) + 1:] for f in os.listdir(tmp_path) if f.startswith(tag + "."))


CASES = [("h8_count_len", "npz", False, "two-engine"), ("h8_pseudo", "npz", False, "single-engine"),
         ("h8_mask", "npz", True, None), ("h8_values", "h5", False, None), ("h16_len", "npz", False, None)]


@pytest.mark.parametrize("name,fmt,use_mask,path", CASES)
def test_two_gloo_ranks_on_one_gpu(tmp_path, name, fmt, use_mask, path):
    argv, suffix, g, calls = write_case(tmp_path, name, fmt, use_mask)
    one, _ = _run(argv + ["-a", "-o", str(tmp_path / "one")], tmp_path, "one")
    two, err = _run(argv + ["-a", "-o", str(tmp_path / "two"), "--gpus", "2", "--devices", "0,0",
                            "--dist-backend", "gloo"], tmp_path, "two")
    assert "error" not in two and all("error" not in r for r in two["ranks"]), two
    assert (two["world"], two["backend"]) == (2, "gloo")
    assert two["path"] in ("two-engine", "single-engine") and (path is None or two["path"] == path)
    assert [r["path"] for r in two["ranks"]] == [two["path"]] * 2
    assert two["em_iterations"] == one["em_iterations"] == int(g["num_iters"])
    assert _outputs(tmp_path, "two") == _outputs(tmp_path, "one")
    check_reports_against_golden(tmp_path / f"two.{suffix}", g)
    if use_mask:
        from sharded_cases import parse_tsv
        head, rows = parse_tsv(open(tmp_path / f"two.{suffix}.genes.tpm").read())
        assert head[-1] == "notes" and [v[-1] for v in rows.values()] == calls
    for level in ("isoforms", "genes"):
        f = f"{suffix}.{level}.alignment_counts"
        assert open(tmp_path / f"two.{f}").read() == open(tmp_path / f"one.{f}").read()


def test_one_rank_rccl_group(tmp_path):
    argv, suffix, g, _ = write_case(tmp_path, "h8_count_len")
    st, err = _run(argv + ["-o", str(tmp_path / "r"), "--gpus", "1", "--dist-backend", "nccl", "-v"], tmp_path, "r")
    assert (st["world"], st["backend"], st["path"]) == (1, "nccl", "two-engine")
    assert st["em_iterations"] == int(g["num_iters"])
    assert "Sharded EM: world 1, backend nccl, two-engine path" in err
    check_reports_against_golden(tmp_path / f"r.{suffix}", g)


def test_two_rank_rccl_group(tmp_path):
    from gbrs_amd import _lib
    if _lib.load().gbrs_device_count() < 2:
        pytest.skip("one GPU visible: RCCL takes one rank per GPU")
    argv, suffix, g, _ = write_case(tmp_path, "h16_len")
    st, _ = _run(argv + ["-o", str(tmp_path / "r"), "--gpus", "2", "--devices", "0,1"], tmp_path, "r")
    assert (st["world"], st["backend"]) == (2, "nccl")
    assert st["em_iterations"] == int(g["num_iters"])
    check_reports_against_golden(tmp_path / f"r.{suffix}", g)


def _synthetic_sample(tmp_path, R):
    """A ~2M-read sample written as .npz, with group and length files (gbrs_amd.synth)."""
    from gbrs_amd import synth
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    inc = synth.make_em_problem(R=R, H=8, L=4000, seed=11)
    apm = AlignmentPropertyMatrix(shape=(inc.num_loci, inc.num_haps, inc.num_rows), indptr=inc.indptr,
                                  indices=inc.indices, haplotype_names=inc.hap_names, locus_names=inc.locus_names)
    apm.save_npz(str(tmp_path / "big.npz"))
    with open(tmp_path / "big.g2t", "w") as fh:
        for i, mem in enumerate(inc.groups):
            fh.write(f"G{i:06d}\t" + "\t".join(inc.locus_names[m] for m in mem) + "\n")
    raw = inc.effective_length(100)[0] + 99.0
    with open(tmp_path / "big.len", "w") as fh:
        for l, name in enumerate(inc.locus_names):
            for h in inc.hap_names:
                fh.write(f"{name}_{h}\t{int(raw[l])}\n")
    return ["quantify", "-i", str(tmp_path / "big.npz"), "-g", str(tmp_path / "big.g2t"), "-L", str(tmp_path / "big.len")]


def test_two_million_reads_both_paths(tmp_path):
    argv = _synthetic_sample(tmp_path, 2_000_000)
    names = ["isoforms.tpm", "isoforms.expected_read_counts", "genes.tpm", "genes.expected_read_counts"]
    for extra, path in (([], "two-engine"), (["-p", "0.25"], "single-engine")):
        tag = "p" if extra else "z"
        one, _ = _run(argv + extra + ["-o", str(tmp_path / f"{tag}one")], tmp_path, f"{tag}one")
        two, _ = _run(argv + extra + ["-o", str(tmp_path / f"{tag}two"), "--gpus", "2", "--devices", "0,0",
                                      "--dist-backend", "gloo"], tmp_path, f"{tag}two")
        assert two["path"] == path, two
        assert two["em_iterations"] == one["em_iterations"]
        check_reports_close(tmp_path / f"{tag}one.multiway", tmp_path / f"{tag}two.multiway", names)


def test_a_failing_rank_ends_the_command(tmp_path):
    """A device ordinal that does not exist: that rank exits with an error, the launcher stops the other one, logs
    which rank failed and returns 0 with no reports."""
    from gbrs_amd import _lib
    n = _lib.load().gbrs_device_count()
    argv, suffix, g, _ = write_case(tmp_path, "h8_count_len")
    out = tmp_path / "out"
    out.mkdir()
    st, err = _run(argv + ["-o", str(out / "q"), "--gpus", "2", "--devices", f"0,{n + 7}", "--dist-backend", "gloo"],
                   tmp_path, "fail")
    assert f"rank 1 of 2 failed" in err and f"device {n + 7} is not one of" in err, err[-2000:]
    assert "rank 1 of 2 failed" in st.get("error", "")
    assert os.listdir(out) == []
    # no child is left: nothing runs the rank module any more
    ps = subprocess.run(["ps", "-eo", "args"], capture_output=True, text=True).stdout
    assert str(out / "q") not in ps
