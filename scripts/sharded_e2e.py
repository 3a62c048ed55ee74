"""`gbrs quantify` against `gbrs quantify --gpus 1 --dist-backend nccl` on the BASELINE configs[1] sample (40M reads x 8
haplotypes x 120k isoforms, written as an EMASE file by a child process, as scripts/e2e_bench.py does): the reports must
agree to 1e-9; prints one JSON line with both commands' wall and stage times.  --profile runs the sharded command once
more under `rocprofv3 --kernel-trace --stats` and adds the times of the sharding kernels (gbrs_amd/csrc/em_shard.inc).

    python scripts/sharded_e2e.py [--rows 40000000] [--format npz] [--profile DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)

import e2e_bench  # noqa: E402

REPORTS = ("isoforms.tpm", "isoforms.expected_read_counts", "genes.tpm", "genes.expected_read_counts")


def max_rel_diff(path_a, path_b):
    """Largest relative difference of two reports' numbers (same rows and header required)."""
    with open(path_a) as fa, open(path_b) as fb:
        ha, hb = fa.readline(), fb.readline()
        if ha != hb:
            raise RuntimeError(f"headers differ: {path_a}")
        a = np.loadtxt(fa, dtype=str, delimiter="\t", ndmin=2)
        b = np.loadtxt(fb, dtype=str, delimiter="\t", ndmin=2)
    if a.shape != b.shape or (a[:, 0] != b[:, 0]).any():
        raise RuntimeError(f"rows differ: {path_a}")
    x, y = a[:, 1:].astype(np.float64), b[:, 1:].astype(np.float64)
    return float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300)))


def kernel_stats(prof_dir):
    """{kernel: (calls, total ms)} of the shard_* kernels in every stats file under prof_dir."""
    out = {}
    for f in glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "shard_" not in name:
                    continue
                key = name.split("(")[0].split(" ")[-1]
                calls, ns = out.get(key, (0, 0.0))
                out[key] = (calls + int(row["Calls"]), ns + float(row["TotalDurationNs"]))
    return {k: dict(calls=c, ms=round(ns / 1e6, 3)) for k, (c, ns) in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40_000_000)
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--loci", type=int, default=120_000)
    ap.add_argument("--format", default="npz", choices=("npz", "h5"))
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 run of the sharded command")
    args = ap.parse_args()
    workdir = tempfile.mkdtemp(prefix="gbrs-sharded-e2e-")
    sample = e2e_bench.build_sample_in_child(workdir, args.rows, args.haps, args.loci, args.format, 0)
    base = ["quantify", "-i", sample["files"][args.format], "-g", sample["group_file"], "-L", sample["length_file"]]
    res = dict(workload=f"configs[1]: R={args.rows} x H={args.haps} x L={args.loci}, {args.format}", entries=sample["N"])
    wall, st = e2e_bench.run_cli(base + ["-o", os.path.join(workdir, "one")], workdir, "one")
    res["single"] = dict(wall_s=round(wall, 3), stages=st)
    sharded = base + ["-o", os.path.join(workdir, "sh"), "--gpus", "1", "--dist-backend", "nccl"]
    wall, st = e2e_bench.run_cli(sharded, workdir, "sh")
    res["sharded_1_rank_rccl"] = dict(wall_s=round(wall, 3), stages=st)
    res["max_rel_diff"] = {r: max_rel_diff(os.path.join(workdir, f"one.multiway.{r}"), os.path.join(workdir, f"sh.multiway.{r}"))
                           for r in REPORTS}
    res["agree_1e-9"] = all(v <= 1e-9 for v in res["max_rel_diff"].values())
    if args.profile:
        args.profile = os.path.abspath(args.profile)
        os.makedirs(args.profile, exist_ok=True)
        env = dict(os.environ, PYTHONPATH=ROOT, GBRS_DATA=workdir, GBRS_ORDERLY_EXIT="1")   # the tracer writes at exit
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", args.profile, "--", sys.executable, "-m",
                            "gbrs_amd"] + base + ["-o", os.path.join(workdir, "prof"), "--gpus", "1", "--dist-backend", "nccl"],
                           env=env, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        res["profile_rc"] = r.returncode
        res["shard_kernels"] = kernel_stats(args.profile)
    print(json.dumps(res), flush=True)
    return 0 if res["agree_1e-9"] else 1


if __name__ == "__main__":
    sys.exit(main())
