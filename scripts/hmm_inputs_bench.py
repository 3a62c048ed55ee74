#!/usr/bin/env python3
"""Wall time of `gbrs get-transition-prob` and `gbrs get-alignment-spec` as fresh processes.

    python scripts/hmm_inputs_bench.py [--markers 47000] [--strains 8] [--files 3] [--runs 3] [--out result.json]

Writes a marker file of --markers genes over 20 chromosomes, and for --strains founder strains --files genes.tpm reports
each over the same genes, into a temporary $GBRS_DATA; runs each command --runs times (the first run of a process on a
machine also pays the HIP runtime's cold start, so every run is listed) and prints one JSON line with the wall seconds of
every run and the command's own stage times (load, device, save; GBRS_STAGE_TIMES).  Every command runs under a time
limit and a failure ends the script.  No speed claim hangs on this: the commands are small."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 120


def write_inputs(work, n_markers, n_strains, n_files, seed=5):
    rng = np.random.default_rng(seed)
    genes = [f"ENSMUSG{k:011d}" for k in range(n_markers)]
    chroms = [str(c) for c in range(1, 20)] + ["X"]
    per = np.array_split(np.arange(n_markers), len(chroms))
    with open(os.path.join(work, "markers.tsv"), "w") as fh:
        for c, idx in zip(chroms, per):
            cm = np.cumsum(rng.uniform(0.0, 0.1, size=len(idx)))
            bp = 3_000_000 + np.cumsum(rng.integers(1_000, 100_000, size=len(idx)))
            fh.writelines(f"{genes[k]}\t{c}\t{int(b)}\t{float(x)!r}\n" for k, b, x in zip(idx, bp, cm))
    with open(os.path.join(work, "ref.gene2transcripts.tsv"), "w") as fh:
        fh.writelines(f"{g}\tENSMUST{k:011d}\n" for k, g in enumerate(genes))
    strains = [chr(ord("A") + i) for i in range(n_strains)]
    with open(os.path.join(work, "samples.tsv"), "w") as sl:
        for i, st in enumerate(strains):
            for f in range(n_files):
                path = os.path.join(work, f"{st}_{f}.genes.tpm")
                v = np.round(rng.lognormal(0.0, 1.5, size=(n_markers, n_strains)), 3)
                v[:, i] += 10.0
                with open(path, "w") as fh:
                    fh.write("locus\t" + "\t".join(strains) + "\ttotal\n")
                    fh.writelines(g + "\t" + "\t".join(repr(float(x)) for x in row) + "\t" + repr(float(row.sum())) + "\n"
                                  for g, row in zip(genes, v))
                sl.write(f"{st}\t{path}\n")
    return strains


def run(cmd, work):
    stage_file = os.path.join(work, "stages.json")
    env = dict(os.environ, GBRS_DATA=work, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()),
               PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, "-m", "gbrs_amd"] + cmd, env=env, cwd=work,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit(f"{cmd[0]} ended with status {r.returncode}\n{r.stderr[-2000:]}")
    with open(stage_file) as fh:
        stages = json.load(fh)
    if "error" in stages:
        sys.exit(f"{cmd[0]} failed: {stages['error']}")
    return dict(wall=round(wall, 4), **{k: round(v, 4) for k, v in stages.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=47_000)
    ap.add_argument("--strains", type=int, default=8)
    ap.add_argument("--files", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="gbrs_hmm_inputs_bench_") as work:
        strains = write_inputs(work, a.markers, a.strains, a.files)
        result = dict(markers=a.markers, strains=a.strains, files_per_strain=a.files,
                      get_transition_prob=[run(["get-transition-prob", "-i", os.path.join(work, "markers.tsv")], work)
                                           for _ in range(a.runs)],
                      get_alignment_spec=[run(["get-alignment-spec", "-i", os.path.join(work, "samples.tsv"), "-s",
                                               ",".join(strains)], work) for _ in range(a.runs)])
        for name in ("tranprob.npz", "ref.gene_pos.ordered.npz", "axes.npz", "ases.npz", "avecs.npz"):
            result[name + "_bytes"] = os.path.getsize(os.path.join(work, name))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
