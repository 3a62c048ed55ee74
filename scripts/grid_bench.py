#!/usr/bin/env python3
"""`gbrs reconstruct --grid-file` and `--sample-file` at DO size, against the chain of three commands.

    python scripts/grid_bench.py [--baseline-root DIR] [--samples 64,256] [--grid-points 64000] [--runs 3] [--out profiles/grid_bench.json]

Inputs: the DO-sized synthetic genome of tests/test_hmm_gpu.py::test_hmm_full_size_properties (synth.make_hmm_problem(H=8):
20 chromosomes, 40,000 genes), gene positions drawn per chromosome, a grid of --grid-points markers spread evenly over the
chromosomes, and one genes.tpm per sample.  Recorded, all wall times of fresh processes unless said otherwise:

  grid_one_sample   `reconstruct -e ... --grid-file` (and once with --grid-genoprobs), --runs times, with its stage times
  grid_pass_ms      device time of the grid pass alone (gbrs_hmm_grid_info), dosage only and with gamma_grid, 1 / 64 / 256
                    samples on one handle in this process
  sample_file       `reconstruct --sample-file ... --grid-file` at every count of --samples: wall, wall per sample, stages
  baseline          `reconstruct`, `interpolate`, `export` of the PARENT commit on the same files, --runs times: the modules
                    under --baseline-root (a built checkout of the parent commit); without the option the entry says
                    "not measured".  The code under test is never its own baseline.

The one time condition of the change is checked at the end: the best one-sample `reconstruct --grid-file` takes no longer
than the parent's best `reconstruct` + `interpolate`.  Every command runs under a time limit and a failure ends the script."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LIMIT = 600


def write_inputs(work, n_samples, grid_points):
    """$GBRS_DATA of the full-size problem, the grid file and n_samples genes.tpm files (sample 0: the problem's own rows,
    the others drawn by the same recipe).  Returns the paths and the problem."""
    from gbrs_amd import synth
    from gbrs_amd.npzfast import savez_compressed
    prob = synth.make_hmm_problem(H=8)
    rng = np.random.default_rng(21)
    paths = dict(tprob=os.path.join(work, "tranprob.npz"), avecs=os.path.join(work, "avecs.npz"),
                 gpos=os.path.join(work, "ref.gene_pos.ordered.npz"), grid=os.path.join(work, "grid.txt"))
    with open(os.path.join(work, "ref.fa.fai"), "w") as fh:
        fh.writelines(f"{c}\t200000000\t0\t60\t61\n" for c in prob.chroms)
    np.savez(paths["tprob"], **prob.tprob)                        # stored members, as the DO tables are read fastest
    savez_compressed(paths["avecs"], prob.avecs)
    gpos, per = {}, grid_points // len(prob.chroms)
    with open(paths["grid"], "w") as fh:
        fh.write("marker\tchr\tbp\tcM\n")
        for k, c in enumerate(prob.chroms):
            n = len(prob.gene_ids[c])
            arr = np.zeros(n, dtype=[("f0", "U24"), ("f1", "f8")])
            arr["f0"] = prob.gene_ids[c]
            arr["f1"] = np.sort(rng.uniform(3.0, 100.0, size=n))
            gpos[c] = arr
            m = per + (grid_points - per * len(prob.chroms) if k == 0 else 0)
            fh.writelines(f"m{c}_{i}\t{c}\t{int(x * 1e6)}\t{float(x)!r}\n" for i, x in enumerate(np.linspace(0.0, 101.0, m)))
    savez_compressed(paths["gpos"], gpos)
    ids = [g for c in prob.chroms for g in prob.gene_ids[c]]
    tpm = []
    for s in range(n_samples):
        e = np.array([prob.expr[g] for g in ids]) if s == 0 else \
            rng.gamma(1.0, 5.0, size=(len(ids), 8)) * (rng.random((len(ids), 8)) < 0.5)
        e = np.round(e, 3)                                        # three decimals, as a report carries them
        path = os.path.join(work, f"s{s}.genes.tpm")
        body = ("%s\t" + "\t".join(["%r"] * 9) + "\n") * len(ids)
        cells = np.column_stack((e, e.sum(axis=1))).tolist()
        with open(path, "w") as fh:
            fh.write("locus\t" + "\t".join(prob.hap_names) + "\ttotal\n")
            fh.write(body % tuple(x for g, row in zip(ids, cells) for x in (g, *row)))
        tpm.append(path)
    return paths, prob, tpm


def run(argv, work, root):
    """One `gbrs` subcommand of the checkout at `root` as a fresh process: wall seconds and its own stage times."""
    stage_file = os.path.join(work, "stages.json")
    env = dict(os.environ, GBRS_DATA=work, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()),
               PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("GBRS_TUNING_LIB", None)
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, "-m", "gbrs_amd"] + argv, env=env, cwd=work,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit(f"{argv[0]} ended with status {r.returncode}\n{r.stderr[-2000:]}")
    with open(stage_file) as fh:
        stages = json.load(fh)
    if "error" in stages:
        sys.exit(f"{argv[0]} failed: {stages['error']}")
    return dict(wall=round(wall, 4), **{k: round(v, 4) for k, v in stages.items()})


def grid_pass_times(paths, prob, tpm, counts):
    """Device milliseconds of the grid pass on one handle of this process, per sample count: (dosage only, with gamma_grid),
    the second of two calls each."""
    from gbrs_amd.hmm import ReconstructContext, _expression_rows, read_gene_tpm
    ctx = ReconstructContext(paths["tprob"], paths["avecs"], paths["gpos"], 0, paths["grid"])
    ctx.load()
    spec = ctx.specificity(8)
    hmm, _ = ctx.handle(8)
    out = {}
    first = True
    for n in counts:
        rows = [_expression_rows(ctx, *read_gene_tpm(f)[1:], 8) for f in tpm[:n]]
        stacked = [np.stack([r[ci] for r in rows]) for ci in range(len(ctx.chroms))]
        if first:
            hmm.set_expression(stacked, [x[0] for x in spec], [x[1] for x in spec], 1.5, 0.12)
        else:
            hmm.set_expression(stacked, expr_threshold=1.5, sigma=0.12)
        first = False
        hmm.run()
        ms = {}
        for label, want in (("dosage", ("dosage",)), ("dosage_and_gamma_grid", ("dosage", "gamma_grid"))):
            if label != "dosage" and n > 64:
                continue                               # 64,000 x 36 doubles per sample on the host as well
            for _ in range(2):
                hmm.grid(want=want)
            ms[label] = round(hmm.grid_info()[1], 4)
        out[str(n)] = dict(ms, hmm_run_ms=round(hmm.info().last_run_ms, 4))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--samples", default="64,256")
    ap.add_argument("--grid-points", type=int, default=64_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grid_bench.json"))
    a = ap.parse_args()
    counts = [int(x) for x in a.samples.split(",") if x]
    with tempfile.TemporaryDirectory(prefix="gbrs_grid_bench_") as work:
        os.environ["GBRS_DATA"] = work                    # the in-process part reads ref.fa.fai there, like the commands
        t0 = time.perf_counter()
        paths, prob, tpm = write_inputs(work, max(counts + [1]), a.grid_points)
        result = dict(genes=prob.num_genes, grid_points=a.grid_points, write_inputs_s=round(time.perf_counter() - t0, 2))
        common = ["-t", paths["tprob"], "-x", paths["avecs"], "-g", paths["gpos"]]
        one = os.path.join(work, "one")
        result["grid_one_sample"] = [run(["reconstruct", "-e", tpm[0], "--grid-file", paths["grid"], "-o", one] + common,
                                         work, REPO) for _ in range(a.runs)]
        result["grid_one_sample_with_genoprobs"] = run(["reconstruct", "-e", tpm[0], "--grid-file", paths["grid"],
                                                        "--grid-genoprobs", "-o", one] + common, work, REPO)
        result["grid_pass_ms"] = grid_pass_times(paths, prob, tpm, [1] + counts)
        result["sample_file"] = {}
        for n in counts:
            listing = os.path.join(work, f"samples_{n}.txt")
            with open(listing, "w") as fh:
                fh.writelines(f"{f}\t{os.path.join(work, f'many{n}_{k}')}\n" for k, f in enumerate(tpm[:n]))
            r = run(["reconstruct", "--sample-file", listing, "--batch-size", str(n), "--grid-file", paths["grid"]] + common,
                    work, REPO)
            r["wall_per_sample"] = round(r["wall"] / n, 4)
            result["sample_file"][str(n)] = r
            for k in range(n):
                for suffix in ("genoprobs.npz", "genotypes.npz", "genotypes.tsv", "interpolated.genoprobs.tsv"):
                    os.remove(os.path.join(work, f"many{n}_{k}.{suffix}"))
        if a.baseline_root:
            root = os.path.abspath(a.baseline_root)
            base = os.path.join(work, "base")
            chain = []
            for _ in range(a.runs):
                chain.append(dict(
                    reconstruct=run(["reconstruct", "-e", tpm[0], "-o", base] + common, work, root),
                    interpolate=run(["interpolate", "-i", base + ".genoprobs.npz", "-g", paths["grid"], "-p", paths["gpos"],
                                     "-o", base + ".interp.npz"], work, root),
                    export=run(["export", "-i", base + ".interp.npz", "-s", ",".join(prob.hap_names), "-g", paths["grid"],
                                "-o", base + ".export.tsv"], work, root)))
            result["baseline"] = chain
            a_ = np.loadtxt(one + ".interpolated.genoprobs.tsv", skiprows=1, delimiter="\t")
            b_ = np.loadtxt(base + ".export.tsv", skiprows=1, delimiter="\t")
            result["max_text_difference_from_the_chain"] = float(np.abs(a_ - b_).max())
            best = min(r["wall"] for r in result["grid_one_sample"])
            allowed = min(r["reconstruct"]["wall"] + r["interpolate"]["wall"] for r in chain)
            result["time_condition"] = dict(grid_one_sample_best=best, parent_reconstruct_plus_interpolate_best=round(allowed, 4),
                                            met=bool(best <= allowed))
        else:
            result["baseline"] = "not measured"
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if isinstance(result["baseline"], list) and not result["time_condition"]["met"]:
        sys.exit("reconstruct --grid-file took longer than the parent's reconstruct + interpolate")


if __name__ == "__main__":
    main()
