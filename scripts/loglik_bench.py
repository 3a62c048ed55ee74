#!/usr/bin/env python
"""Times the log-likelihood pass of `gbrs reconstruct --loglik / --alt-tprob-file` (gbrs_hmm_loglik,
gbrs_hmm_loglik_tables) at the benchmark's HMM size (40k genes x 36 states): 1 and 64 samples per launch.

Per configuration, after one untimed call of every shape: the device time of the reduction (gbrs_hmm_loglik_info), of one
full-genome candidate (the sum of its per-chromosome launches, exp of the tables included), of a candidate that differs on
the last chromosome only, the wall time of the same calls (uploads and copies included), and the device memory the pass
holds; beside them the same handle's HMM pass (last_emission_ms + last_run_ms).

Then the user's view, as fresh commands on table files on disk (members stored, not deflated - the output says so): what a
user does without the feature, `gbrs reconstruct` once per candidate file, against one command with --alt-tprob-file; each
chain twice, alternating.

    python scripts/loglik_bench.py [--out profiles/loglik_bench.json] [--samples 1,64] [--reps 5] [--no-commands]

Needs an MI355X; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik_bench.json"))
    ap.add_argument("--samples", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--no-commands", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from gbrs_amd import _lib, synth
    from gbrs_amd.hmm import DiplotypeHMM
    if _lib.load().gbrs_device_count() < 1:
        raise SystemExit("no device: the log-likelihood pass is timed on an MI355X or not at all")
    H = args.haps
    prob = synth.make_hmm_problem(H=H)
    other = synth.make_hmm_problem(H=H, seed=synth.SEED_HMM + 1)          # the candidate: same shapes, other tables
    chroms = prob.chroms
    n_genes = [len(prob.gene_ids[c]) for c in chroms]
    hmm = DiplotypeHMM(H, chroms, n_genes, [prob.tprob[c] for c in chroms])
    ha = [np.array([g in prob.avecs for g in prob.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([prob.avecs.get(g, np.zeros((H, H))) for g in prob.gene_ids[c]]) for c in chroms]
    base = [np.array([prob.expr[g] for g in prob.gene_ids[c]]) for c in chroms]
    last = len(chroms) - 1

    def candidate(which):
        """(device ms, wall ms) of one candidate over the chromosomes `which`, one launch per chromosome."""
        dev, t0 = 0.0, time.perf_counter()
        for ci in which:
            hmm.loglik_tables(ci, [other.tprob[chroms[ci]]])
            dev += hmm.loglik_info()[0]
        return dev, (time.perf_counter() - t0) * 1e3

    rows = []
    first = True
    for ns in [int(x) for x in args.samples.split(",")]:
        rng = np.random.default_rng(ns)
        ex = [np.stack([e] + [rng.gamma(1.0, 5.0, size=e.shape) * (rng.random(e.shape) < 0.5) for _ in range(ns - 1)])
              for e in base]
        if first:
            hmm.set_expression(ex, av, ha, 1.5, 0.12)
            first = False
        else:
            hmm.set_expression(ex, expr_threshold=1.5, sigma=0.12)
        hmm.run()
        hmm.set_expression(ex, expr_threshold=1.5, sigma=0.12)
        hmm.run()
        inf = hmm.info()
        hmm_ms = inf.last_emission_ms + inf.last_run_ms
        hmm.loglik()                                             # untimed: first launches of the shapes, the buffers
        candidate(range(len(chroms)))
        timed = {}
        for label, call in (("reduction", None), ("full_candidate", range(len(chroms))), ("last_chromosome_candidate", [last])):
            dev, wall = [], []
            for _ in range(args.reps):
                if call is None:
                    t0 = time.perf_counter()
                    ll = hmm.loglik()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    dev.append(hmm.loglik_info()[0])
                else:
                    d, w = candidate(call)
                    dev.append(d)
                    wall.append(w)
            timed[label] = dict(device_ms=sorted(dev), device_ms_median=float(np.median(dev)),
                                call_wall_ms=sorted(wall), call_wall_ms_median=float(np.median(wall)))
        rows.append(dict(samples=ns, genes=int(sum(n_genes)), states=hmm.S, chromosomes=len(chroms),
                         longest_chromosome_genes=int(max(n_genes)), last_chromosome_genes=int(n_genes[last]), timed=timed,
                         hmm_pass_ms_same_handle=hmm_ms, device_bytes=int(hmm.loglik_info()[1]),
                         table_bytes_16_per_entry_longest=int(16 * (max(n_genes) - 1) * hmm.S * hmm.S),
                         mean_loglik_per_sample=float(ll.sum(axis=1).mean())))
        print(json.dumps(rows[-1]), flush=True)
    hmm.close()
    out = dict(what="gbrs_hmm_loglik / gbrs_hmm_loglik_tables at the benchmark's HMM size", reps=args.reps, rows=rows)

    if not args.no_commands:
        import grid_cases
        with tempfile.TemporaryDirectory() as work:
            rng = np.random.default_rng(7)
            where = {c: np.sort(rng.uniform(0.5, 190.0, size=n)) for c, n in zip(chroms, n_genes)}
            paths = grid_cases.write_tables(work, prob, where)
            x_only = dict(prob.tprob)
            x_only[chroms[last]] = other.tprob[chroms[last]]
            files = {"last_chromosome_differs": os.path.join(work, "x_only.npz"), "every_chromosome_differs": os.path.join(work, "other.npz")}
            np.savez(files["last_chromosome_differs"], **x_only)
            np.savez(files["every_chromosome_differs"], **{c: other.tprob[c] for c in chroms})
            tpm = grid_cases.write_genes_tpm(os.path.join(work, "s.genes.tpm"), prob)
            env = dict(os.environ, GBRS_DATA=work, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            common = [sys.executable, "-m", "gbrs_amd", "reconstruct", "-e", tpm, "-x", paths["avecs"], "-g", paths["gpos"]]

            def command(extra, tag):
                t0 = time.perf_counter()
                subprocess.run(common + extra + ["-o", os.path.join(work, tag)], env=env, check=True, timeout=240,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                return time.perf_counter() - t0

            command(["-t", paths["tprob"]], "warm")              # page cache, code objects on disk
            commands = {}
            for label, alt in files.items():
                chain, one = [], []
                for rep in range(2):
                    chain.append(command(["-t", paths["tprob"]], "a") + command(["-t", alt], "b"))
                    one.append(command(["-t", paths["tprob"], "--alt-tprob-file", alt], "c"))
                with open(os.path.join(work, "c.loglik.tsv")) as fh:
                    selected = fh.read().splitlines()[-1]
                commands[label] = dict(two_fresh_commands_wall_s=chain, one_command_with_alt_wall_s=one,
                                       selected=os.path.basename(selected))
                print(json.dumps({label: commands[label]}), flush=True)
            out["commands"] = dict(note="fresh processes, one sample; table files with stored (not deflated) members, in the "
                                        "page cache; the two-command chain has no likelihood to compare, the one command does",
                                   table_file_bytes=os.path.getsize(paths["tprob"]), runs=commands)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(dict(out=args.out)))


if __name__ == "__main__":
    main()
