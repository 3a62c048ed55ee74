#!/usr/bin/env python
"""Times the diagnostics of `gbrs reconstruct --diagnostics` (gbrs_hmm_diagnostics) at the benchmark's HMM
size (40k genes x 36 states): 1 and 64 samples per launch.

Per configuration, after one untimed call of the same shape: the device time of the two kernels
(gbrs_hmm_diagnostics_info), of the pair pass alone (a call that asks for xo and pswitch only) and of the gene pass alone,
and the wall time of the whole call (kernels + the five copies out).  Beside them the same handle's HMM pass
(last_emission_ms + last_run_ms), the device time of `--sim-geno 100` (gbrs_hmm_sample_paths) on the same run, and the numpy
restatement (tests/diagnostics_restate.py) on one core for one sample, timed on the longest chromosome and scaled by genes -
the output says so.

    python scripts/diagnostics_bench.py [--out profiles/diagnostics_bench.json] [--samples 1,64] [--reps 5]

Needs an MI355X; there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics_bench.json"))
    ap.add_argument("--samples", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sim-geno", type=int, default=100)
    ap.add_argument("--haps", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    from gbrs_amd import _lib, synth
    from gbrs_amd.hmm import DiplotypeHMM
    if _lib.load().gbrs_device_count() < 1:
        raise SystemExit("no device: the diagnostics are timed on an MI355X or not at all")
    H = args.haps
    prob = synth.make_hmm_problem(H=H)
    chroms = prob.chroms
    n_genes = [len(prob.gene_ids[c]) for c in chroms]
    hmm = DiplotypeHMM(H, chroms, n_genes, [prob.tprob[c] for c in chroms])
    ha = [np.array([g in prob.avecs for g in prob.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([prob.avecs.get(g, np.zeros((H, H))) for g in prob.gene_ids[c]]) for c in chroms]
    base = [np.array([prob.expr[g] for g in prob.gene_ids[c]]) for c in chroms]
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
        t0 = time.perf_counter()
        hmm.get(0, want=("alpha",))                              # the log-domain arrays the passes read, made once per run
        logs_ms = (time.perf_counter() - t0) * 1e3
        timed = {}
        for label, want in (("all", DiplotypeHMM.DIAGNOSTICS), ("pair", ("xo", "pswitch")),
                            ("gene", ("errlod", "maxprob", "maxmarg"))):
            hmm.diagnostics(want=want)                           # untimed: first launch of the shape, the buffers
            dev, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = hmm.diagnostics(want=want)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(hmm.diagnostics_info())
            timed[label] = dict(device_ms=sorted(dev), device_ms_median=float(np.median(dev)),
                                call_wall_ms=sorted(wall), call_wall_ms_median=float(np.median(wall)))
            if label == "all":
                mean_xo = float(np.mean([sum(a[s].sum() for a in got["xo"]) for s in range(ns)]))
        hmm.sample_paths(args.sim_geno, seed=1)
        hmm.sample_paths(args.sim_geno, seed=2)
        rows.append(dict(samples=ns, genes=int(sum(n_genes)), states=hmm.S, timed=timed,
                         make_logs_first_get_wall_ms=logs_ms, hmm_pass_ms_same_handle=hmm_ms,
                         sim_geno_draws=args.sim_geno, sim_geno_device_ms=hmm.sample_info()[0],
                         table_bytes=int(sum(n - 1 for n in n_genes) * hmm.S * hmm.S * 8),
                         exps_per_sample_pair_pass=int(sum(n - 1 for n in n_genes) * hmm.S * hmm.S),
                         mean_expected_crossovers_per_sample=mean_xo))
        print(json.dumps(rows[-1]), flush=True)
    # the restatement on one core, one sample: the longest chromosome, scaled by genes
    import diagnostics_restate as restate
    ci = int(np.argmax(n_genes))
    own = hmm.get(ci, sample=0, want=("alpha", "beta", "eprob", "gamma"))
    ch, iv = restate.change_table(H), restate.init_vec(H)
    t0 = time.perf_counter()
    restate.crossovers(own["alpha"], own["beta"], own["eprob"], prob.tprob[chroms[ci]], ch)
    restate.error_lod(own["alpha"], own["beta"], own["eprob"], iv)
    restate.most_likely(own["gamma"])
    dt = time.perf_counter() - t0
    restated = dict(measured_s=dt, on=f"chromosome {chroms[ci]} ({n_genes[ci]} genes), one sample, one core",
                    scaled_from_one_chromosome=True, scaled_s_per_sample=dt / n_genes[ci] * sum(n_genes),
                    note="scaled linearly by genes from the measured chromosome")
    hmm.close()
    out = dict(what="gbrs_hmm_diagnostics at the benchmark's HMM size", reps=args.reps, rows=rows, restatement=restated)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(dict(out=args.out, restatement=restated)))


if __name__ == "__main__":
    main()
