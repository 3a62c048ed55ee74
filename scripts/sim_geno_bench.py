#!/usr/bin/env python
"""Times the path draws of `gbrs reconstruct --sim-geno` (gbrs_hmm_sample_paths) at the benchmark's HMM size
(40k genes x 36 states): 1 and 64 samples per launch, K = 100 and K = 1000 draws.

Per configuration, after one untimed call of the same shape: the device time of the sampling kernels over all slabs
(gbrs_hmm_sample_info), the wall time of the whole call (kernels + the copies out, which the call ends with), the copy-out
share as wall minus device, and the time to write one sample's `.sim_geno.npz`.  Beside them the same handle's HMM pass
(last_emission_ms + last_run_ms) and the numpy restatement (tests/sim_geno_restate.py) on one core for one sample, timed on
--restate-draws draws of the longest chromosome and scaled by genes and draws - the output says so.

    python scripts/sim_geno_bench.py [--out profiles/sim_geno_bench.json] [--samples 1,64] [--draws 100,1000] [--reps 3]

Needs an MI355X; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_geno_bench.json"))
    ap.add_argument("--samples", default="1,64")
    ap.add_argument("--draws", default="100,1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate-draws", type=int, default=100)
    ap.add_argument("--haps", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    from gbrs_amd import _lib, synth
    from gbrs_amd.hmm import DiplotypeHMM
    from gbrs_amd.npzfast import savez_compressed
    if _lib.load().gbrs_device_count() < 1:
        raise SystemExit("no device: the draws are timed on an MI355X or not at all")
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
        for K in [int(x) for x in args.draws.split(",")]:
            hmm.sample_paths(K, seed=1)                          # untimed: first launch of the shape, the buffers
            dev, wall = [], []
            for rep in range(args.reps):
                t0 = time.perf_counter()
                drawn = hmm.sample_paths(K, seed=2 + rep)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(hmm.sample_info()[0])
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                savez_compressed(os.path.join(tmp, "s.sim_geno.npz"),
                                 {c: np.ascontiguousarray(drawn["paths"][ci][0]) for ci, c in enumerate(chroms)})
                write_ms = (time.perf_counter() - t0) * 1e3
            rows.append(dict(samples=ns, draws=K, genes=int(sum(n_genes)), states=hmm.S,
                             device_ms=sorted(dev), device_ms_median=float(np.median(dev)),
                             call_wall_ms=sorted(wall), call_wall_ms_median=float(np.median(wall)),
                             copy_out_and_host_ms=float(np.median(wall) - np.median(dev)),
                             npz_write_ms_one_sample=write_ms, device_bytes=int(hmm.sample_info()[1]),
                             path_bytes=int(ns * K * sum(n_genes)), degenerate=int(drawn["degenerate"]),
                             hmm_pass_ms_same_handle=hmm_ms,
                             mean_changes_per_draw=float(drawn["changes"].sum(axis=-1).mean())))
            print(json.dumps(rows[-1]), flush=True)
    # the restatement on one core, one sample: the longest chromosome, a few draws, scaled
    import sim_geno_restate as restate
    ci = int(np.argmax(n_genes))
    alpha = hmm.get(ci, sample=0, want=("alpha",))["alpha"]
    t0 = time.perf_counter()
    restate.sample_paths(alpha, prob.tprob[chroms[ci]], 2, 0, ci, args.restate_draws)
    dt = time.perf_counter() - t0
    per_gene_draw = dt / (n_genes[ci] * args.restate_draws)
    restated = dict(measured_s=dt, on=f"chromosome {chroms[ci]} ({n_genes[ci]} genes), {args.restate_draws} draws, one core",
                    scaled_from_fewer_draws=True,
                    scaled_s_per_sample={str(K): per_gene_draw * sum(n_genes) * K for K in (100, 1000)},
                    note="scaled linearly by genes and draws from the measured run; the per-step Python overhead is "
                         "amortised over the draws, so the K = 1000 figure is an upper estimate")
    hmm.close()
    out = dict(what="gbrs_hmm_sample_paths at the benchmark's HMM size", reps=args.reps, rows=rows, restatement=restated)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(dict(out=args.out, restatement=restated)))


if __name__ == "__main__":
    main()
