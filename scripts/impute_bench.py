#!/usr/bin/env python3
"""The imputation pass (`gbrs reconstruct --snp-file`) at DO size, against the grid route.

    python scripts/impute_bench.py [--samples 1,64] [--snps 143000,10000000] [--chunk 1048576] [--runs 3] [--out profiles/impute_bench.json]

Inputs: the DO-sized synthetic genome of scripts/grid_bench.py (synth.make_hmm_problem(H=8): 20 chromosomes, 40,000 genes x
36 states), gene positions drawn per chromosome, the SNPs spread evenly over the chromosomes at ascending positions with
random founder allele patterns, samples drawn by that script's recipe.  Everything stays in this process: one handle, one
run per sample count, one set_snps per SNP count.  Recorded per (SNPs, samples):

  setup_ms           device time of the search kernel of gbrs_hmm_set_snps, from events; set_snps_wall_ms: the call
  dosage_ms          device time of the kernel that makes D[n][genes][H], once per run
  kernel_ms          device time of the imputation kernel, summed over the chunks of one walk over all SNPs (second walk)
  store_gb_per_s     n x M x 8 bytes of stores over kernel_ms, share_of_hbm against the chip's 8 TB/s
  wall_ms            host clock around hmm.impute(): kernels, synchronise and the copies out into one [n, M] array, best of
                     --runs (D is made by the first walk after the run and reused; wall_first_ms is that first walk)

  grid route, the one that existed before the pass: set_grid(SNP positions), grid()['dosage'] copied to the host and
  2 * einsum('sph,ph->sp', dosage, bits) in numpy on this job's CPUs; the SNPs in slabs of --route-slab where the
  [n, M, H] dosage array would not fit (every slab its own set_grid, which is part of the route).  Timed --runs times,
  once where a walk takes more than --route-once-above seconds.

No ratio is fixed in advance; the numbers are recorded as they come."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8.0e12


def problem(n_samples):
    from gbrs_amd import synth
    prob = synth.make_hmm_problem(H=8)
    rng = np.random.default_rng(21)
    where = [np.sort(rng.uniform(3.0, 100.0, size=len(prob.gene_ids[c]))) for c in prob.chroms]
    expr = []
    for c in prob.chroms:
        n = len(prob.gene_ids[c])
        e = rng.gamma(1.0, 5.0, size=(n_samples, n, 8)) * (rng.random((n_samples, n, 8)) < 0.5)
        e[0] = np.array([prob.expr[g] for g in prob.gene_ids[c]])
        expr.append(np.round(e, 3))
    return prob, where, expr


def snp_set(n_chrom, M, H, seed):
    rng = np.random.default_rng(seed)
    per = M // n_chrom
    points = [np.linspace(0.0, 101.0, per + (M - per * n_chrom if k == 0 else 0)) for k in range(n_chrom)]
    masks = [rng.integers(0, 1 << H, size=len(x), dtype=np.uint32) for x in points]
    return points, masks


def best_of(runs, call):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3


def walk(hmm, n, M, chunk, out):
    """hmm.impute()'s loop with the kernel times of the chunks added up: (dosage_ms, kernel_ms)."""
    from gbrs_amd import _lib
    lib = _lib.load()
    dosage_ms = kernel_ms = 0.0
    for first in range(0, M, chunk):
        part = np.empty((n, min(chunk, M - first)))
        _lib.check(lib.gbrs_hmm_impute(hmm._h, -1, first, part.shape[1], _lib.ptr(part)))
        out[:, first:first + part.shape[1]] = part
        info = hmm.impute_info()
        dosage_ms += info["dosage_ms"]
        kernel_ms += info["kernel_ms"]
    return dosage_ms, kernel_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,64")
    ap.add_argument("--snps", default="143000,10000000")
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--route-slab", type=int, default=1 << 20, help="SNPs per set_grid + grid() of the grid route")
    ap.add_argument("--route-once-above", type=float, default=5.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "impute_bench.json"))
    a = ap.parse_args()
    counts = [int(x) for x in a.samples.split(",") if x]
    sizes = [int(x) for x in a.snps.split(",") if x]
    from gbrs_amd.hmm import DiplotypeHMM
    t0 = time.perf_counter()
    prob, where, expr = problem(max(counts))
    H, chroms = 8, prob.chroms
    result = dict(genes=prob.num_genes, founders=H, states=H * (H + 1) // 2, chunk=a.chunk, route_slab=a.route_slab,
                  make_inputs_s=round(time.perf_counter() - t0, 2), cpus=os.environ.get("OMP_NUM_THREADS", "not set"),
                  hbm_peak_tb_s=HBM_BYTES_PER_S / 1e12, passes={}, grid_route={})
    hmm = DiplotypeHMM(H, chroms, [len(prob.gene_ids[c]) for c in chroms], [prob.tprob[c] for c in chroms])
    ha = [np.array([g in prob.avecs for g in prob.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([prob.avecs.get(g, np.zeros((H, H))) for g in prob.gene_ids[c]]) for c in chroms]
    first = True
    for M in sizes:
        points, masks = snp_set(len(chroms), M, H, 23)
        hmm.set_snps(where, points, masks)                       # warm: code objects
        set_wall = best_of(a.runs, lambda: hmm.set_snps(where, points, masks))
        setup_ms = hmm.impute_info()["setup_ms"]
        all_x = np.concatenate(points)
        bits = ((np.concatenate(masks)[:, None] >> np.arange(H, dtype=np.uint32)) & 1).astype(np.float64)
        for n in counts:
            rows = [e[:n] for e in expr]
            if first:
                hmm.set_expression(rows, av, ha, 1.5, 0.12)
            else:
                hmm.set_expression(rows, expr_threshold=1.5, sigma=0.12)
            first = False
            hmm.run()
            out = np.empty((n, M))
            t = time.perf_counter()
            dosage_ms, _ = walk(hmm, n, M, a.chunk, out)         # first walk after the run: makes D, warms the shape
            wall_first = (time.perf_counter() - t) * 1e3
            _, kernel_ms = walk(hmm, n, M, a.chunk, out)
            del out
            kept = {}

            def device():
                kept["out"] = hmm.impute(chunk=a.chunk)
            wall = best_of(a.runs, device)
            stores = 8.0 * n * M
            entry = dict(setup_ms=round(setup_ms, 4), set_snps_wall_ms=round(set_wall, 3), dosage_ms=round(dosage_ms, 4),
                         kernel_ms=round(kernel_ms, 4), store_bytes=stores, store_gb_per_s=round(stores / kernel_ms / 1e6, 1),
                         share_of_hbm=round(stores / kernel_ms / 1e-3 / HBM_BYTES_PER_S, 4), wall_first_ms=round(wall_first, 3),
                         wall_ms=round(wall, 3), device_bytes=hmm.impute_info()["device_bytes"])
            result["passes"][f"{M}x{n}"] = entry
            print(f"{M} SNPs x {n} samples: {entry}", flush=True)

            # the grid route; its slabs take the chromosomes' SNPs in handle order
            bounds = np.concatenate(([0], np.cumsum([len(x) for x in points])))

            def route():
                got = np.empty((n, M))
                for lo in range(0, M, a.route_slab):
                    hi = min(M, lo + a.route_slab)
                    slab = [all_x[max(lo, b0):min(hi, b1)] if min(hi, b1) > max(lo, b0) else None
                            for b0, b1 in zip(bounds[:-1], bounds[1:])]
                    hmm.set_grid(where, slab)
                    d = hmm.grid()["dosage"]
                    got[:, lo:hi] = 2.0 * np.einsum("sph,ph->sp", d, bits[lo:hi])
                kept["route"] = got
            t = time.perf_counter()
            route()
            once = time.perf_counter() - t
            few = once > a.route_once_above or a.runs < 2
            route_ms = once * 1e3 if few else min(once * 1e3, best_of(a.runs - 1, route))
            differ = float(np.nanmax(np.abs(kept["route"] - kept["out"])))
            result["grid_route"][f"{M}x{n}"] = dict(route_ms=round(route_ms, 3), timed="once" if few else f"best of {a.runs}",
                                                    device_wall_ms=entry["wall_ms"], device_wall_first_ms=entry["wall_first_ms"],
                                                    max_abs_difference=differ)
            print(f"  grid route: {result['grid_route'][f'{M}x{n}']}", flush=True)
            kept.clear()
    hmm.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
