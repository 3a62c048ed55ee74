#!/usr/bin/env python3
"""Permutation thresholds of the genome scan (`--scan-perms`) at eQTL size, against permuting on the host.

    python scripts/scan_perm_bench.py [--samples 64,512] [--phenotypes 1,64,1024] [--perms 1000] [--grid-points 64000]
                                      [--host-perms 8] [--out profiles/scan_perm_bench.json]

Inputs as scripts/scan_bench.py makes them: random founder dosages of --grid-points markers over 20 chromosomes and 8
founders, an intercept and a 0/1 covariate, standard normal phenotypes.  One GenomeScan per sample count.  Recorded per
(sample count, phenotypes), from the second of two calls of GenomeScan.permute:

  permute_ms, product_ms   device time of the whole pass and of its product kernel alone (gbrs_scan_perm_info)
  permute_wall_ms          host clock around permute(): the check and upload of the phenotypes, the pass, perm_max copied out
  tflops                   2 M Hp n_ld P B over product_ms, the matrix pipe's rate as in scan_bench.py
  peak_device_bytes        what the handle held during the pass

  host_permuted route: what the scan offered before the pass existed - the phenotype table permuted on the host and one
  GenomeScan.run(want_lod=False) per permutation, the maximum taken from the peaks.  --host-perms permutations are timed
  (host clock, the permuting included) and the time is scaled linearly to --perms; the record says so.  This route
  permutes the phenotypes, not the residuals, so with a covariate its maxima are another test's: only the time is
  compared."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="64,512")
    ap.add_argument("--phenotypes", default="1,64,1024")
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--grid-points", type=int, default=64_000)
    ap.add_argument("--host-perms", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_perm_bench.json"))
    a = ap.parse_args()
    from gbrs_amd.scan import GenomeScan, perm_thresholds
    H, n_chrom, M, B = 8, 20, a.grid_points, a.perms
    points = [M // n_chrom + (M % n_chrom if k == 0 else 0) for k in range(n_chrom)]
    counts = [int(x) for x in a.samples.split(",") if x]
    phenos = [int(x) for x in a.phenotypes.split(",") if x]
    result = dict(grid_points=M, founders=H, permutations=B, cpus=os.environ.get("OMP_NUM_THREADS", "not set"), cohorts={})
    rng = np.random.default_rng(28)
    for n in counts:
        D = rng.random((n, M, H))
        D /= D.sum(axis=2, keepdims=True)
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        Y = rng.standard_normal((n, max(phenos)))
        scan = GenomeScan(H, points)
        scan.append(D)
        del D
        scan.prepare(Z)
        n_ld = (n + 31) // 32 * 32
        cohort = dict(prepare_ms=round(scan.info()["prepare_ms"], 3), passes={})
        for P in phenos:
            y = np.ascontiguousarray(Y[:, :P])
            scan.permute(y, min(B, 8), seed=28)                  # the first call of a shape pays the kernels' loading
            t0 = time.perf_counter()
            got = scan.permute(y, B, seed=28)
            wall = time.perf_counter() - t0
            info = scan.perm_info()
            flops = 2.0 * M * 8 * n_ld * P * B
            entry = dict(permute_ms=round(info["permute_ms"], 3), product_ms=round(info["product_ms"], 3),
                         permute_wall_ms=round(wall * 1e3, 3), columns=P * B, tflops=round(flops / info["product_ms"] / 1e9, 3),
                         product_share=round(info["product_ms"] / info["permute_ms"], 4), peak_device_bytes=info["peak_device_bytes"],
                         median_threshold_0_05=float(np.median(perm_thresholds(got["perm_max"], [0.05]))))
            scan.run(y, want_lod=False)
            order = np.random.default_rng(1)
            t0 = time.perf_counter()
            for _ in range(a.host_perms):
                peak = scan.run(y[order.permutation(n)], want_lod=False)["peak_lod"]
                np.nanmax(peak, axis=1)
            host = time.perf_counter() - t0
            entry["host_permuted"] = dict(permutations_timed=a.host_perms, measured_wall_ms=round(host * 1e3, 3),
                                          scaled_to_permutations=B, scaled_wall_ms=round(host * 1e3 * B / a.host_perms, 1),
                                          note="one GenomeScan.run(want_lod=False) per host-permuted phenotype table; timed on "
                                               "permutations_timed permutations and scaled linearly to all of them")
            entry["wall_ratio_host_over_device"] = round(host * B / a.host_perms / wall, 2)
            cohort["passes"][str(P)] = entry
            print(f"{n} samples x {P} phenotypes x {B} permutations: {entry}", flush=True)
        scan.close()
        result["cohorts"][str(n)] = cohort
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
