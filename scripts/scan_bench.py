#!/usr/bin/env python3
"""The genome scan (`gbrs reconstruct --scan-pheno`) at eQTL size, against the host route.

    python scripts/scan_bench.py [--samples 64,512] [--phenotypes 1,1024,20000] [--grid-points 64000] [--out profiles/scan_bench.json]

Inputs: random founder dosages (rows that add up to 1) of --grid-points markers over 20 chromosomes and 8 founders,
an intercept and a 0/1 covariate, standard normal phenotypes.  One GenomeScan per sample count.  Recorded per sample count:

  append_s           host clock of append() for the whole cohort (the upload and its check for values that are not finite)
  prepare_ms         device time of the prepare kernel (gbrs_scan_info)
  prepare_wall_ms    host clock around prepare(): the QR of the covariates, the kernel and the ranks copied out

and per (sample count, phenotypes):

  run_ms, product_ms device time of the whole run and of its product kernel alone, the second of two calls
  run_wall_ms        host clock around run(): the check of the phenotypes, the chunks, the copies out
  lod_matrix         whether the P x M LOD matrix was copied out (not above --lod-limit values: peaks only beyond that)
  tflops             2 M Hp n_ld P over product_ms; Hp = 8 rows per grid point and n_ld = n rounded up to 32 are what the
                     kernel multiplies, so this is the matrix pipe's rate, not the useful 2 M 7 n P
  lod_store_gb_s     8 M P bytes of LODs over product_ms
  bound              which of the two floors is higher for the product kernel: the f64 matrix pipe at its peak or the LOD
                     stores at the chip's 8 TB/s

  host route, at --host-points grid points and --host-phenotypes phenotypes on this job's CPUs, scaled linearly to the
  full grid and phenotype count (said so in the record): the dosages as hmm.grid() returns them, X~ by one matmul,
  numpy's batched QR of the (n x 7) designs, and ess = |Q_m' Y~|^2 by batched matmul.  The LODs of the points it covers
  are compared with the device's."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8.0e12
F64_MFMA_FLOPS = 256 * 4 * 2048 / 64 * 2.4e9


def host_route(D, Z, Y):
    """LODs [P, m] of the grid points in D [n, m, H] by batched numpy."""
    n, m, H = D.shape
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    rss0 = (Yt * Yt).sum(axis=0)
    X = np.ascontiguousarray(D[:, :, :H - 1].transpose(1, 0, 2))          # [m, n, H - 1]
    Xt = X - Q @ (Q.T @ X)
    Qm = np.linalg.qr(Xt)[0]                                               # batched
    ess = ((Qm.transpose(0, 2, 1) @ Yt) ** 2).sum(axis=1)                  # [m, P]
    return (0.5 * n * np.log10(rss0 / (rss0 - ess))).T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="64,512")
    ap.add_argument("--phenotypes", default="1,1024,20000")
    ap.add_argument("--grid-points", type=int, default=64_000)
    ap.add_argument("--host-points", type=int, default=4000)
    ap.add_argument("--host-phenotypes", type=int, default=1024)
    ap.add_argument("--lod-limit", type=int, default=1 << 27)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_bench.json"))
    a = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    H, n_chrom, M = 8, 20, a.grid_points
    points = [M // n_chrom + (M % n_chrom if k == 0 else 0) for k in range(n_chrom)]
    counts = [int(x) for x in a.samples.split(",") if x]
    phenos = [int(x) for x in a.phenotypes.split(",") if x]
    result = dict(grid_points=M, founders=H, cpus=os.environ.get("OMP_NUM_THREADS", "not set"),
                  hbm_peak_tb_s=HBM_BYTES_PER_S / 1e12, f64_mfma_peak_tflops=round(F64_MFMA_FLOPS / 1e12, 1), cohorts={})
    rng = np.random.default_rng(27)
    for n in counts:
        t0 = time.perf_counter()
        D = rng.random((n, M, H))
        D /= D.sum(axis=2, keepdims=True)
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        Y = rng.standard_normal((n, max(phenos)))
        make_s = time.perf_counter() - t0
        scan = GenomeScan(H, points)
        t0 = time.perf_counter()
        scan.append(D)
        append_s = time.perf_counter() - t0
        scan.prepare(Z)
        t0 = time.perf_counter()
        scan.prepare(Z)
        prepare_wall = time.perf_counter() - t0
        info = scan.info()
        n_ld = (n + 31) // 32 * 32
        cohort = dict(make_inputs_s=round(make_s, 2), append_s=round(append_s, 3), prepare_ms=round(info["prepare_ms"], 3),
                      prepare_wall_ms=round(prepare_wall * 1e3, 3), full_rank_points=int((info["rank"] == H - 1).sum()),
                      prepare_bytes=8.0 * M * (n * H + 8 * n_ld), runs={})
        cohort["prepare_gb_s"] = round(cohort["prepare_bytes"] / info["prepare_ms"] / 1e6, 1)
        for P in phenos:
            y = np.ascontiguousarray(Y[:, :P])
            want_lod = P * M <= a.lod_limit
            scan.run(y, want_lod=want_lod)
            t0 = time.perf_counter()
            got = scan.run(y, want_lod=want_lod)
            wall = time.perf_counter() - t0
            info = scan.info()
            flops = 2.0 * M * 8 * n_ld * P
            stores = 8.0 * M * P
            mfma_floor, store_floor = flops / F64_MFMA_FLOPS * 1e3, stores / HBM_BYTES_PER_S * 1e3
            entry = dict(run_ms=round(info["run_ms"], 3), product_ms=round(info["product_ms"], 3), run_wall_ms=round(wall * 1e3, 3),
                         lod_matrix=want_lod, flops=flops, useful_flops=2.0 * M * (H - 1) * n * P,
                         tflops=round(flops / info["product_ms"] / 1e9, 3), lod_store_gb_s=round(stores / info["product_ms"] / 1e6, 1),
                         mfma_floor_ms=round(mfma_floor, 4), store_floor_ms=round(store_floor, 4),
                         bound="matrix pipe" if mfma_floor > store_floor else "LOD stores",
                         share_of_floor=round(max(mfma_floor, store_floor) / info["product_ms"], 4),
                         device_bytes=info["device_bytes"])
            cohort["runs"][str(P)] = entry
            print(f"{n} samples x {P} phenotypes: {entry}", flush=True)
            if P == min(a.host_phenotypes, max(phenos)) and want_lod:
                m = min(a.host_points, M)
                t0 = time.perf_counter()
                lod = host_route(D[:, :m], Z, y)
                host_s = time.perf_counter() - t0
                fin = np.isfinite(lod)
                worst = float(np.max(np.abs(got["lod"][:, :m][fin] - lod[fin]) / np.maximum(1.0, np.abs(lod[fin]))))
                scale = M / m
                cohort["host_route"] = dict(points=m, phenotypes=P, measured_s=round(host_s, 3), scaled_to_points=M,
                                            scaled_s=round(host_s * scale, 2),
                                            scaled_to_20000_phenotypes_s=round(host_s * scale * 20000 / P, 1),
                                            note="measured on the first grid points and scaled linearly to the whole grid; the "
                                                 "20000-phenotype figure scales the whole time by the phenotype count, which "
                                                 "overstates the QR's share",
                                            device_prepare_plus_run_wall_ms=round(prepare_wall * 1e3 + wall * 1e3, 2),
                                            max_deviation=worst)
                print(f"{n} samples: host route {cohort['host_route']}", flush=True)
        scan.close()
        del D
        result["cohorts"][str(n)] = cohort
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
