#!/usr/bin/env python
"""The mixed-model genome scan at size: M = 64,000 grid points on 20 chromosomes, H = 8, two covariate
columns, leave-one-chromosome-out kinship; 64 and 512 samples; P = 1, 64 and 1,024 phenotypes.  Per cohort size:
  kinship   the device time of the first GenomeScan.kinship (the 20 products S_c and one sum) and of a later one (the sum)
  rotate    the device time of prepare_lmm's rotations (the covariates and the cohort, 20 decompositions), the second of two
            calls, and the wall-clock time of numpy's 20 eigendecompositions beside it
  run       per P: the device times of the null fits and of the weighted scan (gbrs_scan_lmm_info, the second of two calls)
            and, beside them, the plain gbrs_scan_run of the same phenotypes on the same cohort: what the mixed model costs
            over Haley-Knott
  host      the numpy route in the same job on its CPUs: rotate, fit (the restatement's search), and a weighted batched QR
            of [Z^ | X^_m] per (phenotype, grid point) - timed on a slice of the phenotypes and of the grid points and
            scaled linearly (`host_scaled`).
Writes profiles/scan_lmm_bench.json.

    python scripts/scan_lmm_bench.py [--out profiles/scan_lmm_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def host_route(D, Z, Y, U, lam, points):
    """(seconds rotating, fitting, scanning) for the phenotypes Y on the grid points `points`, all with one decomposition."""
    import scan_lmm_cases as restatement
    n, H = D.shape[0], D.shape[2]
    t0 = time.perf_counter()
    Zs, Ys = U.T @ Z, U.T @ Y
    R = np.einsum('si,smj->mij', U, D[:, points, :H - 1])
    t1 = time.perf_counter()
    hsq = [restatement.search(Ys[:, p], Zs, lam)[0] for p in range(Y.shape[1])]
    t2 = time.perf_counter()
    lod = np.empty((Y.shape[1], len(points)))
    for p, h in enumerate(hsq):
        sw = np.sqrt(1.0 / (h * lam + (1.0 - h)))
        Zh, yh = sw[:, None] * Zs, sw * Ys[:, p]
        q0 = np.linalg.qr(Zh)[0]
        rss0 = yh @ yh - ((q0.T @ yh) ** 2).sum()
        A = np.concatenate([np.broadcast_to(Zh, (len(points),) + Zh.shape), sw[None, :, None] * R], axis=2)
        q = np.linalg.qr(A)[0]
        rss1 = yh @ yh - (np.einsum('mik,i->mk', q, yh) ** 2).sum(axis=1)
        lod[p] = 0.5 * n * np.log10(rss0 / rss1)
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, np.asarray(hsq), lod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_lmm_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid: a rehearsal')
    ap.add_argument('--host-phenotypes', type=int, default=4)
    ap.add_argument('--host-points', type=int, default=256)
    args = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    n_chrom, per_chrom, H, cz = 20, 3200 // (50 if args.quick else 1), 8, 2
    M = n_chrom * per_chrom
    rng = np.random.default_rng(32)
    t0 = time.perf_counter()
    D = rng.random((512, M, H))
    D /= D.sum(axis=2, keepdims=True)
    print(f'cohort of 512 x {M} x {H} made in {time.perf_counter() - t0:.1f} s', flush=True)
    cpus = int(os.environ['OMP_NUM_THREADS']) if 'OMP_NUM_THREADS' in os.environ else os.cpu_count()
    results = []
    for n in (64, 512):
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        K0 = scan.kinship(0)
        first_ms = scan.lmm_info()['kinship_ms']
        scan.kinship(1)
        record = dict(what='kinship', n=n, M=M, H=H, products_and_sum_ms=first_ms, sum_ms=scan.lmm_info()['kinship_ms'],
                      flops=2.0 * n * n * M * H)
        results.append(record)
        print(json.dumps(record), flush=True)
        w0 = time.perf_counter()
        np.linalg.eigh(K0)
        eigh_ms = 1e3 * (time.perf_counter() - w0)
        for _ in range(2):
            matrices = scan.prepare_lmm(Z)
        record = dict(what='rotate', n=n, M=M, H=H, cz=cz, n_eig=n_chrom, rotate_ms=scan.lmm_info()['rotate_ms'],
                      flops=2.0 * n * n * M * (H - 1), host_eigh_ms_each=eigh_ms, device_bytes=scan.lmm_info()['device_bytes'])
        record['tflops'] = record['flops'] / (record['rotate_ms'] * 1e-3) / 1e12
        results.append(record)
        print(json.dumps(record), flush=True)
        scan.prepare(Z)
        lam, U = np.linalg.eigh(matrices[0])
        root = np.linalg.cholesky(matrices[0] / np.mean(np.diag(matrices[0])))
        for P in (1, 64, 1024):
            Y = np.sqrt(0.5) * (root @ rng.normal(size=(n, P))) + np.sqrt(0.5) * rng.normal(size=(n, P))
            for _ in range(2):
                w0 = time.perf_counter()
                got = scan.run_lmm(Y, want_lod=False)
                wall = time.perf_counter() - w0
            info = scan.lmm_info()
            for _ in range(2):
                scan.run(Y, want_lod=False)
            plain = scan.info()
            kp, km = min(args.host_phenotypes, P), min(args.host_points, per_chrom)
            points = np.arange(km)                              # chromosome 0: decomposition 0
            rot_s, fit_s, scan_s, hsq, lod = host_route(D[:n], Z, Y[:, :kp] - Y[:, :kp].mean(axis=0), U, lam, points)
            check = scan.run_lmm(Y[:, :kp], want_lod=True)
            record = dict(what='run', n=n, M=M, H=H, cz=cz, P=P, null_ms=info['null_ms'], point_ms=info['point_ms'],
                          run_ms=info['run_ms'], wall_ms=1e3 * wall, peak_device_bytes=info['peak_device_bytes'],
                          point_us_per_pair=1e3 * info['point_ms'] / (P * M), plain_run_ms=plain['run_ms'],
                          plain_product_ms=plain['product_ms'], plain_prepare_ms=plain['prepare_ms'],
                          mixed_over_plain=info['run_ms'] / plain['run_ms'], mean_hsq=float(got['hsq'].mean()),
                          host_phenotypes=int(kp), host_points=int(km), host_cpus=cpus,
                          host_rotate_ms=1e3 * rot_s * M / km, host_fit_ms=1e3 * fit_s * P * n_chrom / kp,
                          host_scan_ms=1e3 * scan_s * (P / kp) * (M / km), host_scaled=True,
                          worst_hsq_difference_on_slice=float(np.abs(check['hsq'][:, 0] - hsq).max()),
                          worst_lod_difference_on_slice=float(np.abs(check['lod'][:, :km] - lod).max()))
            record['host_over_device'] = (record['host_fit_ms'] + record['host_scan_ms']) / info['run_ms']
            results.append(record)
            print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'mixed-model genome scan, device times from events (the second of two calls); plain_*: gbrs_scan_run and '
                           'gbrs_scan_prepare on the same cohort and phenotypes; host route: numpy on a slice of the phenotypes and '
                           'of the grid points of one chromosome, scaled linearly to P phenotypes, M grid points and n_eig fits per '
                           'phenotype',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
