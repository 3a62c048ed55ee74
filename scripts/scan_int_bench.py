#!/usr/bin/env python
"""The scan with interactive covariates at size: M = 64,000 grid points on 20 chromosomes, H = 8, k + 1
covariate columns (the intercept and the k interactive covariates, the first of them 0/1); 64 and 512 samples; k = 1 (16 rows
of W per grid point) and k = 3 (32 rows); P = 1, 1,024 and 20,000 phenotypes, peaks only.  Per (n, k, P), from one job:
  int       gbrs_scan_int_prepare's device ms, gbrs_scan_int_run's device ms, its product kernel's ms and Tflop/s
            (2 M HPI n_ld P flops: the zero rows are multiplied like the others), the second of two calls;
  plain     gbrs_scan_prepare / gbrs_scan_run on the same cohort, covariates and phenotypes: the same figures, with
            2 M Hp n_ld P flops, so the two product kernels stand side by side;
  host      the route that exists without the device, in the same job on its CPUs: numpy - the covariates projected out of
            [X | X z] per grid point, two np.linalg.lstsq per point for all P phenotypes - timed on a slice of the grid
            points and scaled linearly (`host_scaled`).
Writes profiles/scan_int_bench.json.

    python scripts/scan_int_bench.py [--out profiles/scan_int_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_route(D, Z, zint, Y, points):
    """lod_full, lod_int [P, S] of a slice of grid points by numpy."""
    n, H = D.shape[0], D.shape[2]
    Q = np.linalg.qr(Z)[0]
    Yt = Y - Q @ (Q.T @ Y)
    rss0 = (Yt * Yt).sum(axis=0)
    full, inter = np.empty((Y.shape[1], len(points))), np.empty((Y.shape[1], len(points)))
    for t, m in enumerate(points):
        X = D[:, m, :H - 1]
        A = np.hstack([X] + [X * zint[:, q:q + 1] for q in range(zint.shape[1])])
        A = A - Q @ (Q.T @ A)
        rss = []
        for cols in (A[:, :H - 1], A):
            r = Yt - cols @ np.linalg.lstsq(cols, Yt, rcond=1e-10)[0]
            rss.append((r * r).sum(axis=0))
        full[:, t] = 0.5 * n * np.log10(rss0 / rss[1])
        inter[:, t] = 0.5 * n * np.log10(rss[0] / rss[1])
    return full, inter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_int_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid and a tenth of the phenotypes: a rehearsal')
    ap.add_argument('--host-slice', type=int, default=16)
    args = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    n_chrom, per_chrom, H = 20, 3200 // (50 if args.quick else 1), 8
    M = n_chrom * per_chrom
    sizes = [1, 1024 // (10 if args.quick else 1), 20000 // (10 if args.quick else 1)]
    rng = np.random.default_rng(35)
    t0 = time.perf_counter()
    D = rng.random((512, M, H))
    D /= D.sum(axis=2, keepdims=True)
    print(f'cohort of 512 x {M} x {H} made in {time.perf_counter() - t0:.1f} s', flush=True)
    cpus = int(os.environ['OMP_NUM_THREADS']) if 'OMP_NUM_THREADS' in os.environ else os.cpu_count()
    results = []
    for n in (64, 512):
        n_ld = (n + 31) // 32 * 32
        Yall = rng.normal(size=(n, sizes[-1]))
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        for k in (1, 3):
            Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)] + [rng.normal(size=n) for _ in range(k - 1)])
            Z[:2, 1] = (0.0, 1.0)
            scan.prepare(Z)
            scan.prepare_int(Z, list(range(1, 1 + k)))
            hpi = scan.int_info()['HPI']
            for P in sizes:
                Y = np.ascontiguousarray(Yall[:, :P])
                for _ in range(2):
                    w0 = time.perf_counter()
                    got = scan.run_int(Y, want_lod=False)
                    wall = time.perf_counter() - w0
                info = scan.int_info()
                for _ in range(2):
                    plain = scan.run(Y, want_lod=False)
                base = scan.info()
                points = rng.integers(0, M, size=min(args.host_slice, M))
                cols = min(P, 64)                   # the device's own matrices at the slice, from a run of a few columns
                mats = scan.run_int(Y[:, :cols])
                h0 = time.perf_counter()
                full, inter = host_route(D[:n], Z, Z[:, 1:1 + k], Y, points)
                host_slice_ms = 1e3 * (time.perf_counter() - h0)
                flops, flops_plain = 2.0 * M * hpi * n_ld * P, 2.0 * M * 8 * n_ld * P
                record = dict(n=n, M=M, H=H, c=1 + k, k=k, HPI=hpi, P=P, prepare_ms=info['prepare_ms'], run_ms=info['run_ms'],
                              product_ms=info['product_ms'], product_tflops=flops / (info['product_ms'] * 1e-3) / 1e12,
                              wall_ms=1e3 * wall, device_bytes=info['device_bytes'],
                              plain_prepare_ms=base['prepare_ms'], plain_run_ms=base['run_ms'], plain_product_ms=base['product_ms'],
                              plain_product_tflops=flops_plain / (base['product_ms'] * 1e-3) / 1e12,
                              host_slice=int(len(points)), host_slice_ms=host_slice_ms, host_ms=host_slice_ms * M / len(points),
                              host_scaled=bool(len(points) < M), host_cpus=cpus,
                              worst_lod_full_difference_on_slice=float(np.max(np.abs(mats['lod_full'][:, points] - full[:cols]))),
                              worst_lod_int_difference_on_slice=float(np.max(np.abs(mats['lod_int'][:, points] - inter[:cols]))),
                              peak_full_add_equals_plain_peak_where_indices_agree=bool(
                                  (got['peak_full_add'] == plain['peak_lod'])[got['peak_full_index'] == plain['peak_index']].all()))
                record['host_over_device'] = record['host_ms'] / (info['prepare_ms'] + info['run_ms'])
                results.append(record)
                print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'scan with interactive covariates against the plain scan of the same cohort, device times from events '
                           '(the second of two calls); product flops = 2 M rows n_ld P with rows = HPI (int) or Hp = 8 (plain), zero '
                           'rows included; host route: numpy lstsq per grid point on a slice of points, scaled linearly',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
