#!/usr/bin/env python
"""The mediation pass at size: M = 64,000 grid points on 20 chromosomes, H = 8, two covariate columns; 64
and 512 samples; T = Q = 1,024 and 20,000 targets and mediators, K = 5, top lists only (no [T][Q] matrix leaves the
device).  Per configuration the device times of the second of two GenomeScan.mediate calls from gbrs_scan_mediate_info -
the pass and the product kernel -, the product kernel's Tflop/s (2 n_ld Q (Hp + 1) flop per target: the rows of W and the
s_yz row) against the 78.6 Tflop/s f64 matrix peak, peak device bytes, and scan_lod_kernel on the same cohort with 1,024
phenotypes as the yardstick.  Beside it the route that exists without the pass, in the same job on its CPUs: numpy on
dosages in `DiplotypeHMM.grid()` layout - projection, a QR of the point's founder columns per target, batched matmul with
the projected mediators, the same identities - timed on a slice of the targets and scaled linearly (`host_scaled`).
Writes profiles/scan_mediate_bench.json.

    python scripts/scan_mediate_bench.py [--out profiles/scan_mediate_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_MATRIX_PEAK = 78.6e12


def host_route(D, Qz, Yt, points, Zt, szz):
    """lod_med [len(points), Q] of a slice of targets by numpy; Yt [n, S] and Zt [n, Q] are projected already."""
    n = D.shape[0]
    X = np.ascontiguousarray(D[:, points, :-1].transpose(1, 0, 2))               # [S, n, H - 1]
    X -= Qz @ (Qz.T @ X)
    Qx = np.linalg.qr(X)[0]                                                       # [S, n, H - 1]
    a = np.einsum('snj,ns->sj', Qx, Yt)
    B = Qx.transpose(0, 2, 1) @ Zt                                                # [S, H - 1, Q]
    syy = (Yt * Yt).sum(axis=0)
    syz = Yt.T @ Zt
    rss1 = syy - (a * a).sum(axis=1)
    ezz = szz[None] - (B * B).sum(axis=1)
    eyz = syz - np.einsum('sj,sjq->sq', a, B)
    with np.errstate(divide='ignore', invalid='ignore'):
        rss0p = syy[:, None] - syz * syz / szz[None]
        rss1p = rss1[:, None] - eyz * eyz / ezz
        lod = 0.5 * n * np.log10(rss0p / rss1p)
    used = (szz[None] > 0) & (ezz > 1e-10 * szz[None]) & (rss0p > 1e-10 * syy[:, None])
    return np.where(used, lod, np.nan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_mediate_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid and a tenth of the targets: a rehearsal')
    ap.add_argument('--host-slice', type=int, default=128)
    args = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    n_chrom, per_chrom, H, c, K = 20, 3200 // (50 if args.quick else 1), 8, 2, 5
    M = n_chrom * per_chrom
    sizes = (1024 // (10 if args.quick else 1), 20000 // (10 if args.quick else 1))
    rng = np.random.default_rng(30)
    t0 = time.perf_counter()
    D = rng.random((512, M, H))
    D /= D.sum(axis=2, keepdims=True)
    print(f'cohort of 512 x {M} x {H} made in {time.perf_counter() - t0:.1f} s', flush=True)
    cpus = int(os.environ['OMP_NUM_THREADS']) if 'OMP_NUM_THREADS' in os.environ else os.cpu_count()
    results = []
    for n in (64, 512):
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        Qz = np.linalg.qr(Z)[0]
        Y_all = rng.normal(size=(n, max(sizes)))
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        scan.prepare(Z)
        n_ld = (n + 31) // 32 * 32
        P = 1024
        scan.run(Y_all[:, :P], want_lod=False)
        scan.run(Y_all[:, :P], want_lod=False)
        yard = scan.info()
        yard_tflops = 2.0 * M * 8 * n_ld * P / (yard['product_ms'] * 1e-3) / 1e12
        for size in sizes:
            T = Q = size
            Y = np.ascontiguousarray(Y_all[:, :T])
            points = rng.integers(0, M, size=T)
            for _ in range(2):
                w0 = time.perf_counter()
                got = scan.mediate(Y, points, Y, top=K)
                wall = time.perf_counter() - w0
            info = scan.mediate_info()
            flop = 2.0 * n_ld * Q * (8 + 1) * T
            tflops = flop / (info['product_ms'] * 1e-3) / 1e12
            Yt = Y - Qz @ (Qz.T @ Y)
            szz = (Yt * Yt).sum(axis=0)
            k = min(args.host_slice, T)
            h0 = time.perf_counter()
            lod = host_route(D[:n], Qz, Yt[:, :k], points[:k], Yt, szz)
            host_slice_ms = 1e3 * (time.perf_counter() - h0)
            first = np.nanmin(lod, axis=1)                                        # the slice also checks the pass
            record = dict(n=n, M=M, H=H, c=c, T=T, Q=Q, K=K, pass_ms=info['pass_ms'], product_ms=info['product_ms'],
                          rest_ms=info['pass_ms'] - info['product_ms'], wall_ms=1e3 * wall, product_share=info['product_ms'] / info['pass_ms'],
                          product_tflops=tflops, share_of_f64_matrix_peak=tflops * 1e12 / F64_MATRIX_PEAK,
                          scan_lod_kernel_ms=yard['product_ms'], scan_lod_kernel_tflops=yard_tflops, scan_lod_kernel_P=P,
                          peak_device_bytes=info['peak_device_bytes'], host_slice=int(k), host_slice_ms=host_slice_ms,
                          host_ms=host_slice_ms * T / k, host_scaled=bool(k < T), host_cpus=cpus,
                          worst_top_difference_on_slice=float(np.max(np.abs(got['best_lod'][:k, 0] - first))))
            if record['product_share'] < 0.5:
                record['bound_by'] = 'the [Tc][Q] stores plus selection (with the uploads and projections)'
            elif tflops >= 0.8 * yard_tflops:
                record['bound_by'] = 'the matrix pipe (as scan_lod_kernel is)'
            else:
                record['bound_by'] = 'the gathered-row loads (the product kernel is below scan_lod_kernel on dense rows)'
            record['host_over_device'] = record['host_ms'] / info['pass_ms']
            results.append(record)
            print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'mediation pass, device times from events (the second of two calls), top lists only; flop = 2 n_ld Q (Hp + 1) '
                           'per target; host route: numpy on a slice of the targets, scaled linearly where host_scaled',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
