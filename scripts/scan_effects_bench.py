#!/usr/bin/env python
"""The founder effects pass and the support intervals at size: M = 64,000 grid points on 20 chromosomes,
H = 8, two covariate columns; 64 and 512 samples; 20,000 phenotypes.  Per cohort size:
  effects   the device time (gbrs_scan_effects_info's pass, the second of two calls) for T = 1,024 and 20,000 peaks - target
            t is phenotype t at a random grid point - and for T = 1, which is the part that does not depend on T (the
            upload and projection of all P columns); the difference over the bytes a target must read (its HP rows of W,
            n_ld doubles each, and its 8 H bytes of D per sample) is the rate the gather reaches;
  run       the device time of a 20,000-phenotype GenomeScan.run (peaks only) with and without lod_drop = 1.5, alternating,
            the second of two rounds;
  host      the route that exists without the pass, in the same job on its CPUs: numpy on dosages in `DiplotypeHMM.grid()`
            layout - projection, the last column replaced, np.linalg.pinv per target, the standard errors from it - timed
            on a slice of the targets and scaled linearly (`host_scaled`).
Writes profiles/scan_effects_bench.json.

    python scripts/scan_effects_bench.py [--out profiles/scan_effects_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, the MI355X's HBM3E


def host_route(D, Qz, Yt, columns, points, c):
    """effect, se [S, H] of a slice of targets by numpy; Yt [n, P] is projected already."""
    n, H = D.shape[0], D.shape[2]
    effect, se = np.empty((len(points), H)), np.empty((len(points), H))
    for t, (p, m) in enumerate(zip(columns, points)):
        X = D[:, m, :] - Qz @ (Qz.T @ D[:, m, :])
        X[:, -1] = -X[:, :-1].sum(axis=1)
        pinv = np.linalg.pinv(X, rcond=1e-8)
        effect[t] = pinv @ Yt[:, p]
        r = Yt[:, p] - X @ effect[t]
        se[t] = np.sqrt((r @ r) / (n - c - (H - 1)) * (pinv * pinv).sum(axis=1))
    return effect, se


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_effects_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid and a tenth of the phenotypes: a rehearsal')
    ap.add_argument('--host-slice', type=int, default=256)
    args = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    n_chrom, per_chrom, H, c, drop = 20, 3200 // (50 if args.quick else 1), 8, 2, 1.5
    M = n_chrom * per_chrom
    P = 20000 // (10 if args.quick else 1)
    sizes = (1024 // (10 if args.quick else 1), P)
    rng = np.random.default_rng(31)
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
        Y = rng.normal(size=(n, P))
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        scan.prepare(Z)
        n_ld = (n + 31) // 32 * 32
        points_all = rng.integers(0, M, size=P)
        for _ in range(2):
            scan.effects(Y, [0], points_all[:1])
        fixed_ms = scan.effects_info()['pass_ms']
        Yt = Y - Qz @ (Qz.T @ Y)
        for T in sizes:
            columns, points = np.arange(T), points_all[:T]
            for _ in range(2):
                w0 = time.perf_counter()
                got = scan.effects(Y, columns, points)
                wall = time.perf_counter() - w0
            info = scan.effects_info()
            k = min(args.host_slice, T)
            h0 = time.perf_counter()
            effect, se = host_route(D[:n], Qz, Yt, columns[:k], points[:k], c)
            host_slice_ms = 1e3 * (time.perf_counter() - h0)
            scale = np.maximum(1.0, np.abs(effect).max(axis=1, keepdims=True))
            gather_bytes = T * (8 * n_ld * 8 + n * H * 8)
            targets_ms = max(info['pass_ms'] - fixed_ms, 1e-6)
            record = dict(what='effects', n=n, M=M, H=H, c=c, P=P, T=T, pass_ms=info['pass_ms'], pass_ms_at_T1=fixed_ms,
                          targets_ms=targets_ms, wall_ms=1e3 * wall, gather_bytes=gather_bytes,
                          gather_bytes_per_s=gather_bytes / (targets_ms * 1e-3),
                          share_of_hbm_peak=gather_bytes / (targets_ms * 1e-3) / HBM_PEAK,
                          peak_device_bytes=info['peak_device_bytes'], host_slice=int(k), host_slice_ms=host_slice_ms,
                          host_ms=host_slice_ms * T / k, host_scaled=bool(k < T), host_cpus=cpus,
                          worst_effect_difference_on_slice=float(np.max(np.abs(got['effect'][:k] - effect) / scale)),
                          worst_se_difference_on_slice=float(np.max(np.abs(got['se'][:k] - se))))
            record['host_over_device'] = record['host_ms'] / info['pass_ms']
            results.append(record)
            print(json.dumps(record), flush=True)
        times = {'plain': [], 'support': []}
        for _ in range(2):                                                      # alternating; the second round is reported
            scan.run(Y, want_lod=False)
            times['plain'].append((scan.info()['run_ms'], scan.info()['product_ms']))
            found = scan.run(Y, want_lod=False, lod_drop=drop)
            times['support'].append((scan.info()['run_ms'], scan.info()['product_ms']))
        record = dict(what='run', n=n, M=M, H=H, c=c, P=P, lod_drop=drop, run_ms=times['plain'][1][0], product_ms=times['plain'][1][1],
                      run_support_ms=times['support'][1][0], support_product_ms=times['support'][1][1],
                      support_extra_ms=times['support'][1][0] - times['plain'][1][0],
                      first_round=dict(run_ms=times['plain'][0][0], run_support_ms=times['support'][0][0]),
                      mean_interval_points=float((found['support_hi'] - found['support_lo']).mean()))
        results.append(record)
        print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'founder effects pass and support intervals, device times from events (the second of two calls); '
                           'gather_bytes = T (Hp n_ld 8 + n H 8): the rows of W and the dosage runs a target must read; targets_ms = '
                           'pass_ms - pass_ms_at_T1; host route: numpy pinv per target on a slice, scaled linearly where host_scaled',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
