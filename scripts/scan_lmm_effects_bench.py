#!/usr/bin/env python
"""Founder effects and support intervals under the mixed model at size, on §32's shapes: M = 64,000 grid
points on 20 chromosomes, H = 8, two covariate columns, leave-one-chromosome-out kinship; 64 and 512 samples.  Per cohort size:
  effects   the device time of GenomeScan.effects_lmm from events (gbrs_scan_lmm_effects_info, the second of two calls) for
            T = 1,024 and T = 20,000 targets over a table of 20,000 columns with the heritabilities given, split into the null
            fits (rotations + lmm_null_kernel, every decomposition of a used column) and the target chunks
  support   run_lmm at P = 64 without and with lod_drop = 1.5, alternating, three rounds: gbrs_scan_lmm_info's run_ms
  host      the numpy route (tests/scan_lmm_effects_cases.effects_lmm_rule, heritabilities given) in the same job on its
            CPUs, timed on 256 targets and scaled linearly to T (`host_scaled`)
Writes profiles/scan_lmm_effects_bench.json.

    python scripts/scan_lmm_effects_bench.py [--out profiles/scan_lmm_effects_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_lmm_effects_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid and of the table: a rehearsal')
    ap.add_argument('--host-targets', type=int, default=256)
    args = ap.parse_args()
    import scan_lmm_effects_cases as restatement
    from gbrs_amd.scan import GenomeScan
    shrink = 50 if args.quick else 1
    n_chrom, per_chrom, H, cz, columns = 20, 3200 // shrink, 8, 2, 20000 // shrink
    M = n_chrom * per_chrom
    rng = np.random.default_rng(34)
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
        matrices = scan.prepare_lmm(Z)
        root = np.linalg.cholesky(matrices[0] / np.mean(np.diag(matrices[0])))
        Y = np.sqrt(0.5) * (root @ rng.normal(size=(n, columns))) + np.sqrt(0.5) * rng.normal(size=(n, columns))
        hsq = rng.uniform(0.1, 0.9, size=(columns, n_chrom))
        for T in (1024 // shrink, columns):
            col = rng.permutation(columns)[:T].astype(np.int64)
            at = rng.integers(0, M, size=T).astype(np.int64)
            for _ in range(2):
                w0 = time.perf_counter()
                got = scan.effects_lmm(Y, col, at, hsq=hsq)
                wall = time.perf_counter() - w0
            info = scan.lmm_effects_info()
            kt = min(args.host_targets, T)
            eigs, used = {}, sorted(set((at[:kt] // per_chrom).tolist()))
            w0 = time.perf_counter()
            for c in used:
                lam, U = np.linalg.eigh(matrices[c])
                eigs[c] = (np.ascontiguousarray(U), lam)
            eigh_s = time.perf_counter() - w0
            w0 = time.perf_counter()
            want = restatement.effects_lmm_rule(D[:n], Z, Y, [per_chrom] * n_chrom, eigs, list(range(n_chrom)), col[:kt], at[:kt], hsq)
            host_s = time.perf_counter() - w0
            record = dict(what='effects', n=n, M=M, H=H, cz=cz, P=columns, T=T, columns_fitted=info['columns'], pass_ms=info['pass_ms'],
                          null_ms=info['null_ms'], target_ms=info['target_ms'], wall_ms=1e3 * wall,
                          null_share=info['null_ms'] / info['pass_ms'], target_us_each=1e3 * info['target_ms'] / T,
                          null_us_per_fit=1e3 * info['null_ms'] / (info['columns'] * n_chrom),
                          peak_device_bytes=info['peak_device_bytes'], host_targets=int(kt), host_cpus=cpus,
                          host_ms=1e3 * host_s * T / kt, host_eigh_ms_each=1e3 * eigh_s / len(used), host_scaled=True,
                          worst_effect_difference_on_slice=float(np.abs(got['effect'][:kt] - want[0]).max()),
                          worst_lod_difference_on_slice=float(np.abs(got['lod'][:kt] - want[2]).max()))
            record['host_over_device'] = record['host_ms'] / info['pass_ms']
            results.append(record)
            print(json.dumps(record), flush=True)
        P = 64
        rounds = {'without': [], 'with': []}
        for _ in range(3):
            scan.run_lmm(Y[:, :P], want_lod=False)
            rounds['without'].append(scan.lmm_info()['run_ms'])
            scan.run_lmm(Y[:, :P], want_lod=False, lod_drop=1.5)
            rounds['with'].append(scan.lmm_info()['run_ms'])
        record = dict(what='support', n=n, M=M, H=H, cz=cz, P=P, lod_drop=1.5, run_ms_without=rounds['without'], run_ms_with=rounds['with'],
                      last_with_over_without=rounds['with'][-1] / rounds['without'][-1])
        results.append(record)
        print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'founder effects and support intervals under the mixed model, device times from events (effects: the '
                           'second of two calls, heritabilities given, split into null fits and target chunks; support: run_lmm '
                           'without and with lod_drop, alternating); host route: numpy restatement on a slice of the targets, '
                           'scaled linearly to T, eigendecompositions apart',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
