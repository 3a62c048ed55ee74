#!/usr/bin/env python
"""SNP association under the mixed model at size: M = 64,000 grid points on 20 chromosomes, H = 8, two
covariate columns, leave-one-chromosome-out kinship; 143,000 and 10 M SNPs; 64 and 512 samples; P = 1, 64 and 1,024
phenotypes.  Per shape:
  pass      the device time of gbrs_scan_lmm_snps and of its three parts - the null fits, the dosages with their rotation,
            the product kernel - from gbrs_scan_lmm_snp_info, and the product kernel's Tflop/s, 2 M_snp P n_ld (cz + 2)
            flop, beside the 78.6 of the f64 matrix pipe; `runs` says how many calls the figures rest on (the last one's)
  plain     gbrs_scan_snps on the same SNPs and phenotypes: what the mixed model costs over the unweighted test
  host      the numpy route (tests/scan_lmm_snp_cases.snp_lmm_rule at the device's heritabilities) in the same job on its
            CPUs, timed on a slice of the phenotypes and of the SNPs of one chromosome and scaled linearly (`host_scaled`)
Writes profiles/scan_lmm_snp_bench.json.

    python scripts/scan_lmm_snp_bench.py [--out profiles/scan_lmm_snp_bench.json] [--quick] [--snps 143000,10000000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PIPE_TFLOPS = 78.6                         # f64 matrix pipe of an MI355X
POINT_NS_PER_PAIR = (14, 39)               # lmm_point_kernel per (grid point, phenotype), DESIGN.md §32: context


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_lmm_snp_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the grid and of the SNPs: a rehearsal')
    ap.add_argument('--snps', default='143000,10000000')
    ap.add_argument('--host-phenotypes', type=int, default=2)
    ap.add_argument('--host-snps', type=int, default=2048)
    args = ap.parse_args()
    import scan_lmm_snp_cases as restatement
    from gbrs_amd.scan import GenomeScan
    shrink = 50 if args.quick else 1
    n_chrom, per_chrom, H, cz = 20, 3200 // shrink, 8, 2
    M = n_chrom * per_chrom
    rng = np.random.default_rng(33)
    t0 = time.perf_counter()
    D = rng.random((512, M, H))
    D /= D.sum(axis=2, keepdims=True)
    print(f'cohort of 512 x {M} x {H} made in {time.perf_counter() - t0:.1f} s', flush=True)
    cpus = int(os.environ['OMP_NUM_THREADS']) if 'OMP_NUM_THREADS' in os.environ else os.cpu_count()
    grid = [np.linspace(0.0, 100.0, per_chrom) for _ in range(n_chrom)]
    results = []
    for n in (64, 512):
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        matrices = scan.prepare_lmm(Z)
        scan.prepare(Z)
        root = np.linalg.cholesky(matrices[0] / np.mean(np.diag(matrices[0])))
        eigs = [np.linalg.eigh(matrices[0])[::-1]]
        for total in [int(v) // shrink for v in args.snps.split(',')]:
            per = [total // n_chrom + (c < total % n_chrom) for c in range(n_chrom)]
            pos = [np.sort(rng.uniform(0.0, 100.0, size=k)) for k in per]
            masks = [rng.integers(1, 255, size=k).astype(np.uint32) for k in per]
            scan.set_snps(grid, pos, masks)
            for P in (1, 64, 1024):
                Y = np.sqrt(0.5) * (root @ rng.normal(size=(n, P))) + np.sqrt(0.5) * rng.normal(size=(n, P))
                runs = 1 if total * P * n > 2e11 else 2
                for _ in range(runs):
                    w0 = time.perf_counter()
                    got = scan.run_snps_lmm(Y, want_lod=False)
                    wall = time.perf_counter() - w0
                info = scan.lmm_snp_info()
                for _ in range(runs):
                    scan.run_snps(Y, want_lod=False)
                plain = scan.snp_info()
                n_ld = (n + 31) // 32 * 32
                flops = 2.0 * total * P * n_ld * (cz + 2)
                record = dict(what='pass', n=n, M=M, H=H, cz=cz, n_eig=n_chrom, M_snp=total, P=P, runs=runs, pass_ms=info['pass_ms'],
                              null_ms=info['null_ms'], rotate_ms=info['rotate_ms'], product_ms=info['product_ms'],
                              wall_ms=1e3 * wall, column_bytes=info['column_bytes'], peak_device_bytes=info['peak_device_bytes'],
                              product_flops=flops, product_tflops=flops / (info['product_ms'] * 1e-3) / 1e12,
                              pipe_tflops=PIPE_TFLOPS, product_ns_per_pair=1e6 * info['product_ms'] / (total * P),
                              point_kernel_ns_per_pair=list(POINT_NS_PER_PAIR), plain_pass_ms=plain['pass_ms'],
                              plain_row_ms=plain['row_ms'], plain_product_ms=plain['product_ms'],
                              plain_product_tflops=2.0 * total * P * n_ld / (plain['product_ms'] * 1e-3) / 1e12,
                              mixed_over_plain=info['pass_ms'] / plain['pass_ms'], mean_used=float(got['n_used'].sum() / (P * total)))
                kp, km = min(args.host_phenotypes, P), min(args.host_snps, per[0])
                check = scan.run_snps_lmm(Y[:, :kp], want_lod=True)
                X = scan.snp_dosage(0, km)
                w0 = time.perf_counter()
                rule = restatement.snp_lmm_rule(X, [km], Z, Y[:, :kp], eigs, [0], hsq=check['hsq'][:, :1])
                host_s = time.perf_counter() - w0
                record.update(host_phenotypes=int(kp), host_snps=int(km), host_cpus=cpus, host_scaled=True,
                              host_ms=1e3 * host_s * (P / kp) * (total / km),
                              worst_lod_difference_on_slice=float(np.abs(check['lod'][:, :km] - rule['lod']).max()))
                record['host_over_device'] = record['host_ms'] / info['pass_ms']
                results.append(record)
                print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'SNP association under the mixed model, device times from events (the last of `runs` calls); plain_*: '
                           'gbrs_scan_snps on the same SNPs and phenotypes; host route: numpy on a slice of the phenotypes and of '
                           'the SNPs of one chromosome at the device\'s heritabilities, scaled linearly to P phenotypes and M_snp '
                           'SNPs (the rotation of the slice and the null fits included)',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
