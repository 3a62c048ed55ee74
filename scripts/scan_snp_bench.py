#!/usr/bin/env python
"""The SNP association pass at size: M = 64,000 grid points on 20 chromosomes, H = 8; 143,000 and 10 M
SNPs sorted by position; 64 and 512 samples; P = 1, 64 and 1,024 phenotypes, two covariate columns.  Per configuration
the device times of GenomeScan.run_snps(want_lod=False) from gbrs_scan_snp_info - the pass, the row kernel, the product
kernel; the best of `--reps` passes - beside the route that exists without it, in the same job on its CPUs: the rows of
snp_dosage computed by numpy from dosages in `DiplotypeHMM.grid()` layout, then projection, normalisation, one matmul and
the LOD formula.  The host route is timed on a slice of the SNPs and scaled linearly to the set (`host_scaled`).  Writes
profiles/scan_snp_bench.json.

    python scripts/scan_snp_bench.py [--out profiles/scan_snp_bench.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_route(D, Q, Yt, rss0, lo, hi, t, masks):
    """LODs [P, len(lo)] of a slice of SNPs by numpy."""
    n, H = D.shape[0], D.shape[2]
    bits = ((masks[:, None] >> np.arange(H, dtype=np.uint32)) & 1).astype(np.float64)
    a_lo = np.einsum('sjh,jh->sj', D[:, lo], bits)
    a_hi = np.einsum('sjh,jh->sj', D[:, hi], bits)
    X = 2.0 * (a_lo + t * (a_hi - a_lo))
    raw = (X * X).sum(axis=0)
    X -= Q @ (Q.T @ X)
    G = (X * X).sum(axis=0)
    used = (G > 0.0) & (G > 1e-10 * raw)
    X /= np.sqrt(np.where(used, G, 1.0))
    ess = (Yt.T @ X) ** 2
    with np.errstate(divide='ignore', invalid='ignore'):
        lod = 0.5 * n * np.log10(rss0[:, None] / (rss0[:, None] - ess))
    return np.where(used, lod, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/scan_snp_bench.json')
    ap.add_argument('--quick', action='store_true', help='a fiftieth of the SNPs and of the grid: a rehearsal')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--host-slice', type=int, default=20000)
    args = ap.parse_args()
    from gbrs_amd.scan import GenomeScan
    shrink = 50 if args.quick else 1
    n_chrom, per_chrom, H, c = 20, 3200 // shrink, 8, 2
    M = n_chrom * per_chrom
    rng = np.random.default_rng(29)
    t0 = time.perf_counter()
    D = rng.random((512, M, H))
    D /= D.sum(axis=2, keepdims=True)
    grid = [np.sort(rng.uniform(0.0, 100.0, size=per_chrom)) for _ in range(n_chrom)]
    print(f'cohort of 512 x {M} x {H} made in {time.perf_counter() - t0:.1f} s', flush=True)
    results = []
    for n in (64, 512):
        Z = np.column_stack([np.ones(n), rng.integers(0, 2, size=n)])
        Z[:2, 1] = (0.0, 1.0)
        Q = np.linalg.qr(Z)[0]
        Y_all = rng.normal(size=(n, 1024))
        scan = GenomeScan(H, [per_chrom] * n_chrom)
        scan.append(D[:n])
        scan.prepare(Z)
        for M_snp in (143_000 // shrink, 10_000_000 // shrink):
            counts = np.full(n_chrom, M_snp // n_chrom)
            counts[:M_snp - counts.sum()] += 1
            pos = [np.sort(rng.uniform(g[0], g[-1], size=k)) for g, k in zip(grid, counts)]
            masks = [rng.integers(1, 255, size=k).astype(np.uint32) for k in counts]
            t0 = time.perf_counter()
            scan.set_snps(grid, pos, masks)
            set_s = time.perf_counter() - t0
            # the host route's slice: the first SNPs of the first chromosome
            k = min(args.host_slice, len(pos[0]))
            at = np.searchsorted(grid[0], pos[0][:k], 'right') - 1
            lo, hi = np.clip(at, 0, per_chrom - 1), np.minimum(np.clip(at, 0, per_chrom - 1) + 1, per_chrom - 1)
            t = np.where(grid[0][hi] > grid[0][lo], (pos[0][:k] - grid[0][lo]) / np.where(grid[0][hi] > grid[0][lo], grid[0][hi] - grid[0][lo], 1.0), 0.0)
            for P in (1, 64, 1024):
                Y = np.ascontiguousarray(Y_all[:, :P])
                best = None
                for _ in range(args.reps):
                    w0 = time.perf_counter()
                    got = scan.run_snps(Y, want_lod=False)
                    wall = time.perf_counter() - w0
                    info = scan.snp_info()
                    if best is None or info['pass_ms'] < best['pass_ms']:
                        best = dict(pass_ms=info['pass_ms'], row_ms=info['row_ms'], product_ms=info['product_ms'], wall_ms=1e3 * wall,
                                    staged=info['staged'], peak_device_bytes=info['peak_device_bytes'], snp_bytes=info['device_bytes'])
                Yt = Y - Q @ (Q.T @ Y)
                rss0 = (Yt * Yt).sum(axis=0)
                h0 = time.perf_counter()
                lod = host_route(D[:n], Q, Yt, rss0, lo, hi, t, masks[0][:k])
                host_slice_ms = 1e3 * (time.perf_counter() - h0)
                # the slice also checks the pass: the device's peak over these SNPs cannot be below the host's by more than rounding
                record = dict(n=n, M=M, H=H, c=c, M_snp=int(M_snp), P=P, used=int(got['used'].sum()), set_snps_ms=1e3 * set_s,
                              host_slice=int(k), host_slice_ms=host_slice_ms, host_ms=host_slice_ms * M_snp / k,
                              host_scaled=bool(k < M_snp), host_cpus=os.cpu_count() if 'OMP_NUM_THREADS' not in os.environ
                              else int(os.environ['OMP_NUM_THREADS']), host_slice_max_lod=float(lod.max()),
                              device_max_lod=float(np.nanmax(got['peak_lod'])), **best)
                record['bound_by'] = 'row kernel' if best['row_ms'] > best['product_ms'] else 'product kernel'
                record['host_over_device'] = record['host_ms'] / best['pass_ms']
                results.append(record)
                print(json.dumps(record), flush=True)
        scan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump({'what': 'SNP association pass, device times from events (best of reps), LOD matrix not copied out (peaks and '
                           'used flags only); host route: numpy on a slice of the SNPs, scaled linearly where host_scaled',
                   'quick': bool(args.quick), 'results': results}, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
