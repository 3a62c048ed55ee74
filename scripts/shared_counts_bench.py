#!/usr/bin/env python3
"""Wall clock of `count-shared-multireads-pairwise` on generated samples.

Per sample - "one_isoform" (the bench generator's reads, gbrs_amd/synth_torch.py variant "survey") and "multi_isoform"
(a read aligns to 1 + Poisson(2) isoforms of its gene):
  1. a child process writes the sample as an EMASE file plus its group file, and the rows [0, numpy-rows) as plain
     arrays for the one-core comparison;
  2. the command runs as a fresh process (`python -m gbrs_amd count-shared-multireads-pairwise --separate-outputs`); its
     stage times come from GBRS_STAGE_TIMES: load, upload (gbrs_matops_create), kernels (both gbrs_matops_shared_counts
     calls with their copies out), write (both .npz files); next to them what the library reports per level: distinct
     (read, column) entries, pairs emitted, batches, pair budget, nnz, peak device bytes of the call and the
     milliseconds between its first and last device operation;
  3. one separate run under `rocprofv3 --kernel-trace --stats` for the per-kernel device times;
  4. for orientation only: the numpy restatement (tests/shared_counts_restate.py) on one core on the row subsample,
     scaled linearly to the full row count and labelled as scaled; where scipy is installed (it is not on the GPU
     machines) also scipy's own `P.T * P` on the same subsample, labelled likewise.
Every step that uses the GPU is a child process under a `timeout` of its own, and the first failure ends the run.

Prints one JSON object.  Needs an MI355X.  Usage:
    python scripts/shared_counts_bench.py [--reads N] [--haps H] [--loci L] [--format h5|npz] [--workdir DIR] [--keep]
                                          [--samples one_isoform,multi_isoform] [--no-profile] [--numpy-rows N]
                                          [--json OUT]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

VARIANTS = {'one_isoform': 'survey', 'multi_isoform': 'multi_isoform'}
LIMITS = dict(make_sample=600, command=600, profile=900)               # seconds, per child process


def make_sample(workdir, rows, haps, loci, fmt, sub_rows, variant):
    import numpy as np
    import torch
    from gbrs_amd import synth, synth_torch
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    prob = synth_torch.make_em_problem_device(rows, haps, loci, synth.SEED_BASE_EM + 1, 'cuda:0', variant=variant)
    ip = [t.cpu().numpy().view(np.uint32) for t in prob['indptr']]
    ix = [t.cpu().numpy().view(np.uint32) for t in prob['indices']]
    starts = [int(s) for s in prob['gene_starts']]
    del prob
    torch.cuda.empty_cache()
    lname = [f'T{l:07d}' for l in range(loci)]
    hname = [chr(65 + h) for h in range(haps)]
    out = dict(entries=int(sum(len(i) for i in ix)))
    t0 = time.perf_counter()
    out['a'] = os.path.join(workdir, f'a.{fmt}')
    AlignmentPropertyMatrix(shape=(loci, haps, rows), indptr=ip, indices=ix, haplotype_names=hname,
                            locus_names=lname).save(out['a'])
    out['write_s'] = round(time.perf_counter() - t0, 2)
    bounds = starts + [loci]
    out['groups'] = os.path.join(workdir, 'ref.gene2transcripts.tsv')
    out['num_groups'] = len(starts)
    with open(out['groups'], 'w') as g:
        for k in range(len(starts)):
            g.write(f'G{k:07d}\t' + '\t'.join(lname[bounds[k]:bounds[k + 1]]) + '\n')
    if sub_rows:
        sub = {}
        for h in range(haps):
            col = np.repeat(np.arange(loci, dtype=np.int64), np.diff(ip[h].astype(np.int64)))
            sel = ix[h] < sub_rows
            sub[f'indptr{h}'] = np.searchsorted(col[sel], np.arange(loci + 1)).astype(np.uint32)
            sub[f'indices{h}'] = ix[h][sel]
        group = np.full(loci, -1, dtype=np.int32)
        for k in range(len(starts)):
            group[bounds[k]:bounds[k + 1]] = k
        out['sub'] = os.path.join(workdir, 'sub.npz')
        np.savez(out['sub'], locus_group=group, num_groups=len(starts), **sub)
    print(json.dumps(out), flush=True)


def one_core_seconds(path, sub_rows, haps, loci):
    """The restatement, and scipy's product where scipy is installed, on the row subsample: seconds per level."""
    import numpy as np
    import shared_counts_restate as rs
    z = np.load(path)
    ip, ix = [z[f'indptr{h}'] for h in range(haps)], [z[f'indices{h}'] for h in range(haps)]
    levels = dict(isoform=(None, 0), gene=(z['locus_group'], int(z['num_groups'])))
    out = dict(numpy={}, scipy={})
    for level, (grp, G) in levels.items():
        t0 = time.perf_counter()
        rs.shared_counts(sub_rows, loci, haps, ip, ix, grp, G)
        out['numpy'][level] = time.perf_counter() - t0
    try:
        import scipy.sparse as sp
    except ImportError:
        return out
    data = [sp.csc_matrix((np.ones(len(i)), i.astype(np.int64), p.astype(np.int64)), shape=(sub_rows, loci))
            for p, i in zip(ip, ix)]
    conv = sp.csc_matrix((np.ones(int((z['locus_group'] >= 0).sum())),
                          (np.flatnonzero(z['locus_group'] >= 0), z['locus_group'][z['locus_group'] >= 0])),
                         shape=(loci, int(z['num_groups'])))
    for level in levels:
        t0 = time.perf_counter()                       # emase_utils.py:142-146, after _bundle_inline for the genes
        mats = data if level == 'isoform' else [d * conv for d in data]
        hapsum = mats[0]
        for d in mats[1:]:
            hapsum = hapsum + d
        hapsum = sp.csr_matrix(hapsum)
        hapsum.data = np.ones(hapsum.nnz)
        (hapsum.transpose() * hapsum).nnz
        out['scipy'][level] = time.perf_counter() - t0
    return out


def run_sample(name, args, workdir, env, res):
    from bam2emase_bench import kernel_stats
    sub_rows = min(args.numpy_rows, args.reads)
    t0 = time.time()
    r = subprocess.run(['timeout', '-k', '10', str(LIMITS['make_sample']), sys.executable, os.path.abspath(__file__),
                        '--make-sample', '--variant', VARIANTS[name], '--workdir', workdir, '--reads', str(args.reads),
                        '--haps', str(args.haps), '--loci', str(args.loci), '--format', args.format, '--numpy-rows',
                        str(sub_rows)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        res[name] = dict(failed='make-sample', rc=r.returncode, stderr=r.stderr[-800:])
        return False
    s = json.loads(r.stdout.strip().splitlines()[-1])
    row = dict(entries=s['entries'], num_groups=s['num_groups'], generate_s=round(time.time() - t0, 1),
               sample_write_s=s['write_s'], input_bytes=os.path.getsize(s['a']))
    res[name] = row
    base = os.path.join(workdir, 'out')
    outputs = [f'{base}.isoforms.shared_read_counts.npz', f'{base}.genes.shared_read_counts.npz']
    stage_file = os.path.join(workdir, 'stages.json')
    cmd = [sys.executable, '-m', 'gbrs_amd', 'count-shared-multireads-pairwise', '-i', s['a'], '-g', s['groups'], '-o',
           base, '--separate-outputs']
    e = dict(env, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()))
    t0 = time.time()
    r = subprocess.run(['timeout', '-k', '10', str(LIMITS['command'])] + cmd, env=e, cwd=workdir, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    wall = time.time() - t0
    st = json.load(open(stage_file)) if os.path.exists(stage_file) else {}
    if r.returncode != 0 or 'error' in st or not all(os.path.exists(o) for o in outputs):
        row['failed'] = st.get('error', r.stderr[-500:])
        row['rc'] = r.returncode
        return False
    row.update(wall_s=round(wall, 3), output_bytes=[os.path.getsize(o) for o in outputs],
               stages_s={k: round(st[k], 4) for k in ('startup', 'load', 'upload', 'kernels', 'write', 'main') if k in st},
               levels={lvl: st[f'shared_counts_{lvl}'] for lvl in ('isoform', 'genes')})
    row['device_ms_both_calls'] = round(sum(v['device_ms'] for v in row['levels'].values()), 3)
    row['peak_device_bytes'] = max(v['peak_device_bytes'] for v in row['levels'].values())
    for o in outputs:
        os.remove(o)
    print(f'[shared_counts_bench] {name}: {row}', file=sys.stderr, flush=True)
    if not args.no_profile and shutil.which('rocprofv3'):
        prof = os.path.join(workdir, 'prof')
        e = dict(env, GBRS_ORDERLY_EXIT='1')                              # the tracer writes at exit
        r = subprocess.run(['timeout', '-k', '10', str(LIMITS['profile']), 'rocprofv3', '--kernel-trace', '--stats',
                            '--output-format', 'csv', '-d', prof, '--'] + cmd, env=e, cwd=workdir, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        row['profile_rc'] = r.returncode
        if r.returncode != 0:
            row['failed'] = 'profile run: ' + r.stderr[-500:]
            return False
        row['kernels'] = kernel_stats(prof)
        row['kernel_ms_total'] = round(sum(v['ms'] for v in row['kernels'].values()), 3)
        for o in outputs:
            if os.path.exists(o):
                os.remove(o)
        shutil.rmtree(prof, ignore_errors=True)
        print(f'[shared_counts_bench] {name}: kernels {row["kernel_ms_total"]} ms', file=sys.stderr, flush=True)
    if sub_rows:
        secs = one_core_seconds(s['sub'], sub_rows, args.haps, args.loci)
        scale = args.reads / sub_rows
        row['numpy_restatement_one_core'] = dict(
            rows=sub_rows, seconds={k: round(v, 3) for k, v in secs['numpy'].items()},
            scaled_to_full_s={k: round(v * scale, 1) for k, v in secs['numpy'].items()},
            note='SCALED linearly from the row subsample; arrays in memory, no file read or write')
        if secs['scipy']:
            row['scipy_product_one_core'] = dict(
                rows=sub_rows, seconds={k: round(v, 3) for k, v in secs['scipy'].items()},
                scaled_to_full_s={k: round(v * scale, 1) for k, v in secs['scipy'].items()},
                note='scipy hapsum.T * hapsum as in the reference, on this host CPU; SCALED linearly from the row subsample')
    os.remove(s['a'])
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=40_000_000)
    ap.add_argument('--haps', type=int, default=8)
    ap.add_argument('--loci', type=int, default=120_000)
    ap.add_argument('--format', default='h5', choices=('npz', 'h5'))
    ap.add_argument('--samples', default='one_isoform,multi_isoform')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--numpy-rows', type=int, default=1_000_000, help='rows of the one-core comparison (0 = skip)')
    ap.add_argument('--json', default=None)
    ap.add_argument('--make-sample', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--variant', default='survey', help=argparse.SUPPRESS)
    args = ap.parse_args()
    workdir = args.workdir or tempfile.mkdtemp(prefix='shared_counts_bench_')
    os.makedirs(workdir, exist_ok=True)
    if args.make_sample:
        make_sample(workdir, args.reads, args.haps, args.loci, args.format, min(args.numpy_rows, args.reads), args.variant)
        return 0
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = dict(reads=args.reads, haps=args.haps, loci=args.loci, format=args.format, samples={})
    ok = True
    for name in [x for x in args.samples.split(',') if x]:
        if name not in VARIANTS:
            raise SystemExit(f'unknown sample {name!r}')
        ok = run_sample(name, args, workdir, env, res['samples'])
        if not ok:
            break                                                         # nothing more is started after a failure
    if not args.keep and args.workdir is None:
        shutil.rmtree(workdir, ignore_errors=True)
    text = json.dumps(res)
    if args.json:
        with open(args.json, 'w') as fh:
            fh.write(text + '\n')
    print(text, flush=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
