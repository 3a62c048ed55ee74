#!/usr/bin/env python3
"""Wall clock of `get-common-alignments`, `combine`, `pull-out-unique-reads` and `stencil` on a generated sample.

  1. a child process writes the sample: the bench generator's reads (gbrs_amd/synth_torch.py) as the first end, and a
     second end made from it by dropping about a third of the entries and adding 0.2 % random ones (seeded), plus a
     group file and a genotype file with a two-haplotype call per gene;
  2. every command runs as a fresh process (`python -m gbrs_amd <command>`); its stage times come from
     GBRS_STAGE_TIMES: load, upload (gbrs_matops_create), kernels (the edit calls; for the two-file commands they
     include the upload of the second operand), download, write;
  3. one separate run per command under `rocprofv3 --kernel-trace --stats` for the per-kernel device times;
  4. for orientation only: the numpy restatement (tests/matops_restate.py) on one core on a row subsample, scaled
     linearly to the full row count and labelled as scaled.

Prints one JSON object.  Needs an MI355X.  Usage:
    python scripts/matops_bench.py [--reads N] [--haps H] [--loci L] [--format h5|npz] [--workdir DIR] [--keep]
                                   [--no-profile] [--numpy-rows N] [--json OUT]
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


def make_sample(workdir, rows, haps, loci, fmt, sub_rows):
    import numpy as np
    import torch
    from gbrs_amd import synth, synth_torch
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    prob = synth_torch.make_em_problem_device(rows, haps, loci, synth.SEED_BASE_EM + 1, 'cuda:0')
    ip = [t.cpu().numpy().view(np.uint32) for t in prob['indptr']]
    ix = [t.cpu().numpy().view(np.uint32) for t in prob['indices']]
    starts = [int(s) for s in prob['gene_starts']]
    del prob
    torch.cuda.empty_cache()
    lname = [f'T{l:07d}' for l in range(loci)]
    hname = [chr(65 + h) for h in range(haps)]
    rng = np.random.default_rng(20)
    ipb, ixb = [], []
    for h in range(haps):
        col = np.repeat(np.arange(loci, dtype=np.int64), np.diff(ip[h].astype(np.int64)))
        keys = col * rows + ix[h]
        keys = keys[rng.random(len(keys)) >= 1 / 3]
        n_add = max(1, int(0.002 * len(ix[h])))
        keys = np.unique(np.concatenate((keys, rng.integers(0, loci, n_add) * rows + rng.integers(0, rows, n_add))))
        ipb.append(np.searchsorted(keys // rows, np.arange(loci + 1)).astype(np.uint32))
        ixb.append((keys % rows).astype(np.uint32))
    out = dict(entries_a=int(sum(len(i) for i in ix)), entries_b=int(sum(len(i) for i in ixb)), write_s={})
    for tag, (p, i) in (('a', (ip, ix)), ('b', (ipb, ixb))):
        t0 = time.perf_counter()
        path = os.path.join(workdir, f'{tag}.{fmt}')
        AlignmentPropertyMatrix(shape=(loci, haps, rows), indptr=p, indices=i, haplotype_names=hname,
                                locus_names=lname).save(path)
        out[tag], out['write_s'][tag] = path, round(time.perf_counter() - t0, 2)
    bounds = starts + [loci]
    out['groups'] = os.path.join(workdir, 'ref.gene2transcripts.tsv')
    out['genotypes'] = os.path.join(workdir, 'genotypes.tsv')
    calls = rng.integers(0, haps, size=(len(starts), 2))
    with open(out['groups'], 'w') as g, open(out['genotypes'], 'w') as t:
        t.write('#Gene_ID\tDiplotype\n')
        for k in range(len(starts)):
            g.write(f'G{k:07d}\t' + '\t'.join(lname[bounds[k]:bounds[k + 1]]) + '\n')
            t.write(f'G{k:07d}\t{hname[calls[k, 0]]}{hname[calls[k, 1]]}\n')
    if sub_rows:
        # rows [0, sub_rows) of both ends for the one-core restatement
        sub = {}
        for tag, (p, i) in (('a', (ip, ix)), ('b', (ipb, ixb))):
            for h in range(haps):
                col = np.repeat(np.arange(loci, dtype=np.int64), np.diff(p[h].astype(np.int64)))
                sel = i[h] < sub_rows
                sub[f'{tag}_indptr{h}'] = np.searchsorted(col[sel], np.arange(loci + 1)).astype(np.uint32)
                sub[f'{tag}_indices{h}'] = i[h][sel]
        group = np.full(loci, -1, dtype=np.int32)
        for k in range(len(starts)):
            group[bounds[k]:bounds[k + 1]] = k
        allowed = np.zeros(loci, dtype=np.uint32)
        allowed[group >= 0] = ((1 << calls[:, 0]) | (1 << calls[:, 1])).astype(np.uint32)[group[group >= 0]]
        out['sub'] = os.path.join(workdir, 'sub.npz')
        np.savez(out['sub'], locus_group=group, allowed=allowed, **sub)
    print(json.dumps(out), flush=True)


def numpy_seconds(path, sub_rows, haps, loci):
    import numpy as np
    import matops_restate as rs
    z = np.load(path)
    a = ([z[f'a_indptr{h}'] for h in range(haps)], [z[f'a_indices{h}'] for h in range(haps)])
    b = ([z[f'b_indptr{h}'] for h in range(haps)], [z[f'b_indices{h}'] for h in range(haps)])
    out = {}
    for name, fn in (('get-common-alignments', lambda: rs.intersect(sub_rows, loci, haps, a, b)),
                     ('combine', lambda: rs.append_rows(sub_rows, sub_rows, loci, haps, a, b)),
                     ('pull-out-unique-reads', lambda: rs.keep_rows(sub_rows, loci, haps, a[0], a[1], rs.unique_rows(
                         sub_rows, loci, haps, a[0], a[1], z['locus_group'], False))),
                     ('stencil', lambda: rs.mask_columns(sub_rows, loci, haps, a[0], a[1], z['allowed']))):
        t0 = time.perf_counter()
        fn()
        out[name] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=40_000_000)
    ap.add_argument('--haps', type=int, default=8)
    ap.add_argument('--loci', type=int, default=120_000)
    ap.add_argument('--format', default='h5', choices=('npz', 'h5'))
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--numpy-rows', type=int, default=1_000_000, help='rows of the one-core restatement (0 = skip)')
    ap.add_argument('--json', default=None)
    ap.add_argument('--make-sample', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    workdir = args.workdir or tempfile.mkdtemp(prefix='matops_bench_')
    os.makedirs(workdir, exist_ok=True)
    sub_rows = min(args.numpy_rows, args.reads)
    if args.make_sample:
        make_sample(workdir, args.reads, args.haps, args.loci, args.format, sub_rows)
        return 0
    from bam2emase_bench import kernel_stats
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--make-sample', '--workdir', workdir, '--reads',
                        str(args.reads), '--haps', str(args.haps), '--loci', str(args.loci), '--format', args.format,
                        '--numpy-rows', str(sub_rows)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(json.dumps(dict(failed='make-sample', stderr=r.stderr[-800:])), flush=True)
        return 1
    s = json.loads(r.stdout.strip().splitlines()[-1])
    res = dict(reads=args.reads, haps=args.haps, loci=args.loci, format=args.format, entries_a=s['entries_a'],
               entries_b=s['entries_b'], generate_s=round(time.time() - t0, 1), sample_write_s=s['write_s'],
               input_bytes=dict(a=os.path.getsize(s['a']), b=os.path.getsize(s['b'])), commands={})
    out = os.path.join(workdir, f'out.{args.format}')
    stage_file = os.path.join(workdir, 'stages.json')
    commands = {
        'get-common-alignments': ['-i', s['a'], '-i', s['b'], '-o', out],
        'combine': ['-i', s['a'], '-i', s['b'], '-o', out],
        'pull-out-unique-reads': ['-i', s['a'], '-g', s['groups'], '-o', out],
        'stencil': ['-i', s['a'], '-G', s['genotypes'], '-g', s['groups'], '-o', out],
    }
    for name, argv in commands.items():
        cmd = [sys.executable, '-m', 'gbrs_amd', name] + argv
        e = dict(env, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()))
        t0 = time.time()
        r = subprocess.run(cmd, env=e, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        wall = time.time() - t0
        with open(stage_file) as fh:
            st = json.load(fh)
        if r.returncode != 0 or 'error' in st or not os.path.exists(out):
            res['commands'][name] = dict(failed=st.get('error', r.stderr[-500:]))
            print(json.dumps(res), flush=True)
            return 1
        row = dict(wall_s=round(wall, 3), output_bytes=os.path.getsize(out),
                   stages_s={k: round(st[k], 4) for k in ('load', 'upload', 'kernels', 'download', 'write') if k in st})
        os.remove(out)
        print(f'[matops_bench] {name}: {row}', file=sys.stderr, flush=True)
        if not args.no_profile and shutil.which('rocprofv3'):
            prof = os.path.join(workdir, 'prof_' + name)
            e = dict(env, GBRS_ORDERLY_EXIT='1')                              # the tracer writes at exit
            r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '--'] + cmd,
                               env=e, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            row['profile_rc'] = r.returncode
            row['kernels'] = kernel_stats(prof)
            row['device_ms_total'] = round(sum(v['ms'] for v in row['kernels'].values()), 3)
            if os.path.exists(out):
                os.remove(out)
            shutil.rmtree(prof, ignore_errors=True)
            print(f'[matops_bench] {name}: device {row["device_ms_total"]} ms', file=sys.stderr, flush=True)
        res['commands'][name] = row
    if sub_rows:
        secs = numpy_seconds(s['sub'], sub_rows, args.haps, args.loci)
        res['numpy_restatement_one_core'] = dict(
            rows=sub_rows, seconds={k: round(v, 3) for k, v in secs.items()},
            scaled_to_full_s={k: round(v * args.reads / sub_rows, 1) for k, v in secs.items()},
            note='SCALED linearly from the row subsample; arrays in memory, no file read or write')
    if not args.keep and args.workdir is None:
        shutil.rmtree(workdir, ignore_errors=True)
    text = json.dumps(res)
    if args.json:
        with open(args.json, 'w') as fh:
            fh.write(text + '\n')
    print(text, flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
