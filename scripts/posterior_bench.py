#!/usr/bin/env python3
"""What `gbrs quantify -w --posterior-values` costs at BASELINE configs[1] size (40M reads x 8 haplotypes x 120k
isoforms, 361M stored entries), multiread models 4 and 3.

  1. a child process writes the bench generator's sample as an EMASE `.h5` with its group and length files
     (scripts/e2e_bench.py build_sample);
  2. a child process (`--library`) loads the file, and per model builds an EMfactory with keep_posterior, takes three
     steps and measures: the H posterior() calls (passes + copy out, per haplotype; the first call of model 4 also
     makes the per-read denominators), a device-to-host copy of one haplotype's bytes alone, and - model 4 only, the
     file does not depend on the model - export_posterior_probability(values=True) split into fetching the values and
     writing the `.h5`; the device memory a handle takes with and without GBRS_EM_POSTERIOR; the time of an EM step with
     and without the flag;
  3. the same child once more under `rocprofv3 --kernel-trace --stats` (no export) for the device time of the passes;
  4. the command as a fresh process, `-w` alone and `-w --posterior-values`: wall and its `reports` stage.
Every step that uses the GPU is a child process under a `timeout` of its own, and the first failure ends the run.

Prints one JSON object (and writes it to --json).  Needs an MI355X.  Usage:
    python scripts/posterior_bench.py [--rows N] [--haps H] [--loci L] [--models 4,3] [--workdir DIR] [--keep]
                                      [--no-profile] [--no-command] [--json profiles/posterior_bench_40M.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
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

LIMITS = dict(make_sample=600, library=1100, profile=600, command=1100)            # seconds, per child process
STEPS = 3


def say(*a):
    print('[posterior_bench]', *a, file=sys.stderr, flush=True)


def library(args):
    """Child-process body: everything measured through the Python interface on the sample file."""
    import numpy as np
    import torch
    from gbrs_amd import _lib
    from gbrs_amd.alignment import load_alignment
    from gbrs_amd.em import EMfactory, read_length_file
    clock = time.perf_counter
    t0 = clock()
    apm = load_alignment(args.sample, grpfile=args.groups)
    eff = read_length_file(apm, args.lengths, 100)
    L, H, R = apm.shape
    nnz = [len(i) for i in apm.indices]
    out = dict(reads=R, haps=H, loci=L, entries=int(sum(nnz)), value_bytes=int(8 * sum(nnz)), load_s=round(clock() - t0, 2),
               models={})
    say(f'loaded {out["entries"]} entries in {out["load_s"]} s')

    def free_bytes():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    def factory(model, keep):
        em = EMfactory(apm, grouped_models=model != 4, keep_posterior=keep)
        em.set_target_lengths(eff)
        em.prepare()
        return em

    def step_ms(em, model, n=10):
        em.update_allelic_expression(model)                          # warm-up
        lib = _lib.load()
        t = clock()
        _lib.check(lib.gbrs_em_step(em._h, n, None) if model == 4 else lib.gbrs_em_step_model(em._h, model, n, None))
        return (clock() - t) * 1e3 / n

    torch.zeros(1, device='cuda')
    for model in [int(m) for m in args.models.split(',')]:
        row = out['models'][str(model)] = {}
        factory(model, False).close()                                # the first handle of a process pays for more than itself
        before = free_bytes()
        em = factory(model, False)
        row['handle_bytes_without_flag'] = before - free_bytes()
        row['step_ms_without_flag'] = round(step_ms(em, model), 4)
        em.close()
        before = free_bytes()
        em = factory(model, True)
        row['handle_bytes_with_flag'] = before - free_bytes()
        row['step_ms_with_flag'] = round(step_ms(em, model), 4)
        em.prepare()
        for _ in range(STEPS):
            em.update_allelic_expression(model)
        before = free_bytes()
        calls, total = [], 0.0
        for h in range(H):
            t = clock()
            p = em.posterior(h)
            calls.append(round((clock() - t) * 1e3, 2))
            total += float(p.sum())
            del p
        row['posterior_call_ms'] = calls                              # passes + copy out; [0] of model 4: + denominators
        row['posterior_all_haps_ms'] = round(sum(calls), 2)
        row['staging_bytes'] = before - free_bytes()                  # one haplotype's values on the device
        row['extra_device_bytes'] = row['handle_bytes_with_flag'] - row['handle_bytes_without_flag'] + row['staging_bytes']
        # what the flag keeps, from the shapes: theta before the step, D_r, one haplotype's values, and - where the
        # handle would have dropped them (tile layout without the grouped models) - the row ids
        row['extra_device_bytes_by_shape'] = int(8 * L * H + 8 * R + 8 * max(nnz) + (4 * sum(nnz) if model == 4 else 0))
        row['posterior_mass_over_reads'] = total / R                  # every read's posteriors add up to 1
        say(f'model {model}: {row}')
        if model == 4 and not args.no_export:
            fetch = [0.0]

            def timed(h):
                t = clock()
                v = em.posterior(h)
                fetch[0] += clock() - t
                return v
            path = os.path.join(os.path.dirname(args.sample), 'posterior_values.h5')
            t = clock()
            apm.save(path, title='Posterior Probability', incidence_only=False, values=timed)
            whole = clock() - t
            out['export'] = dict(total_s=round(whole, 2), fetch_s=round(fetch[0], 2), h5_write_s=round(whole - fetch[0], 2),
                                 file_bytes=os.path.getsize(path))
            os.remove(path)
            t = clock()
            apm.save(path, title='Posterior Probability')
            out['export']['incidence_only_write_s'] = round(clock() - t, 2)
            out['export']['incidence_only_file_bytes'] = os.path.getsize(path)
            os.remove(path)
            say(f'export: {out["export"]}')
        em.close()
    # a device-to-host copy of the longest haplotype's values alone, to pageable memory as the call does it
    buf = torch.zeros(max(nnz), dtype=torch.float64, device='cuda')
    host = np.empty(max(nnz))
    torch.cuda.synchronize()
    t = clock()
    torch.from_numpy(host).copy_(buf)
    torch.cuda.synchronize()
    out['copy_out_one_hap_ms'] = round((clock() - t) * 1e3, 2)
    out['copy_out_one_hap_bytes'] = int(8 * max(nnz))
    print(json.dumps(out), flush=True)
    return 0


def posterior_kernels(prof_dir):
    """{kernel (template arguments kept): calls, ms} of the kernels this feature adds."""
    out = {}
    for f in glob.glob(os.path.join(prof_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get('Name', '')
                if not any(k in name for k in ('post_den_kernel', 'post_value_kernel', 'keep_theta_kernel')):
                    continue
                key = name.replace('void ', '').replace('gbrs::', '').split('(')[0]
                calls, ns = out.get(key, (0, 0.0))
                out[key] = (calls + int(row['Calls']), ns + float(row['TotalDurationNs']))
    return {k: dict(calls=c, ms=round(ns / 1e6, 3)) for k, (c, ns) in sorted(out.items())}


def run_command(argv, workdir, tag, env):
    """One `gbrs` subcommand as a fresh process under its time limit: (wall seconds, stage dict)."""
    stages = os.path.join(workdir, f'stages_{tag}.json')
    t0 = time.time()
    e = dict(env, GBRS_DATA=workdir, GBRS_STAGE_TIMES=stages, GBRS_T0=repr(t0))
    r = subprocess.run(['timeout', '-k', '10', str(LIMITS['command']), sys.executable, '-m', 'gbrs_amd'] + argv, env=e,
                       cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    wall = time.time() - t0
    if r.returncode != 0 or not os.path.exists(stages):
        raise RuntimeError(f'gbrs {argv[0]} failed (rc {r.returncode}): {r.stderr[-800:]}')
    with open(stages) as fh:
        st = json.load(fh)
    if st.get('error'):
        raise RuntimeError(f'gbrs {argv[0]} logged an error: {st["error"]}')
    return wall, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=40_000_000)
    ap.add_argument('--haps', type=int, default=8)
    ap.add_argument('--loci', type=int, default=120_000)
    ap.add_argument('--models', default='4,3')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--no-command', action='store_true')
    ap.add_argument('--no-export', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--library', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--sample', help=argparse.SUPPRESS)
    ap.add_argument('--groups', help=argparse.SUPPRESS)
    ap.add_argument('--lengths', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.library:
        return library(args)
    workdir = args.workdir or tempfile.mkdtemp(prefix='posterior_bench_')
    os.makedirs(workdir, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = dict(rows=args.rows, haps=args.haps, loci=args.loci, steps_before_posterior=STEPS)
    ok = True
    try:
        t0 = time.time()
        r = subprocess.run(['timeout', '-k', '10', str(LIMITS['make_sample']), sys.executable,
                            os.path.join(ROOT, 'scripts', 'e2e_bench.py'), '--make-sample', '--workdir', workdir, '--rows',
                            str(args.rows), '--haps', str(args.haps), '--loci', str(args.loci), '--format', 'h5',
                            '--cpu-rows', '0'], env=env, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'sample generation failed (rc {r.returncode})')
        sample = json.loads(r.stdout.strip().splitlines()[-1])
        res['sample'] = dict(entries=int(sample['N']), file_bytes=sample['bytes']['h5'], generate_s=round(time.time() - t0, 1))
        say(f'sample: {res["sample"]}')
        child = [sys.executable, os.path.abspath(__file__), '--library', '--sample', sample['files']['h5'], '--groups',
                 sample['group_file'], '--lengths', sample['length_file'], '--models', args.models]
        r = subprocess.run(['timeout', '-k', '10', str(LIMITS['library'])] + child + (['--no-export'] if args.no_export else []),
                           env=env, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'library child failed (rc {r.returncode})')
        res['library'] = json.loads(r.stdout.strip().splitlines()[-1])
        if not args.no_profile and shutil.which('rocprofv3'):
            prof = os.path.join(workdir, 'prof')
            r = subprocess.run(['timeout', '-k', '10', str(LIMITS['profile']), 'rocprofv3', '--kernel-trace', '--stats',
                                '--output-format', 'csv', '-d', prof, '--'] + child + ['--no-export'], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise RuntimeError(f'profile run failed (rc {r.returncode}): {r.stderr[-500:]}')
            res['kernels'] = posterior_kernels(prof)
            shutil.rmtree(prof, ignore_errors=True)
            say(f'kernels: {res["kernels"]}')
        if not args.no_command:
            res['command'] = {}
            for tag, extra in (('report_posterior', ['-w']), ('posterior_values', ['-w', '--posterior-values'])):
                base = os.path.join(workdir, f'out_{tag}')
                wall, st = run_command(['quantify', '-i', sample['files']['h5'], '-g', sample['group_file'], '-L',
                                        sample['length_file'], '-o', base] + extra, workdir, tag, env)
                h5 = f'{base}.multiway.posterior.h5'
                res['command'][tag] = dict(wall_s=round(wall, 2), file_bytes=os.path.getsize(h5), em_iterations=st.get('em_iterations'),
                                           stages_s={k: round(st[k], 3) for k in ('startup', 'load', 'mask', 'em_setup', 'em_run',
                                                                                  'reports', 'main') if k in st})
                os.remove(h5)
                say(f'{tag}: {res["command"][tag]}')
    except RuntimeError as e:                                           # nothing more is started after a failure
        res['failed'] = str(e)
        ok = False
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
