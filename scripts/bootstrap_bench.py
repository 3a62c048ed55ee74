#!/usr/bin/env python3
"""What `gbrs quantify --bootstrap B` costs at BASELINE configs[1] size (40M reads x 8 haplotypes x 120k isoforms) and on
the multi-isoform variant of the same sample.

Per variant:
  1. a child process writes the bench generator's sample as an EMASE `.h5` with its group and length files;
  2. a child process (`--library`) loads the file and measures through the Python interface: an ordinary handle's device
     bytes and unweighted step time; a resampling handle's device bytes, the bytes the flag added (gbrs_em_resample_info),
     the time of one `resample` call, the weighted step time on that handle after a draw, B replicates through
     em.bootstrap() (seconds and iterations per replicate), and the ratio of one resample call to one EM step on the
     same handle;
  3. the same child once more under `rocprofv3 --kernel-trace --stats` for the device time of the new kernels;
  4. the command as a fresh process, without the option and with `--bootstrap B`: wall and its stages.
Every step that uses the GPU is a child process under a `timeout` of its own, and the first failure ends the run.

Prints one JSON object (and writes it to --json).  Needs an MI355X.  Usage:
    python scripts/bootstrap_bench.py [--rows N] [--haps H] [--loci L] [--replicates B] [--variants survey,multi_isoform]
                                      [--workdir DIR] [--keep] [--no-profile] [--no-command]
                                      [--json profiles/bootstrap_bench_40M.json]
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

LIMITS = dict(make_sample=600, library=900, profile=600, command=900)            # seconds, per child process
NEW_KERNELS = ('resample_draw_kernel', 'resample_big_kernel', 'install_weights_kernel', 'stats_sum_kernel',
               'stats_current_kernel', 'stats_group_kernel', 'stats_fold_kernel')


def say(*a):
    print('[bootstrap_bench]', *a, file=sys.stderr, flush=True)


def make_sample(args):
    """Child-process body: the sample of one variant as `.h5` + support files."""
    import numpy as np
    import torch
    from e2e_bench import write_support_files
    from gbrs_amd import synth, synth_torch
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    t0 = time.perf_counter()
    prob = synth_torch.make_em_problem_device(args.rows, args.haps, args.loci, synth.SEED_BASE_EM + 1, 'cuda:0',
                                              variant=args.variant)
    ip = [t.cpu().numpy().view(np.uint32) for t in prob['indptr']]
    ix = [t.cpu().numpy().view(np.uint32) for t in prob['indices']]
    eff = prob['eff_len'].cpu().numpy()
    gene_starts, N = prob['gene_starts'], prob['N']
    del prob
    torch.cuda.empty_cache()
    lname, hname, gname, grp, lens = write_support_files(args.workdir, args.loci, args.haps, gene_starts, eff[0])
    apm = AlignmentPropertyMatrix(shape=(args.loci, args.haps, args.rows), indptr=ip, indices=ix, haplotype_names=hname,
                                  locus_names=lname)
    path = os.path.join(args.workdir, 'sample.h5')
    apm.save(path)
    print(json.dumps(dict(file=path, group_file=grp, length_file=lens, N=int(N), bytes=os.path.getsize(path),
                          build_s=round(time.perf_counter() - t0, 1))), flush=True)
    return 0


def library(args):
    """Child-process body: everything measured through the Python interface on the sample file."""
    import ctypes as C
    import torch
    from gbrs_amd import _lib
    from gbrs_amd.alignment import load_alignment
    from gbrs_amd.em import EMfactory, read_length_file
    clock = time.perf_counter
    t0 = clock()
    apm = load_alignment(args.sample, grpfile=args.groups)
    eff = read_length_file(apm, args.lengths, 100)
    L, H, R = apm.shape
    out = dict(reads=R, haps=H, loci=L, entries=int(sum(len(i) for i in apm.indices)), load_s=round(clock() - t0, 2))
    lib = _lib.load()

    def free_bytes():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[0])

    def factory(resample):
        em = EMfactory(apm, resample=resample)
        em.set_target_lengths(eff)
        em.prepare()
        return em

    def step_ms(em, n=20):
        em.update_allelic_expression(4)                              # warm-up
        _lib.check(lib.gbrs_em_sync(em._h))
        t = clock()
        _lib.check(lib.gbrs_em_step(em._h, n, None))
        _lib.check(lib.gbrs_em_sync(em._h))
        return (clock() - t) * 1e3 / n

    torch.zeros(1, device='cuda')
    factory(False).close()                                           # the first handle of a process pays for more than itself
    before = free_bytes()
    em = factory(False)
    out['handle_bytes_ordinary'] = before - free_bytes()
    out['step_ms_ordinary_unweighted'] = round(step_ms(em), 4)
    inf = em.info()
    out['ordinary_words'] = int(inf.num_device_words)
    em.close()
    before = free_bytes()
    t = clock()
    em = factory(True)
    out['resampling_handle_setup_s'] = round(clock() - t, 3)
    out['handle_bytes_resampling'] = before - free_bytes()
    extra, big, cut = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    _lib.check(lib.gbrs_em_resample_info(em._h, C.byref(extra), C.byref(big), C.byref(cut)))
    out['extra_device_bytes_from_the_flag'] = int(extra.value)
    out['resampling_words'] = int(em.info().num_device_words)
    out['big_rows'], out['cut'] = int(big.value), int(cut.value)
    out['step_ms_resampling_base_weights'] = round(step_ms(em), 4)
    em.resample(1, 0)                                                # warm-up (code object, first launch)
    calls = []
    for b in range(1, 6):
        t = clock()
        em.resample(1, b)
        calls.append(round((clock() - t) * 1e3, 4))
    out['resample_call_ms'] = calls
    out['resample_ms'] = round(sorted(calls)[len(calls) // 2], 4)
    out['zero_weight_fraction'] = round(float((em.weights() == 0).mean()), 4)
    em.reprepare(0.0)
    out['step_ms_resampling_weighted'] = round(step_ms(em), 4)
    out['resample_over_step'] = round(out['resample_ms'] / out['step_ms_resampling_weighted'], 3)
    t = clock()
    res = em.bootstrap(4, args.replicates, seed=7, tol=1e-4, max_iters=999)
    wall = clock() - t
    out['replicates'] = args.replicates
    out['seconds_per_replicate'] = round(wall / args.replicates, 5)
    out['iterations_per_replicate'] = round(float(res['num_iters'].mean()), 2)
    out['iterations_min_max'] = [int(res['num_iters'].min()), int(res['num_iters'].max())]
    out['median_relative_sd_of_expressed_gene_tpm'] = None
    if 'genes' in res:
        import numpy as np
        m, s = res['genes']['tpm_total_mean'], res['genes']['tpm_total_sd']
        out['median_relative_sd_of_expressed_gene_tpm'] = round(float(np.median(s[m > 1.0] / m[m > 1.0])), 5)
    em.close()
    print(json.dumps(out), flush=True)
    return 0


def new_kernels(prof_dir):
    """{kernel: calls, ms} of the kernels this feature adds."""
    out = {}
    for f in glob.glob(os.path.join(prof_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get('Name', '')
                if not any(k in name for k in NEW_KERNELS):
                    continue
                key = name.replace('void ', '').replace('gbrs::', '').split('(')[0]
                calls, ns = out.get(key, (0, 0.0))
                out[key] = (calls + int(row['Calls']), ns + float(row['TotalDurationNs']))
    return {k: dict(calls=c, ms=round(ns / 1e6, 3), us_per_call=round(ns / 1e3 / max(c, 1), 2)) for k, (c, ns) in sorted(out.items())}


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


def one_variant(args, variant, workdir, env):
    res = {}
    me = os.path.abspath(__file__)
    t0 = time.time()
    r = subprocess.run(['timeout', '-k', '10', str(LIMITS['make_sample']), sys.executable, me, '--make-sample', '--workdir',
                        workdir, '--rows', str(args.rows), '--haps', str(args.haps), '--loci', str(args.loci), '--variant',
                        variant], env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'sample generation failed (rc {r.returncode})')
    sample = json.loads(r.stdout.strip().splitlines()[-1])
    res['sample'] = dict(entries=sample['N'], file_bytes=sample['bytes'], generate_s=round(time.time() - t0, 1))
    say(f'{variant} sample: {res["sample"]}')
    child = [sys.executable, me, '--library', '--sample', sample['file'], '--groups', sample['group_file'], '--lengths',
             sample['length_file'], '--replicates', str(args.replicates)]
    r = subprocess.run(['timeout', '-k', '10', str(LIMITS['library'])] + child, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'library child failed (rc {r.returncode})')
    res['library'] = json.loads(r.stdout.strip().splitlines()[-1])
    say(f'{variant} library: {res["library"]}')
    if not args.no_profile and shutil.which('rocprofv3'):
        prof = os.path.join(workdir, 'prof')
        r = subprocess.run(['timeout', '-k', '10', str(LIMITS['profile']), 'rocprofv3', '--kernel-trace', '--stats',
                            '--output-format', 'csv', '-d', prof, '--'] + child, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'profile run failed (rc {r.returncode}): {r.stderr[-500:]}')
        res['kernels'] = new_kernels(prof)
        shutil.rmtree(prof, ignore_errors=True)
        say(f'{variant} kernels: {res["kernels"]}')
    if not args.no_command:
        res['command'] = {}
        for tag, extra in (('plain', []), ('bootstrap', ['--bootstrap', str(args.replicates)])):
            base = os.path.join(workdir, f'out_{variant}_{tag}')
            wall, st = run_command(['quantify', '-i', sample['file'], '-g', sample['group_file'], '-L', sample['length_file'],
                                    '-o', base] + extra, workdir, tag, env)
            res['command'][tag] = dict(wall_s=round(wall, 2), em_iterations=st.get('em_iterations'),
                                       stages_s={k: round(st[k], 3) for k in ('startup', 'load', 'mask', 'em_setup', 'em_run',
                                                                              'reports', 'bootstrap', 'main') if k in st})
            say(f'{variant} {tag}: {res["command"][tag]}')
    os.remove(sample['file'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=40_000_000)
    ap.add_argument('--haps', type=int, default=8)
    ap.add_argument('--loci', type=int, default=120_000)
    ap.add_argument('--replicates', type=int, default=20)
    ap.add_argument('--variants', default='survey,multi_isoform')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--no-command', action='store_true')
    ap.add_argument('--json', default=None)
    ap.add_argument('--library', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--make-sample', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--variant', default='survey', help=argparse.SUPPRESS)
    ap.add_argument('--sample', help=argparse.SUPPRESS)
    ap.add_argument('--groups', help=argparse.SUPPRESS)
    ap.add_argument('--lengths', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.make_sample:
        return make_sample(args)
    if args.library:
        return library(args)
    workdir = args.workdir or tempfile.mkdtemp(prefix='bootstrap_bench_')
    os.makedirs(workdir, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = dict(rows=args.rows, haps=args.haps, loci=args.loci, replicates=args.replicates, variants={})
    ok = True
    try:
        for variant in [v for v in args.variants.split(',') if v]:
            res['variants'][variant] = {}
            res['variants'][variant] = one_variant(args, variant, workdir, env)
            if args.json:                                            # what is measured so far survives a later failure
                with open(args.json, 'w') as fh:
                    fh.write(json.dumps(res) + '\n')
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
