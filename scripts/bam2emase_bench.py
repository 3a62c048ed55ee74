#!/usr/bin/env python3
"""Wall clock of `gbrs bam2emase` on a generated BAM file of stated size.

  1. writes a seeded BAM (worker processes generate and deflate their own slices; BGZF blocks concatenate): reads
     with Illumina-shaped names of 38 bytes that share a 20-byte prefix, `--per-read` adjacent records each (the
     haplotypes of one locus, then the next locus), records of realistic size (100-base sequence and qualities);
  2. runs `python -m gbrs_amd bam2emase` as a fresh process and collects wall time and the stage times (read =
     inflate + parse, rank, build, write: host clock around work that ends in a device synchronise);
  3. one separate run under `rocprofv3 --kernel-trace --stats` for the per-kernel device times;
  4. for orientation only: the pure-Python record loop of tests/bam2emase_restate.py (what the reference's converter
     does per record, without pysam's own cost) on a subsample, scaled linearly to the full record count and
     labelled as scaled.

`--bam2ec` times `gbrs bam2ec` instead, in the same job and on the same generated file: `bam2ec` on the file, `bam2ec`
on the file given twice (the lane merge), the two-step path it replaces (`bam2emase` to an .h5, then `compress`), one
`bam2ec` run under `rocprofv3 --kernel-trace --stats`, and the device memory in use above the idle level while `bam2ec`
runs (sampled every few milliseconds from this process).  Every step is a fresh process under its own time limit; the
first one that fails ends the job.  The files of the one-step and the two-step path are compared member by member.

`--paired` times `gbrs bam2ec --mate-file` on a paired-end sample aligned one end at a time.  Beside the generated file
it writes a second-end file with the same read names in which every read keeps a seeded subset of its records (its first
record always; one of four seeded subsets, so the classes stay a small multiple of the loci), then runs, as fresh
processes in the same job: `bam2ec -i first -I second` (twice, the faster run counts; device memory sampled as above),
the four-command chain it replaces (`bam2emase` on either end, `get-common-alignments`, `compress`), and one paired
run under `rocprofv3 --kernel-trace --stats`.  The two class files are compared member by member; the exit status is 0
only if they are equal and the one command took less wall clock than the chain.

Prints one JSON object.  Needs an MI355X.  Usage:
    python scripts/bam2emase_bench.py [--reads N] [--per-read K] [--haps H] [--loci L] [--format npz|h5]
                                      [--workdir DIR] [--keep] [--no-profile] [--json OUT] [--bam2ec | --paired]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAME_W, SEQ = 38, 100
EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def read_names(ids):
    """38-byte names A00123:45:HXXXXXXXX:<lane>:<tile 4>:<x 5>:<y 5> of the read numbers `ids` (injective)."""
    import numpy as np
    y = ids % 100000
    x = (ids // 100000) % 100000
    tile = 1101 + (ids // 10**10) % 8000
    lane = 1 + (ids // (10**10 * 8000)) % 8
    z = np.char.zfill
    s = np.char.add('A00123:45:HXXXXXXXX:', lane.astype('U1'))
    for part, w in ((tile, 4), (x, 5), (y, 5)):
        s = np.char.add(np.char.add(s, ':'), z(part.astype(f'U{w}'), w))
    return np.char.encode(s, 'ascii').astype(f'S{NAME_W}')


def slice_records(args):
    """Worker: records of reads [r0, r1) -> BGZF bytes in `part`.  Read number k of the file is named after
    (k * 2654435761) mod 2^40, so the file is not in name order.  An eighth item that is true makes the slice one of
    the second end (`--paired`): the same records, of which every read keeps one of four seeded subsets."""
    import numpy as np
    r0, r1, per, haps, loci, seed, part = args[:7]
    mate = len(args) > 7 and args[7]
    rng = np.random.default_rng([seed, r0])
    n = r1 - r0
    ids = (np.arange(r0, r1, dtype=np.int64) * 2654435761) % (1 << 40)
    names = read_names(ids)
    dt = np.dtype([('block_size', '<i4'), ('refid', '<i4'), ('pos', '<i4'), ('l_read_name', 'u1'), ('mapq', 'u1'),
                   ('bin', '<u2'), ('n_cigar', '<u2'), ('flag', '<u2'), ('l_seq', '<i4'), ('next_refid', '<i4'),
                   ('next_pos', '<i4'), ('tlen', '<i4'), ('name', f'S{NAME_W}'), ('nul', 'u1'), ('cigar', '<u4'),
                   ('seq', 'u1', (SEQ // 2,)), ('qual', 'u1', (SEQ,))])
    rec = np.zeros(n * per, dtype=dt)
    locus = rng.integers(0, loci - 1, size=n)
    k = np.tile(np.arange(per), n)
    rec['refid'] = (np.repeat(locus, per) + k // haps) * haps + k % haps
    rec['block_size'] = dt.itemsize - 4
    rec['pos'] = rng.integers(0, 2000, size=n * per)
    rec['l_read_name'] = NAME_W + 1
    rec['mapq'] = 255
    rec['bin'] = 4680
    rec['n_cigar'] = 1
    rec['flag'] = np.where(k == 0, 0, 256)
    rec['l_seq'] = SEQ
    rec['next_refid'] = -1
    rec['next_pos'] = -1
    rec['name'] = np.repeat(names, per)
    rec['cigar'] = SEQ << 4
    seq = rng.integers(0, 4, size=(n, SEQ // 2, 2))                      # the same read sequence in all its records
    rec['seq'] = np.repeat(((1 << seq[:, :, 0]) << 4 | (1 << seq[:, :, 1])).astype(np.uint8), per, axis=0)
    rec['qual'] = np.repeat(rng.choice(np.array([2, 14, 27, 37, 37, 37], dtype=np.uint8), size=(n, SEQ)), per, axis=0)
    if mate:
        masks = np.random.default_rng([seed, 2]).random((4, per)) < 0.7
        masks[:, 0] = True                                               # a read keeps its first record in every subset
        rec = rec[masks[np.random.default_rng([seed, r0, 2]).integers(0, 4, size=n)].reshape(-1)]
    plain = rec.tobytes()
    with open(part, 'wb') as fh:
        for at in range(0, len(plain), 0xFF00):
            chunk = plain[at:at + 0xFF00]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            cdata = co.compress(chunk) + co.flush()
            fh.write(struct.pack('<BBBBIBBHBBHH', 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, 25 + len(cdata)) + cdata +
                     struct.pack('<II', zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return len(plain)


def write_bam(path, reads, per, haps, loci, seed, procs, mate=False):
    lname = [f'T{l:07d}' for l in range(loci)]
    hname = [chr(65 + h) for h in range(haps)]
    text = b'@HD\tVN:1.6\tSO:unsorted\n'
    head = [b'BAM\x01', struct.pack('<i', len(text)), text, struct.pack('<i', loci * haps)]
    for l in lname:
        for h in hname:
            n = f'{l}_{h}'.encode()
            head += [struct.pack('<i', len(n) + 1), n, b'\x00', struct.pack('<i', 3000)]
    head = b''.join(head)
    step = max(1, min(250_000, (reads + procs - 1) // procs))
    jobs = [(r0, min(reads, r0 + step), per, haps, loci, seed, f'{path}.part{k}') + ((True,) if mate else ())
            for k, r0 in enumerate(range(0, reads, step))]
    plain = len(head)
    with open(path, 'wb') as out:
        for at in range(0, len(head), 0xFF00):
            chunk = head[at:at + 0xFF00]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            cdata = co.compress(chunk) + co.flush()
            out.write(struct.pack('<BBBBIBBHBBHH', 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, 25 + len(cdata)) + cdata +
                      struct.pack('<II', zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
        with ProcessPoolExecutor(max_workers=procs) as pool:
            for job, n in zip(jobs, pool.map(slice_records, jobs)):
                plain += n
                with open(job[6], 'rb') as fh:
                    shutil.copyfileobj(fh, out, 1 << 24)
                os.remove(job[6])
        out.write(EOF_BLOCK)
    ids = os.path.join(os.path.dirname(path), 'locus_ids.tsv')
    with open(ids, 'w') as fh:
        fh.write('\n'.join(lname) + '\n')
    return ids, hname, plain


def kernel_stats(prof_dir):
    out = {}
    for f in glob.glob(os.path.join(prof_dir, '**', '*kernel_stats.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get('Name', '').replace('(anonymous namespace)::', '')
                if name.startswith('void '):
                    name = name[5:]
                key = name.split('(')[0].split('<')[0][:70]           # template and call arguments dropped
                calls, ns = out.get(key, (0, 0.0))
                out[key] = (calls + int(row['Calls']), ns + float(row['TotalDurationNs']))
    return {k: dict(calls=c, ms=round(ns / 1e6, 3)) for k, (c, ns) in sorted(out.items(), key=lambda kv: -kv[1][1])}


class DeviceMemoryWatch:
    """Device memory in use on device 0, polled from a thread of this process while a child runs (hipMemGetInfo counts
    every process's allocations).  peak_above_idle_bytes is the largest reading minus the reading before the child
    started, so it includes the child's runtime context; None when the runtime could not be asked."""

    def __init__(self, interval=0.004):
        import ctypes
        import threading
        self.interval, self.peak, self.idle, self.samples = interval, None, None, 0
        self._stop = threading.Event()
        self._thread = None
        try:
            self._hip = ctypes.CDLL('libamdhip64.so')
            self._free, self._total = ctypes.c_size_t(0), ctypes.c_size_t(0)
            if self._hip.hipSetDevice(0) != 0 or self._used() is None:
                self._hip = None
        except OSError:
            self._hip = None

    def _used(self):
        import ctypes
        if self._hip.hipMemGetInfo(ctypes.byref(self._free), ctypes.byref(self._total)) != 0:
            return None
        return self._total.value - self._free.value

    def _poll(self):
        self._hip.hipSetDevice(0)
        while not self._stop.is_set():
            u = self._used()
            if u is not None:
                self.peak = u if self.peak is None else max(self.peak, u)
                self.samples += 1
            time.sleep(self.interval)

    def __enter__(self):
        import threading
        if self._hip is not None:
            self.idle = self._used()
            self._thread = threading.Thread(target=self._poll, daemon=True)
            self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._thread is not None:
            self._thread.join()

    @property
    def peak_above_idle_bytes(self):
        return None if self.peak is None or self.idle is None else max(0, self.peak - self.idle)


def run_staged(cmd, stage_file, limit_s, watch_memory=False):
    """One fresh process under a time limit -> dict(wall_s, stages..., [peak_device_bytes_above_idle]) or dict(failed=...)."""
    env = dict(os.environ, PYTHONPATH=ROOT, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()))
    if os.path.exists(stage_file):
        os.remove(stage_file)
    watch = DeviceMemoryWatch() if watch_memory else None
    t0 = time.time()
    try:
        if watch is not None:
            with watch:
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit_s)
        else:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        return dict(failed=f'time limit of {limit_s} s')
    wall = time.time() - t0
    st = {}
    if os.path.exists(stage_file):
        with open(stage_file) as fh:
            st = json.load(fh)
    if r.returncode != 0 or 'error' in st or not st:
        return dict(failed=st.get('error', f'exit status {r.returncode}: {r.stderr[-500:]}'))
    out = dict(wall_s=round(wall, 3), **{k: round(v, 4) for k, v in st.items()})
    if watch is not None:
        out['peak_device_bytes_above_idle'] = watch.peak_above_idle_bytes
        out['memory_samples'] = watch.samples
    return out


def files_equal(a, b):
    """The class files of the one-step and the two-step path, member by member."""
    import numpy as np
    from gbrs_amd.alignment import load_alignment, read_rname
    x, y = load_alignment(a), load_alignment(b)
    same = x.shape == y.shape and x.hname == y.hname and x.lname == y.lname and read_rname(a) is None
    same = same and x.count is not None and y.count is not None and np.array_equal(x.count, y.count)
    for h in range(x.shape[1]):
        same = same and np.array_equal(x.indptr[h], y.indptr[h]) and np.array_equal(x.indices[h], y.indices[h])
    return bool(same), int(x.shape[2]), float(x.count.sum())


def bench_bam2ec(args, res, workdir, bam, ids, hname):
    py = [sys.executable, '-m', 'gbrs_amd']
    common = ['-m', ids, '-h', ','.join(hname)]
    stage_file = os.path.join(workdir, 'stages.json')
    one, twice = os.path.join(workdir, 'one.compressed.h5'), os.path.join(workdir, 'twice.compressed.h5')
    mid, two = os.path.join(workdir, 'sample.h5'), os.path.join(workdir, 'two.compressed.h5')
    limit = max(120, int(args.reads / 100_000))                       # 400 s at 40M reads: ten times what a step takes
    steps = [('bam2ec', py + ['bam2ec', '-i', bam] + common + ['-o', one], True, 2),
             ('bam2ec_file_twice', py + ['bam2ec', '-i', bam, '-i', bam] + common + ['-o', twice], True, 1),
             ('bam2emase', py + ['bam2emase', '-i', bam] + common + ['-o', mid], False, 1),
             ('compress', py + ['compress', '-i', mid, '-o', two], False, 1)]
    for name, cmd, watch, times in steps:
        runs = []
        for _ in range(times):
            print(f'[bench] {name} ...', file=sys.stderr, flush=True)
            r = run_staged(cmd, stage_file, limit, watch_memory=watch)
            if 'failed' in r:
                res[name] = r
                return 1
            runs.append(r)
        res[name] = dict(min(runs, key=lambda x: x['wall_s']), runs=len(runs))
    res['two_step_wall_s'] = round(res['bam2emase']['wall_s'] + res['compress']['wall_s'], 3)
    res['output_bytes'] = dict(bam2ec=os.path.getsize(one), bam2ec_file_twice=os.path.getsize(twice),
                               bam2emase=os.path.getsize(mid), compress=os.path.getsize(two))
    same, n_ecs, n_reads = files_equal(one, two)
    res['bam2ec_equals_two_step'], res['num_ecs'], res['count_sum'] = same, n_ecs, n_reads
    if not args.no_profile and shutil.which('rocprofv3'):
        env = dict(os.environ, PYTHONPATH=ROOT, GBRS_ORDERLY_EXIT='1')           # the tracer writes at exit
        for key, step in (('profile', steps[0]), ('profile_file_twice', steps[1])):
            print(f'[bench] {step[0]} under rocprofv3 ...', file=sys.stderr, flush=True)
            prof = os.path.join(workdir, key)
            try:
                r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '--'] + step[1],
                                   env=env, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                   timeout=2 * limit)
            except subprocess.TimeoutExpired:
                res[key] = dict(rc='time limit')
                return 1
            k = kernel_stats(prof)
            res[key] = dict(rc=r.returncode, kernels=k, device_ms_total=round(sum(v['ms'] for v in k.values()), 3),
                            stage_device_ms=stage_device_ms(prof),
                            gather_rname_kernel_calls=sum(v['calls'] for n, v in k.items() if 'gather_rname' in n))
            if r.returncode != 0:
                return 1
    return 0 if same else 1


def bench_paired(args, res, workdir, bam, mate, ids, hname):
    py = [sys.executable, '-m', 'gbrs_amd']
    common = ['-m', ids, '-h', ','.join(hname)]
    stage_file = os.path.join(workdir, 'stages.json')
    one, four = os.path.join(workdir, 'one.compressed.h5'), os.path.join(workdir, 'four.compressed.h5')
    end1, end2, both = (os.path.join(workdir, f'{k}.h5') for k in ('end1', 'end2', 'common'))
    limit = max(120, int(args.reads / 100_000))
    chain = ('bam2emase_first', 'bam2emase_second', 'get_common_alignments', 'compress')
    steps = [('bam2ec_paired', py + ['bam2ec', '-i', bam, '--mate-file', mate] + common + ['-o', one], True, 2),
             (chain[0], py + ['bam2emase', '-i', bam] + common + ['-o', end1], False, 1),
             (chain[1], py + ['bam2emase', '-i', mate] + common + ['-o', end2], False, 1),
             (chain[2], py + ['get-common-alignments', '-i', end1, '-i', end2, '-o', both], False, 1),
             (chain[3], py + ['compress', '-i', both, '-o', four], False, 1)]
    for name, cmd, watch, times in steps:
        runs = []
        for _ in range(times):
            print(f'[bench] {name} ...', file=sys.stderr, flush=True)
            r = run_staged(cmd, stage_file, limit, watch_memory=watch)
            if 'failed' in r:
                res[name] = r
                return 1
            runs.append(r)
        res[name] = dict(min(runs, key=lambda x: x['wall_s']), runs=len(runs))
    res['chain_wall_s'] = round(sum(res[k]['wall_s'] for k in chain), 3)
    res['output_bytes'] = dict(bam2ec_paired=os.path.getsize(one), bam2emase_first=os.path.getsize(end1),
                               bam2emase_second=os.path.getsize(end2), get_common_alignments=os.path.getsize(both),
                               compress=os.path.getsize(four))
    same, n_ecs, n_reads = files_equal(one, four)
    res['paired_equals_chain'], res['num_ecs'], res['count_sum'] = same, n_ecs, n_reads
    res['paired_below_chain'] = res['bam2ec_paired']['wall_s'] < res['chain_wall_s']
    if not args.no_profile and shutil.which('rocprofv3'):
        env = dict(os.environ, PYTHONPATH=ROOT, GBRS_ORDERLY_EXIT='1')           # the tracer writes at exit
        print('[bench] bam2ec_paired under rocprofv3 ...', file=sys.stderr, flush=True)
        prof = os.path.join(workdir, 'profile')
        try:
            r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '--'] + steps[0][1],
                               env=env, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=2 * limit)
        except subprocess.TimeoutExpired:
            res['profile'] = dict(rc='time limit')
            return 1
        k = kernel_stats(prof)
        res['profile'] = dict(rc=r.returncode, kernels=k, device_ms_total=round(sum(v['ms'] for v in k.values()), 3))
        if r.returncode != 0:
            return 1
    return 0 if same and res['paired_below_chain'] else 1


def stage_device_ms(prof_dir):
    """Device time of the rank and the classes stage of `bam2ec` from the kernel trace, in dispatch order: a file's rank
    stage starts with pack_names_kernel, its classes stage with record_keys_kernel.  None without a trace."""
    rows = []
    for f in glob.glob(os.path.join(prof_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                try:
                    rows.append((int(row['Start_Timestamp']), int(row['End_Timestamp']), row['Kernel_Name']))
                except (KeyError, ValueError):
                    return None
    if not rows:
        return None
    rows.sort()
    out, stage = dict(before=0.0, rank=0.0, classes=0.0), 'before'
    for t0, t1, name in rows:
        if 'pack_names_kernel' in name:
            stage = 'rank'
        elif 'record_keys_kernel' in name:
            stage = 'classes'
        out[stage] += (t1 - t0) / 1e6
    return {k: round(v, 3) for k, v in out.items()}


def python_loop_seconds(reads, per, haps, loci):
    """The restatement's per-record loop (set of names, sorted, dict look-ups, split, two appends) on `reads` reads."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from bam2emase_restate import restate
    ids = (np.arange(reads, dtype=np.int64) * 2654435761) % (1 << 40)
    names = [n.decode() for n in np.repeat(read_names(ids), per)]
    lname = [f'T{l:07d}' for l in range(loci)]
    hname = [chr(65 + h) for h in range(haps)]
    refs = [f'{l}_{h}' for l in lname for h in hname]
    rng = np.random.default_rng(1)
    k = np.tile(np.arange(per), reads)
    refids = ((np.repeat(rng.integers(0, loci - 1, size=reads), per) + k // haps) * haps + k % haps).tolist()
    flags = np.where(k == 0, 0, 256).tolist()
    t0 = time.time()
    restate(refs, names, refids, flags, hname, lname)
    return time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=4_000_000)
    ap.add_argument('--per-read', type=int, default=9)
    ap.add_argument('--haps', type=int, default=8)
    ap.add_argument('--loci', type=int, default=120_000)
    ap.add_argument('--format', default='npz', choices=('npz', 'h5'))
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--python-reads', type=int, default=100_000, help='reads of the pure-Python loop (0 = skip)')
    ap.add_argument('--procs', type=int, default=int(os.environ.get('OMP_NUM_THREADS', '16')))
    ap.add_argument('--json', default=None)
    ap.add_argument('--bam2ec', action='store_true', help='time `gbrs bam2ec` against `bam2emase` + `compress` (see above)')
    ap.add_argument('--paired', action='store_true',
                    help='time `gbrs bam2ec --mate-file` against the four-command chain it replaces (see above)')
    args = ap.parse_args()
    if args.bam2ec and args.paired:
        ap.error('--bam2ec and --paired are two jobs')
    workdir = args.workdir or tempfile.mkdtemp(prefix='bam2emase_bench_')
    os.makedirs(workdir, exist_ok=True)
    bam = os.path.join(workdir, 'sample.bam')
    t0 = time.time()
    ids, hname, plain = write_bam(bam, args.reads, args.per_read, args.haps, args.loci, 20, args.procs)
    res = dict(reads=args.reads, records=args.reads * args.per_read, haps=args.haps, loci=args.loci,
               name_bytes=NAME_W, bam_bytes=os.path.getsize(bam), inflated_bytes=plain,
               generate_s=round(time.time() - t0, 2), format=args.format,
               configs1_records=360_000_000, below_configs1=args.reads * args.per_read < 360_000_000)
    if args.paired:
        t0 = time.time()
        mate = os.path.join(workdir, 'sample_2.bam')
        _, _, plain2 = write_bam(mate, args.reads, args.per_read, args.haps, args.loci, 20, args.procs, mate=True)
        res.update(mate_bam_bytes=os.path.getsize(mate), mate_inflated_bytes=plain2, mate_records=(plain2 - plain) // 229
                   + args.reads * args.per_read, mate_generate_s=round(time.time() - t0, 2))
    if args.bam2ec or args.paired:
        res['format'] = 'h5'
        rc = (bench_paired(args, res, workdir, bam, mate, ids, hname) if args.paired else
              bench_bam2ec(args, res, workdir, bam, ids, hname))
        if not args.keep and args.workdir is None:
            shutil.rmtree(workdir, ignore_errors=True)
        text = json.dumps(res)
        if args.json:
            with open(args.json, 'w') as fh:
                fh.write(text + '\n')
        print(text, flush=True)
        return rc
    out = os.path.join(workdir, f'sample.{args.format}')
    stage_file = os.path.join(workdir, 'stages.json')
    cmd = [sys.executable, '-m', 'gbrs_amd', 'bam2emase', '-i', bam, '-m', ids, '-h', ','.join(hname), '-o', out]
    runs = []
    for _ in range(2):                                        # the second run reads the file from the page cache
        env = dict(os.environ, PYTHONPATH=ROOT, GBRS_STAGE_TIMES=stage_file, GBRS_T0=repr(time.time()))
        t0 = time.time()
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        wall = time.time() - t0
        with open(stage_file) as fh:
            st = json.load(fh)
        if r.returncode != 0 or 'error' in st or not os.path.exists(out):
            print(json.dumps(dict(res, failed=st.get('error', r.stderr[-500:]))), flush=True)
            return 1
        runs.append(dict(wall_s=round(wall, 3), **{k: round(v, 4) for k, v in st.items()}))
    res['runs'] = runs
    best = min(runs, key=lambda x: x['wall_s'])
    res['wall_s'] = best['wall_s']
    res['stages_s'] = {k: best[k] for k in ('read', 'rank', 'build', 'write')}
    res['read_input_MB_per_s'] = round(res['bam_bytes'] / 1e6 / best['read'], 1)
    res['read_inflated_MB_per_s'] = round(plain / 1e6 / best['read'], 1)
    res['output_bytes'] = os.path.getsize(out)
    if not args.no_profile and shutil.which('rocprofv3'):
        prof = os.path.join(workdir, 'prof')
        env = dict(os.environ, PYTHONPATH=ROOT, GBRS_ORDERLY_EXIT='1')           # the tracer writes at exit
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', prof, '--'] + cmd,
                           env=env, cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        res['profile_rc'] = r.returncode
        res['kernels'] = kernel_stats(prof)
        res['device_ms_total'] = round(sum(v['ms'] for v in res['kernels'].values()), 3)
    if args.python_reads:
        n = min(args.python_reads, args.reads)
        s = python_loop_seconds(n, args.per_read, args.haps, args.loci)
        res['python_record_loop'] = dict(reads=n, seconds=round(s, 3),
                                         scaled_to_full_s=round(s * args.reads / n, 1),
                                         note='SCALED linearly from the subsample; the restatement\'s loop only, '
                                              'without pysam decoding, temporary files or PyTables')
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
