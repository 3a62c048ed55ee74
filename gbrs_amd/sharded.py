"""`gbrs quantify --gpus N`: one sample's reads sharded over N ranks, one process per GPU.

The parent (launch) starts N fresh `python -m gbrs_amd.sharded` children and never imports torch or opens a
device itself.  Every rank loads the whole file, cuts out its row block on the device (gbrs_shard_plan / _index /
_gather, gbrs_amd/csrc/em_shard.inc: the same blocks as gbrs_amd.dist.shard_rows), builds its engine(s) from the
block and runs the EM with one all-reduce of the partial vector per iteration (gbrs_amd.dist).  Two engines per
rank (PipelinedShardedEM: the all-reduce of one locus range behind the E-step of the other) when the loci can be
cut at a gene boundary that no row of any block straddles and the pseudocount is 0; one engine (ShardedEM)
otherwise.  Rank 0 writes the reports of the single-GPU command once every rank has reported success.
"""
from __future__ import annotations

import json
import logging
import os
import sys
import time
from dataclasses import dataclass, field

import numpy as np

logger = logging.getLogger('gbrs')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_TIMEOUT_S = 300         # process group timeout: a lost rank ends the run instead of hanging it


# ---- parent ------------------------------------------------------------------------------------------------------

def device_list(args):
    """The N device ordinals of `--gpus N` (`--devices`, else --device + k)."""
    if args.devices is None:
        return [args.device + k for k in range(args.gpus)]
    return [int(x) for x in str(args.devices).split(',') if x.strip() != '']


def check_args(args):
    """The combinations the sharded path refuses before any child starts (RuntimeError, logged by the CLI)."""
    if args.gpus < 1:
        raise RuntimeError(f'--gpus must be at least 1, got {args.gpus}')
    if args.multiread_model != 4:
        raise RuntimeError(f'--gpus: multiread model {args.multiread_model} is not available on the sharded path '
                           '(models 1-3 run on one GPU)')
    if getattr(args, 'posterior_values', False):
        raise RuntimeError('--gpus: --posterior-values is not available on the sharded path')
    if args.report_posterior:
        raise RuntimeError('--gpus: -w/--report-posterior is not available on the sharded path')
    if args.merge_identical_rows:
        raise RuntimeError('--gpus: --merge-identical-rows is not available on the sharded path')
    if getattr(args, 'bootstrap', None) is not None:
        raise RuntimeError('--gpus: --bootstrap is not available on the sharded path (the replicates run on one GPU)')
    try:
        devices = device_list(args)
    except ValueError:
        raise RuntimeError(f'--devices must be comma-separated device ordinals, got {args.devices!r}') from None
    if len(devices) != args.gpus:
        raise RuntimeError(f'--devices names {len(devices)} devices for --gpus {args.gpus}')
    if args.dist_backend == 'nccl' and len(set(devices)) != len(devices):
        raise RuntimeError('--devices repeats a device: RCCL takes one rank per GPU (--dist-backend gloo allows it)')
    return devices


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def launch_plan(args, argv, port, environ=None):
    """[(command, environment)] of the N ranks."""
    environ = dict(os.environ if environ is None else environ)
    devices = check_args(args)
    world = args.gpus
    threads = None
    if not environ.get('GBRS_IO_THREADS'):
        # every rank decodes the whole file; without a user setting each would take min(32, affinity) threads
        threads = max(1, min(32, len(os.sched_getaffinity(0))) // world)
    pypath = environ.get('PYTHONPATH')
    plan = []
    for k in range(world):
        env = dict(environ, RANK=str(k), WORLD_SIZE=str(world), LOCAL_RANK=str(k), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), GBRS_SHARD_DEVICE=str(devices[k]), GBRS_SHARD_BACKEND=args.dist_backend,
                   PYTHONPATH=ROOT if not pypath else ROOT + os.pathsep + pypath)
        if threads is not None:
            env['GBRS_IO_THREADS'] = str(threads)
        env.pop('GBRS_STAGE_TIMES', None)
        plan.append(([sys.executable, '-m', 'gbrs_amd.sharded'] + list(argv), env))
    return plan


def _relay(k, stream, tail):
    for line in stream:
        tail.append(line.rstrip('\n'))
        del tail[:-20]
        sys.stderr.write(line if k == 0 else f'[rank {k}] {line}')
        sys.stderr.flush()


def launch(args, argv, stages):
    """Run the N ranks and wait for them.  A rank that exits non-zero takes the others down (they would wait in a
    collective); the failure is raised here for the CLI to log."""
    import subprocess
    import tempfile
    import threading
    plan = launch_plan(args, argv, free_port())
    want_times = bool(os.getenv('GBRS_STAGE_TIMES'))
    tmp = tempfile.TemporaryDirectory(prefix='gbrs-shard-') if want_times else None
    procs, tails, relays = [], [], []
    try:
        for k, (cmd, env) in enumerate(plan):
            if tmp is not None:
                env['GBRS_STAGE_TIMES'] = os.path.join(tmp.name, f'rank{k}.json')
            p = subprocess.Popen(cmd, env=env, stdin=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            tail = []
            t = threading.Thread(target=_relay, args=(k, p.stderr, tail), daemon=True)
            t.start()
            procs.append(p)
            tails.append(tail)
            relays.append(t)
        failed = None
        while failed is None and any(p.poll() is None for p in procs):
            for k, p in enumerate(procs):
                if p.poll() not in (None, 0):
                    failed = k
                    break
            else:
                time.sleep(0.05)
        if failed is None:
            failed = next((k for k, p in enumerate(procs) if p.returncode != 0), None)
        if failed is not None:
            _stop(procs)
        for t in relays:
            t.join(timeout=5)
        if tmp is not None:
            ranks = []
            for k in range(len(plan)):
                try:
                    with open(os.path.join(tmp.name, f'rank{k}.json')) as fh:
                        ranks.append(json.load(fh))
                except (OSError, ValueError):
                    ranks.append({})
            stages.update(world=args.gpus, backend=args.dist_backend, ranks=ranks,
                          path=ranks[0].get('path'), em_iterations=ranks[0].get('em_iterations'))
        if failed is not None:
            why = next((ln for ln in reversed(tails[failed]) if ln.strip()), 'no message')
            raise RuntimeError(f'rank {failed} of {args.gpus} failed (exit status {procs[failed].returncode}): {why}')
    finally:
        _stop(procs)
        if tmp is not None:
            tmp.cleanup()


def _stop(procs):
    for p in procs:
        if p.poll() is None:
            p.terminate()
    for p in procs:
        try:
            p.wait(timeout=10)
        except Exception:     # noqa: BLE001 - SIGTERM ignored: kill
            p.kill()
            p.wait()


# ---- device sharding (libgbrs_hip) -------------------------------------------------------------------------------

def _ptrs(tensors):
    from . import _lib
    return _lib.raw_table([t.data_ptr() if t is not None and t.numel() else None for t in tensors])


def shard_plan(R, L, H, indptr, indices, world, device):
    """Row bounds [world + 1] of device CSC tensors (int32 views of the uint32 arrays): dist.shard_rows' blocks."""
    import ctypes as C
    from . import _lib
    bounds = np.zeros(world + 1, dtype=np.uint64)
    _lib.check(_lib.load().gbrs_shard_plan(R, L, H, _ptrs(indptr), _ptrs(indices), int(world), int(device),
                                           bounds.ctypes.data_as(C.c_void_p)))
    return [int(b) for b in bounds]


def shard_block(torch, R, L, H, indptr, indices, values, r0, r1, l_split, device):
    """Local CSC tensors of rows [r0, r1) on the device: (indptr, indices, values or None, straddling rows)."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    dev = indptr[0].device
    ip_out = [torch.empty(L + 1, dtype=torch.int32, device=dev) for _ in range(H)]
    nnz = np.zeros(H, dtype=np.uint64)
    _lib.check(lib.gbrs_shard_index(R, L, H, _ptrs(indptr), _ptrs(indices), int(r0), int(r1), int(device),
                                    _ptrs(ip_out), nnz.ctypes.data_as(C.c_void_p)))
    ix_out = [torch.empty(int(n), dtype=torch.int32, device=dev) for n in nnz]
    v_out = None if values is None else [torch.empty(int(n), dtype=torch.float64, device=dev) for n in nnz]
    straddling = C.c_uint64(0)
    _lib.check(lib.gbrs_shard_gather(R, L, H, _ptrs(indptr), _ptrs(indices), int(r0), int(r1), int(l_split),
                                     None if values is None else _ptrs(values), int(device),
                                     nnz.ctypes.data_as(C.c_void_p), _ptrs(ix_out),
                                     None if values is None else _ptrs(v_out), C.byref(straddling)))
    return ip_out, ix_out, v_out, int(straddling.value)


def check_blocks(bounds):
    """Every rank's block must hold rows: the same decision on every rank (the bounds are)."""
    sizes = np.diff(np.asarray(bounds, dtype=np.int64))
    if (sizes <= 0).any():
        raise RuntimeError(f'--gpus {len(sizes)}: the row blocks {list(map(int, sizes))} leave a rank without reads')


@dataclass
class Shard:
    r0: int
    r1: int
    bounds: list
    straddling: int = 0             # local rows with entries on both sides of l_split
    sides: tuple = (0, 0)           # local entries left / right of l_split
    data: dict = field(default_factory=dict)


class HipOps:
    """What the rank driver does on its device: torch tensors as the allocator, libgbrs_hip for the work, torch.distributed
    for the collectives (RCCL with "nccl"; host copies with "gloo")."""

    def __init__(self, torch, dist, device, backend):
        self.torch, self.dist, self.device, self.backend = torch, dist, device, backend
        self.dev = torch.device(f'cuda:{device}')
        self.world = dist.get_world_size()

    def min_all(self, v):
        t = self.torch.tensor([int(v)], dtype=self.torch.int64, device=self.dev if self.backend == 'nccl' else 'cpu')
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return int(t.item())

    def shard(self, aln, rank, world, l_split):
        torch = self.torch
        L, H, R = aln.shape
        for h in range(H):                       # the kernels read indices[h] up to indptr[h][L]
            if len(aln.indptr[h]) != L + 1 or int(aln.indptr[h][-1]) != len(aln.indices[h]):
                raise RuntimeError(f'Malformed CSC arrays for haplotype {h}.')
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)       # noqa: E731
        ip = [up(p.view(np.int32)) for p in aln.indptr]
        ix = [up(i.view(np.int32)) for i in aln.indices]
        vals = None if aln.values is None else [up(v) for v in aln.values]
        cnt = None if aln.count is None else up(aln.count)
        torch.cuda.synchronize(self.dev)
        bounds = shard_plan(R, L, H, ip, ix, world, self.device)
        check_blocks(bounds)
        r0, r1 = bounds[rank], bounds[rank + 1]
        lip, lix, lv, straddling = shard_block(torch, R, L, H, ip, ix, vals, r0, r1, l_split, self.device)
        lcnt = None if cnt is None else cnt[r0:r1].clone()
        cuts = [int(p[l_split]) for p in lip] if l_split else [0] * H
        left = sum(cuts)
        total = sum(int(t.numel()) for t in lix)
        del ip, ix, vals, cnt                     # the full sample leaves the device before the EM
        torch.cuda.synchronize(self.dev)
        torch.cuda.empty_cache()
        return Shard(r0, r1, bounds, straddling, (left, total - left),
                     dict(indptr=lip, indices=lix, values=lv, count=lcnt, cuts=cuts))

    def engines(self, shard, L, H, eff_len, allowed, l_split):
        """One engine over the block (l_split = 0), or two over the locus ranges [0, l_split) and [l_split, L)."""
        from . import _lib
        from .engine import EmEngine
        torch = self.torch
        d = shard.data
        R = shard.r1 - shard.r0
        vals = d['values']
        flags = _lib.GBRS_EM_KEEP_CSC if vals is not None else 0
        eff = None if eff_len is None else torch.from_numpy(np.ascontiguousarray(eff_len, dtype=np.float64)).to(self.dev)
        cnt_ptr = None if d['count'] is None else d['count'].data_ptr()
        if not l_split:
            parts = [(L, d['indptr'], d['indices'], vals, eff, allowed)]
        else:
            flags |= _lib.GBRS_EM_SIDE_BY_SIDE
            cuts = d['cuts']
            a = (l_split, [p[:l_split + 1] for p in d['indptr']], [x[:c] for x, c in zip(d['indices'], cuts)],
                 None if vals is None else [v[:c] for v, c in zip(vals, cuts)],
                 None if eff is None else eff[:, :l_split].contiguous(), None if allowed is None else allowed[:l_split])
            b = (L - l_split, [(p[l_split:] - c).contiguous() for p, c in zip(d['indptr'], cuts)],
                 [x[c:] for x, c in zip(d['indices'], cuts)], None if vals is None else [v[c:] for v, c in zip(vals, cuts)],
                 None if eff is None else eff[:, l_split:].contiguous(), None if allowed is None else allowed[l_split:])
            parts = [a, b]
        torch.cuda.synchronize(self.dev)
        engs = []
        for nl, ip, ix, vv, el, al in parts:
            e = EmEngine.from_device(R, nl, H, [t.data_ptr() for t in ip], [t.data_ptr() if t.numel() else None for t in ix],
                                     cnt_ptr, None if el is None else el.data_ptr(), device=self.device, flags=flags,
                                     allowed=al)
            if vv is not None:                    # the engine takes the starting values from the host
                e.set_initial_values([v.cpu().numpy() for v in vv])
            engs.append(e)
        shard.data.clear()
        torch.cuda.empty_cache()
        return engs

    def _view(self, ptr, n):
        class _Dev:
            def __init__(self):
                self.__cuda_array_interface__ = dict(shape=(n,), typestr='<f8', data=(ptr, False), version=2)
        return self.torch.as_tensor(_Dev(), device=self.dev)

    def driver(self, engs):
        from .dist import PipelinedShardedEM, ShardedEM, torch_allreduce
        torch, dist = self.torch, self.dist
        if len(engs) == 1:
            eng = engs[0]
            if self.backend == 'nccl':
                return ShardedEM(eng, torch_allreduce(dist, torch, self.dev))
            views = {}

            def host_allreduce(ptr, n):         # gloo: through a host copy
                eng.sync()
                if (ptr, n) not in views:
                    views[(ptr, n)] = self._view(ptr, n)
                v = views[(ptr, n)]
                h = v.cpu()
                dist.all_reduce(h)
                v.copy_(h)
                torch.cuda.synchronize(self.dev)
            return ShardedEM(eng, host_allreduce)
        # Every locus range on a stream of its own with its collective issued in line on that stream: nothing orders
        # the two ranges against each other, so the device overlaps the all-reduce of one with the E-step of the other.
        torch.cuda.synchronize(self.dev)
        streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        for e, st in zip(engs, streams):
            e.set_stream(st.cuda_stream)
        self._streams = streams                  # alive as long as the engines use them
        views, turn = {}, {}
        gloo = self.backend != 'nccl'

        class _Done:
            def wait(self):
                pass

        class _OnStream:                         # an engine that says whose buffer the next all-reduce is
            def __init__(self, eng, st):
                self._eng, self._st = eng, st

            def __getattr__(self, name):
                return getattr(self._eng, name)

            def estep_partial(self):
                turn['stream'] = self._st
                return self._eng.estep_partial()

            def prepare_partial(self):
                turn['stream'] = self._st
                return self._eng.prepare_partial()

        def start_allreduce(ptr, n):
            if ptr not in views:
                views[ptr] = self._view(ptr, n)
            with torch.cuda.stream(turn['stream']):
                if gloo:                         # the copy out waits for the range's stream, the copy back is on it
                    h = views[ptr].cpu()
                    dist.all_reduce(h)
                    views[ptr].copy_(h)
                else:
                    dist.all_reduce(views[ptr])
            return _Done()
        return PipelinedShardedEM(_OnStream(engs[0], streams[0]), _OnStream(engs[1], streams[1]), start_allreduce)

    def results(self, drv, engs):
        """(theta, expected read counts), H x L with the locus ranges side by side."""
        for e in engs:
            e.sync()
        theta = np.concatenate([e.theta() for e in engs], axis=1)
        counts = np.concatenate([e.expected_counts() for e in engs], axis=1)
        return theta, counts

    def close(self, engs):
        for e in engs:
            e.close()


# ---- reports -----------------------------------------------------------------------------------------------------

def group_sums(apm, values):
    """(H x G) sums of the columns of `values` over the members of every gene (apm.group_csr())."""
    gptr, mem = apm.group_csr()
    H = values.shape[0]
    G = len(gptr) - 1
    if G == 0:
        return np.zeros((H, 0))
    cols = np.concatenate([values[:, mem], np.zeros((H, 1))], axis=1)
    out = np.add.reduceat(cols, gptr[:-1], axis=1)
    out[:, np.diff(gptr) == 0] = 0.0
    return np.asfortranarray(out)


class ShardedReports:
    """The report side of EMfactory over the gathered arrays, for quantify._write_expression_reports: same files, same
    order, same writer.  The isoform TPM report rescales theta in place, which the gene-level TPM report inherits."""
    report_pool = None

    def __init__(self, apm, theta, counts):
        self.apm, self.theta, self.counts = apm, theta, counts

    def _level(self, grp_wise, values):
        if grp_wise:
            return self.apm.gname, group_sums(self.apm, values)
        return self.apm.lname, values

    def report_read_counts(self, filename, grp_wise=False, reorder='as-is', notes=None):
        from .em import write_locus_table
        names, values = self._level(grp_wise, self.counts)
        write_locus_table(filename, self.apm.hname, names, values, reorder, notes, pool=self.report_pool)

    def report_depths(self, filename, tpm=True, grp_wise=False, reorder='as-is', notes=None):
        from .em import write_locus_table
        names, values = self._level(grp_wise, self.theta)
        if tpm:
            values *= 1000000.0 / values.sum()
        write_locus_table(filename, self.apm.hname, names, values, reorder, notes, pool=self.report_pool)


# ---- one rank ----------------------------------------------------------------------------------------------------

def gene_starts(apm):
    gptr, mem = apm.group_csr()
    nonempty = np.diff(gptr) > 0
    return np.unique(mem[gptr[:-1][nonempty]])         # members ascend inside a gene: the first is the smallest


def run_rank(args, rank, world, ops, marks, backend='nccl'):
    """The per-rank driver: load, shard, choose the path, run the EM, rank 0 writes the reports."""
    from . import quantify as Q
    from .alignment import load_alignment
    from .dist import balanced_gene_boundary
    from .em import _print_progress, read_length_file
    clock = time.perf_counter
    group_file = Q._default_support_file(args.group_file, Q.DEFAULT_GROUP_FILE,
                                         'A group file is not given. Group-level results will not be reported.')
    length_file = Q._default_support_file(args.length_file, Q.DEFAULT_LENGTH_FILE,
                                          'A length file is not given. Transcript length adjustment will *not* be performed.')
    genotype_file = args.genotype_file
    for label, value in (('Alignment File', args.alignment_file), ('Group File', group_file),
                         ('Length File', length_file), ('Genotype File', genotype_file),
                         ('Outbase', args.outbase), ('Multiread Model', args.multiread_model),
                         ('Pseudocount', args.pseudocount), ('Tolerance', args.tolerance),
                         ('Report Alignment Counts', args.report_alignment_counts),
                         ('Report Posterior', args.report_posterior)):
        logger.info(f'{label}: {value}')
    t0 = clock()
    logger.info(f'Loading EMASE file: {args.alignment_file}')
    aln = load_alignment(args.alignment_file, grpfile=group_file)
    eff = None
    if length_file is not None:
        eff = read_length_file(aln, length_file, 100)
        if not np.all(eff > 0.0):
            raise RuntimeError('There exist transcripts missing length information.')
    gene_notes = isoform_notes = allowed = None
    if genotype_file is None:
        outbase = f'{args.outbase}.multiway'
    else:
        outbase = f'{args.outbase}.diploid'
        logger.info(f'Loading and processing genotype calls from: {genotype_file}')
        allowed, gene_notes, isoform_notes = Q.genotype_mask_from_file(aln, genotype_file) or \
            Q.diplotype_mask(aln, Q.read_genotype_table(genotype_file))
    marks['load'] = clock() - t0

    # the two-engine form needs a gene boundary near half the entries (the same cut on every rank: the full indptr
    # is on every rank) that no row of any block straddles, with entries on both sides of it in every block
    L, H, R = aln.shape
    l_split = 0
    if args.pseudocount == 0.0 and group_file is not None and aln.num_groups:
        cut = balanced_gene_boundary(aln.indptr, gene_starts(aln))
        l_split = cut if 0 < cut < L else 0
    t0 = clock()
    shard = ops.shard(aln, rank, world, l_split)
    marks['shard'] = clock() - t0
    two = bool(l_split) and shard.straddling == 0 and min(shard.sides) > 0
    two = ops.min_all(int(two)) == 1
    marks['path'] = 'two-engine' if two else 'single-engine'
    logger.info(f'Sharded EM: world {world}, backend {backend}, {marks["path"]} path'
                + (f' (loci cut at {l_split} of {L})' if two else '') + f', rows {shard.r0}-{shard.r1} on rank {rank}')

    logger.info('Running EMASE')
    t0 = clock()
    engs = ops.engines(shard, L, H, eff, allowed, l_split if two else 0)
    drv = ops.driver(engs)
    drv.prepare(args.pseudocount)
    marks['em_setup'] = clock() - t0
    np.seterr(all='raise', under='ignore')      # the state the reference leaves numpy in (EMfactory.run)
    t0 = clock()
    drv.run(model=4, tol=args.tolerance, max_iters=args.max_iters)
    theta, counts = ops.results(drv, engs)
    marks['em_run'] = clock() - t0
    marks['em_iterations'] = drv.num_iters
    ops.close(engs)
    if ops.min_all(1) != 1:                      # every rank got here: rank 0 may write
        raise RuntimeError('a rank did not finish the EM')
    if rank != 0:
        return
    _print_progress(drv.err_history, np.full(len(drv.err_history), marks['em_run']))
    t0 = clock()
    Q._write_expression_reports(ShardedReports(aln, theta, counts), outbase, group_file is not None, isoform_notes,
                                gene_notes, False)
    marks['reports'] = clock() - t0
    if args.report_alignment_counts:
        t0 = clock()
        from .counts import AlignmentCounter, report_alignment_counts as write_counts
        # the counts of the alignments as loaded: the `-G` mask only ever went to the engines
        with AlignmentCounter(aln, device=getattr(ops, 'device', 0)) as counter:
            for level, grp_wise in (('isoform', False), ('gene', True)):
                if grp_wise and group_file is None:
                    continue
                path = f'{outbase}.{level}s.alignment_counts'
                logger.info(f'Generating {level} Alignment Counts: {path}')
                write_counts(aln, path, grp_wise=grp_wise, device=getattr(ops, 'device', 0), counter=counter)
        marks['alignment_counts'] = clock() - t0
    logger.debug('Done')


def rank_main(argv=None):
    """Child process of launch(): RANK / WORLD_SIZE / MASTER_* / GBRS_SHARD_DEVICE / GBRS_SHARD_BACKEND from the
    environment, the quantify arguments on the command line.  Exit status 0 on success, 1 on failure."""
    import datetime
    from .cli import build_parser, configure_logging
    args = build_parser().parse_args(argv)
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    device = int(os.environ['GBRS_SHARD_DEVICE'])
    backend = os.environ.get('GBRS_SHARD_BACKEND', 'nccl')
    log = configure_logging(args.verbose)
    if rank != 0:
        log.setLevel(logging.ERROR)             # rank 0 speaks for the command
    marks = {'rank': rank, 'device': device}
    failure = None
    t_main = time.perf_counter()
    try:
        import torch
        import torch.distributed as dist
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if not 0 <= device < n:
            raise RuntimeError(f'rank {rank}: device {device} is not one of the {n} visible devices')
        torch.cuda.set_device(device)
        timeout = datetime.timedelta(seconds=float(os.environ.get('GBRS_DIST_TIMEOUT', DEFAULT_TIMEOUT_S)))
        if backend == 'nccl':
            dist.init_process_group('nccl', timeout=timeout, device_id=torch.device(f'cuda:{device}'))
        else:
            dist.init_process_group(backend, timeout=timeout)
        run_rank(args, rank, world, HipOps(torch, dist, device, backend), marks, backend=backend)
        dist.destroy_process_group()
    except Exception as e:   # noqa: BLE001 - reported, and the exit status tells the launcher
        failure = e
        if log.level == logging.DEBUG:
            log.exception(e)
        else:
            log.critical(f'{type(e).__name__}: {e}')
    marks['main'] = time.perf_counter() - t_main
    path = os.getenv('GBRS_STAGE_TIMES')
    if path:
        if failure is not None:
            marks['error'] = f'{type(failure).__name__}: {failure}'
        with open(path, 'w') as fh:
            json.dump(marks, fh)
    return 0 if failure is None else 1


if __name__ == '__main__':
    code = rank_main()
    if os.getenv('GBRS_ORDERLY_EXIT'):          # as for the `gbrs` process (cli.run): tools that finish at exit
        sys.exit(code)
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(code)       # no orderly teardown of a process group that another rank may have left
