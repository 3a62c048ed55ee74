"""`gbrs reconstruct` on MI355X: same inputs, outputs and defaults as
gbrs_utils.reconstruct (gbrs/gbrs_utils.py:382-609); the emission model, forward, backward,
posterior, Viterbi and backtrace all run in HIP kernels through include/gbrs_hip.h.
No CPU fallback: without libgbrs_hip.so / a gfx950 device every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import logging
import os
import time
import types
from collections import OrderedDict
from itertools import combinations_with_replacement

import numpy as np

from . import _lib
from .npzfast import FastNpz, savez_compressed

logger = logging.getLogger('gbrs')


class DiplotypeHMM:
    """Device handle for one set of transition tables (sample independent)."""

    def __init__(self, num_haps, chroms, n_genes, tprob, device=0):
        """chroms: names; n_genes[c]; tprob[c] float64 [n_t, S, S] log T[i][to, from]."""
        lib = _lib.load()
        self.H = int(num_haps)
        self.S = self.H * (self.H + 1) // 2
        self.chroms = list(chroms)
        self.n_genes = np.asarray(n_genes, dtype=np.int32)
        self._tp = [np.ascontiguousarray(t, dtype=np.float64) for t in tprob]
        for c, t in zip(self.chroms, self._tp):
            if t.ndim != 3 or t.shape[1:] != (self.S, self.S):
                raise ValueError(f'tprob[{c}] has shape {t.shape}, expected (n, {self.S}, {self.S})')
        self.n_trans = np.asarray([len(t) for t in self._tp], dtype=np.int32)
        for c, n, nt in zip(self.chroms, self.n_genes, self.n_trans):
            if nt < n - 1:
                raise IndexError(f'index {n - 2} is out of bounds for axis 0 with size {nt}')
        h = C.c_void_p()
        _lib.check(lib.gbrs_hmm_create(self.H, len(self.chroms), _lib.ptr(self.n_genes),
                                       _lib.ptr(self.n_trans), _lib.ptr_table(self._tp), device,
                                       C.byref(h)))
        self._h = h
        self.n_samples = 0

    def close(self):
        if getattr(self, '_h', None) is not None:
            _lib.load().gbrs_hmm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_expression(self, expr, avecs=None, has_avec=None, expr_threshold=1.5, sigma=0.12):
        """expr[c] [n_samples, n_c, H] (or [n_c, H]); avecs[c] [n_c, H, H]; has_avec[c] bool [n_c].
        avecs / has_avec are sample independent and stay on the device once given: pass them with the
        first sample (or batch) and leave them out afterwards."""
        if (avecs is None) != (has_avec is None):
            raise ValueError('avecs and has_avec go together')
        ex, av, ha = [], [], []
        ns = None
        for c, n in enumerate(self.n_genes):
            e = np.ascontiguousarray(expr[c], dtype=np.float64)
            if e.ndim == 2:
                e = e[None]
            if e.shape[1:] != (n, self.H):
                raise ValueError(f'expr[{c}] has shape {e.shape}')
            ns = e.shape[0] if ns is None else ns
            if e.shape[0] != ns:
                raise ValueError('inconsistent number of samples')
            ex.append(e)
            if avecs is not None:
                a = np.ascontiguousarray(avecs[c], dtype=np.float64)
                if a.shape != (n, self.H, self.H):
                    raise ValueError(f'avecs[{c}] has shape {a.shape}')
                av.append(a)
                ha.append(np.ascontiguousarray(has_avec[c], dtype=np.uint8))
        _lib.check(_lib.load().gbrs_hmm_set_expression(
            self._h, ns, _lib.ptr_table(ex), _lib.ptr_table(av) if av else None,
            _lib.ptr_table(ha) if ha else None, float(expr_threshold), float(sigma)))
        self.n_samples = ns

    def set_eprob(self, eprob):
        ep = []
        ns = None
        for c, n in enumerate(self.n_genes):
            e = np.ascontiguousarray(eprob[c], dtype=np.float64)
            if e.ndim == 2:
                e = e[None]
            if e.shape[1:] != (n, self.S):
                raise ValueError(f'eprob[{c}] has shape {e.shape}')
            ns = e.shape[0] if ns is None else ns
            ep.append(np.ascontiguousarray(e))
        _lib.check(_lib.load().gbrs_hmm_set_eprob(self._h, ns, _lib.ptr_table(ep)))
        self.n_samples = ns

    def run(self):
        _lib.check(_lib.load().gbrs_hmm_run(self._h))

    def get(self, chrom, sample=0, want=('gamma', 'states', 'calls')):
        c = chrom if isinstance(chrom, int) else self.chroms.index(chrom)
        n, S = int(self.n_genes[c]), self.S
        m = min(n, int(self.n_trans[c]))
        bufs = dict(gamma=np.empty((S, n)), states=np.empty(m + 1, dtype=np.int32),
                    calls=np.empty(n, dtype=np.int32), alpha=np.empty((S, n)), beta=np.empty((S, n)),
                    delta=np.empty((S, n)), scaler=np.empty(n), eprob=np.empty((n, S)))
        args = [(_lib.ptr(bufs[k]) if k in want else None)
                for k in ('gamma', 'states', 'calls', 'alpha', 'beta', 'delta', 'scaler', 'eprob')]
        _lib.check(_lib.load().gbrs_hmm_get(self._h, sample, c, *args))
        return {k: bufs[k] for k in want}

    def _by_chrom(self, table):
        """A per-chromosome argument - a sequence in the handle's order or a dict by chromosome name - as a list over
        the handle's chromosomes, None where it has nothing."""
        if isinstance(table, dict):
            return [table.get(c) for c in self.chroms]
        return list(table) + [None] * (len(self.chroms) - len(table))

    def set_grid(self, gene_positions, grid):
        """The marker grid of the handle (sample independent, uploaded once).  Both arguments go by handle chromosome:
        a sequence in the handle's order or a dict by chromosome name.  grid[c]: grid positions in file order, None,
        empty or absent for a chromosome that is not on the grid; gene_positions[c]: the positions of its genes in
        genome order.  The knots are made as postproc.interpolate_arrays makes them; a grid point outside them raises
        interp1d's ValueError, a grid chromosome without gene positions the chain's IndexError."""
        points = [np.zeros(0) if g is None else np.ascontiguousarray(g, dtype=np.float64) for g in self._by_chrom(grid)]
        where = [np.zeros(0) if len(g) == 0 or x is None else np.ascontiguousarray(x, dtype=np.float64)
                 for g, x in zip(points, self._by_chrom(gene_positions))]
        n_grid = np.asarray([len(g) for g in points], dtype=np.int32)
        n_pos = np.asarray([len(x) for x in where], dtype=np.int32)
        lib = _lib.load()
        status = lib.gbrs_hmm_set_grid(self._h, _lib.ptr(n_pos), _lib.ptr_table(where), _lib.ptr(n_grid),
                                       _lib.ptr_table(points))
        _raise_grid_error(lib, status)
        self.grid_points = [int(m) for m in n_grid]
        self.grid_offsets = [int(o) for o in np.concatenate(([0], np.cumsum(n_grid)[:-1]))]

    def grid(self, sample=None, want=('dosage',)):
        """The last run on the handle's grid, one device pass: `dosage` [n, M, H] founder dosages, the grid points of the
        handle's chromosomes one after the other (chromosome c: rows grid_offsets[c] .. + grid_points[c]); `gamma_grid`
        per sample a list over the handle's chromosomes of (S x grid_points[c]) arrays, None off the grid.  sample=None:
        every sample of the run (n of them); an index: that sample, without the leading axis / list."""
        n = self.n_samples if sample is None else 1
        M = sum(getattr(self, 'grid_points', ()))
        out = {}
        dosage = np.empty((n, M, self.H)) if 'dosage' in want else None
        flat = np.empty((n, self.S * M)) if 'gamma_grid' in want else None
        _lib.check(_lib.load().gbrs_hmm_grid(self._h, -1 if sample is None else int(sample), _lib.ptr(dosage),
                                             _lib.ptr(flat)))
        if dosage is not None:
            out['dosage'] = dosage if sample is None else dosage[0]
        if flat is not None:
            per_sample = [[flat[k, self.S * o:self.S * (o + m)].reshape(self.S, m) if m else None
                           for o, m in zip(self.grid_offsets, self.grid_points)] for k in range(n)]
            out['gamma_grid'] = per_sample if sample is None else per_sample[0]
        return out

    def grid_info(self):
        """(grid points on the handle, device milliseconds of the last grid pass)."""
        m, ms = C.c_int64(), C.c_double()
        _lib.check(_lib.load().gbrs_hmm_grid_info(self._h, C.byref(m), C.byref(ms)))
        return m.value, ms.value

    def set_panel(self, arrays):
        """The reference panel of the handle: one (M x H) dosage array per entry on the handle's grid
        points, rows as `grid()['dosage']` has them (handle chromosome c: rows grid_offsets[c] .. + grid_points[c]).
        Uploaded once; an empty sequence drops the panel.  set_grid drops it too."""
        M = sum(getattr(self, 'grid_points', ()))
        panel = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
        for j, a in enumerate(panel):
            if a.shape != (M, self.H):
                raise ValueError(f'panel entry {j} has shape {a.shape}, expected ({M}, {self.H})')
        _lib.check(_lib.load().gbrs_hmm_set_panel(self._h, len(panel), _lib.ptr_table(panel)))

    def match(self, sample=None):
        """The last run against the panel, one device pass: `cross` [n, n_chrom, n_panel], the sums of products of a
        sample's and an entry's grid dosages per handle chromosome, and `sample_norm` [n, n_chrom], the sums of the
        sample's squares.  sample=None: every sample of the run; an index: that sample, without the leading axis."""
        n = self.n_samples if sample is None else 1
        n_panel = self.match_info()['n_panel']
        cross, norm = np.empty((n, len(self.chroms), n_panel)), np.empty((n, len(self.chroms)))
        _lib.check(_lib.load().gbrs_hmm_match(self._h, -1 if sample is None else int(sample), _lib.ptr(cross),
                                              _lib.ptr(norm)))
        return {'cross': cross if sample is None else cross[0], 'sample_norm': norm if sample is None else norm[0]}

    def match_info(self):
        """n_panel, panel_norm [n_panel, n_chrom], the device milliseconds of the last match pass's kernels and the
        device bytes the panel and the pass's outputs hold."""
        lib = _lib.load()
        m, ms, nbytes = C.c_int32(), C.c_double(), C.c_uint64()
        _lib.check(lib.gbrs_hmm_match_info(self._h, C.byref(m), None, C.byref(ms), C.byref(nbytes)))
        norm = np.zeros((m.value, len(self.chroms)))
        if m.value:
            _lib.check(lib.gbrs_hmm_match_info(self._h, None, _lib.ptr(norm), None, None))
        return {'n_panel': m.value, 'panel_norm': norm, 'last_ms': ms.value, 'device_bytes': nbytes.value}

    def set_snps(self, gene_positions, positions, masks):
        """The SNPs of the handle (sample independent, uploaded once).  The arguments go by handle
        chromosome like set_grid's: a sequence in the handle's order or a dict by chromosome name.  positions[c]: the
        SNP positions of the chromosome in file order (None, empty or absent: it has none), masks[c]: their founder
        allele patterns as uint32, bit h set when founder h carries the alternative allele; gene_positions[c]: the
        positions of its genes.  The SNPs of a chromosome are a grid: a SNP outside the knots raises the grid's
        ValueError.  All empty drops the SNPs.  Independent of set_grid and set_panel."""
        points = [np.zeros(0) if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in self._by_chrom(positions)]
        bits = [np.zeros(0, dtype=np.uint32) if m is None else np.ascontiguousarray(m, dtype=np.uint32)
                for m in self._by_chrom(masks)]
        for c, x, m in zip(self.chroms, points, bits):
            if x.shape != m.shape or x.ndim != 1:
                raise ValueError(f'chromosome {c}: {x.shape} SNP positions and {m.shape} patterns')
        where = [np.zeros(0) if len(x) == 0 or g is None else np.ascontiguousarray(g, dtype=np.float64)
                 for x, g in zip(points, self._by_chrom(gene_positions))]
        n_snps = np.asarray([len(x) for x in points], dtype=np.int32)
        n_pos = np.asarray([len(g) for g in where], dtype=np.int32)
        lib = _lib.load()
        status = lib.gbrs_hmm_set_snps(self._h, _lib.ptr(n_pos), _lib.ptr_table(where), _lib.ptr(n_snps),
                                       _lib.ptr_table(points), _lib.ptr_table(bits))
        _raise_grid_error(lib, status)
        self.snp_points = [int(m) for m in n_snps]
        self.snp_offsets = [int(o) for o in np.concatenate(([0], np.cumsum(n_snps)[:-1]))]

    def impute(self, sample=None, chunk=1 << 20):
        """The expected number of alternative alleles at every SNP of the handle from the last run: [n, M], the SNPs of
        the handle's chromosomes one after the other (chromosome c: columns snp_offsets[c] .. + snp_points[c]).
        sample=None: every sample of the run (n of them); an index: that sample, [M].  The range is walked in chunks of
        `chunk` SNPs, one device pass and one copy each; the founder dosages at the genes are made by the first."""
        if chunk < 1:
            raise ValueError('chunk must be at least 1')
        lib = _lib.load()
        n = self.n_samples if sample is None else 1
        which = -1 if sample is None else int(sample)
        M = self.impute_info()['n_snps']
        out = np.empty((n, M))
        if M <= chunk:
            _lib.check(lib.gbrs_hmm_impute(self._h, which, 0, M, _lib.ptr(out)))
        else:
            for first in range(0, M, chunk):
                part = np.empty((n, min(chunk, M - first)))
                _lib.check(lib.gbrs_hmm_impute(self._h, which, first, part.shape[1], _lib.ptr(part)))
                out[:, first:first + part.shape[1]] = part
        return out if sample is None else out[0]

    def impute_info(self):
        """n_snps on the handle, the device milliseconds of the last imputation pass's kernels (`last_ms`; its parts
        `dosage_ms` and `kernel_ms`, and `setup_ms` of the last set_snps) and the device bytes the SNPs, the gene
        dosages and the output chunk hold."""
        lib = _lib.load()
        m, ms, nbytes = C.c_int64(), C.c_double(), C.c_uint64()
        setup, dosage, kernel = C.c_double(), C.c_double(), C.c_double()
        _lib.check(lib.gbrs_hmm_impute_info(self._h, C.byref(m), C.byref(ms), C.byref(nbytes)))
        _lib.check(lib.gbrs_hmm_impute_times(self._h, C.byref(setup), C.byref(dosage), C.byref(kernel)))
        return {'n_snps': m.value, 'last_ms': ms.value, 'device_bytes': nbytes.value, 'setup_ms': setup.value,
                'dosage_ms': dosage.value, 'kernel_ms': kernel.value}

    def sample_paths(self, n_draws, seed=0, sample=None, streams=None):
        """Diplotype paths drawn from the joint posterior of the last run, one device pass per slab of
        draws.  sample=None: every sample of the run (n of them); an index: that sample, without the leading axis.
        streams: one 32-bit id per sample of the call (default: the sample's index in the run); a sample's draws depend
        on (seed, its stream), not on where in a batch it ran.  Returns `paths`, per chromosome a uint8 array
        (n?, n_draws, n_c) of state indices; `changes`, int32 (n?, n_draws, n_chrom) founder changes along each draw;
        `degenerate`, the decisions that fell back to the argmax."""
        n = self.n_samples if sample is None else 1
        n_draws = int(n_draws)
        ids = None
        if streams is not None:
            ids = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError(f'{len(ids)} streams for {n} samples')
        total = int(self.n_genes.sum())
        flat = np.empty((n, max(n_draws, 0), total), dtype=np.uint8)
        changes = np.empty((n, max(n_draws, 0), len(self.chroms)), dtype=np.int32)
        degenerate = C.c_uint64(0)
        _lib.check(_lib.load().gbrs_hmm_sample_paths(self._h, -1 if sample is None else int(sample), n_draws,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(ids), _lib.ptr(flat),
                                                     _lib.ptr(changes), C.byref(degenerate)))
        offs = np.concatenate(([0], np.cumsum(self.n_genes)))
        paths = [flat[:, :, offs[c]:offs[c + 1]] for c in range(len(self.chroms))]
        if sample is not None:
            paths, changes = [p[0] for p in paths], changes[0]
        return {'paths': paths, 'changes': changes, 'degenerate': int(degenerate.value)}

    def sample_info(self):
        """(device milliseconds of the last sample_paths call's kernels, device bytes its buffers hold)."""
        ms, nbytes = C.c_double(), C.c_uint64()
        _lib.check(_lib.load().gbrs_hmm_sample_info(self._h, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    DIAGNOSTICS = ('xo', 'pswitch', 'errlod', 'maxprob', 'maxmarg')

    def diagnostics(self, sample=None, want=DIAGNOSTICS):
        """Diagnostics of the last run, one device pass over the pair posteriors for `xo` / `pswitch` and
        one over the genes for the rest; only what `want` names is computed.  sample=None: every sample of the run (n of
        them); an index: that sample, without the leading axis.  Returns per name a list over the handle's chromosomes of
        arrays (n?, n_c) - `xo` (expected founder changes between genes i and i + 1) and `pswitch` (the probability that
        the diplotype changes there) cut to n_c - 1; `errlod` the error LOD of every gene, `maxmarg` (int32) the first
        most likely diplotype and `maxprob` its posterior."""
        unknown = [k for k in want if k not in self.DIAGNOSTICS]
        if unknown:
            raise ValueError(f'unknown diagnostics: {unknown}')
        n = self.n_samples if sample is None else 1
        total = int(self.n_genes.sum())
        flat = {k: np.empty((n, total), dtype=np.int32 if k == 'maxmarg' else np.float64) if k in want else None
                for k in self.DIAGNOSTICS}
        _lib.check(_lib.load().gbrs_hmm_diagnostics(self._h, -1 if sample is None else int(sample),
                                                    *[_lib.ptr(flat[k]) for k in self.DIAGNOSTICS]))
        offs = np.concatenate(([0], np.cumsum(self.n_genes)))
        out = {}
        for k in want:
            cut = 1 if k in ('xo', 'pswitch') else 0
            per = [flat[k][:, offs[c]:max(offs[c + 1] - cut, offs[c])] for c in range(len(self.chroms))]
            out[k] = per if sample is None else [a[0] for a in per]
        return out

    def pair_posterior(self, chrom, sample=0):
        """(n_c - 1, S, S): xi[i][k][j], the posterior that the sample has diplotype k at gene i and j at gene i + 1 of
        the chromosome (an index or a name), from the last run."""
        c = chrom if isinstance(chrom, int) else self.chroms.index(chrom)
        n = int(self.n_genes[c]) if 0 <= c < len(self.chroms) else 1     # out of range: the library says so
        xi = np.empty((max(n - 1, 1), self.S, self.S))
        _lib.check(_lib.load().gbrs_hmm_pair_posterior(self._h, int(sample), c, _lib.ptr(xi)))
        return xi[:max(n - 1, 0)]

    def diagnostics_info(self):
        """Device milliseconds of the last diagnostics call's kernels."""
        ms = C.c_double()
        _lib.check(_lib.load().gbrs_hmm_diagnostics_info(self._h, C.byref(ms)))
        return ms.value

    def loglik(self, sample=None):
        """float64 (n, n_chrom): the data log-likelihood of the last run per sample and chromosome under the handle's own
        tables, minus the sum of the run's `scaler` row; one reduction over what the forward pass kept.
        sample=None: every sample of the run (n of them); an index: that sample (n = 1)."""
        n = self.n_samples if sample is None else 1
        out = np.empty((n, len(self.chroms)))
        _lib.check(_lib.load().gbrs_hmm_loglik(self._h, -1 if sample is None else int(sample), _lib.ptr(out)))
        return out

    def loglik_tables(self, chrom, tables, sample=None):
        """float64 (K, n): the data log-likelihood of the last run's emissions on one chromosome (an index or a name) under
        each of K other transition tables, float64 (n_t, S, S) in natural log with n_t >= n_c - 1; one launch runs the
        forward recursion for all (table, sample) pairs.  The handle's tables and results stay as they are."""
        c = chrom if isinstance(chrom, int) else self.chroms.index(chrom)
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        for k, t in enumerate(tabs):
            if t.ndim != 3 or t.shape[1:] != (self.S, self.S):
                raise ValueError(f'table {k} has shape {t.shape}, expected (n, {self.S}, {self.S})')
        n = self.n_samples if sample is None else 1
        n_trans = np.asarray([len(t) for t in tabs], dtype=np.int32)
        out = np.empty((len(tabs), n))
        _lib.check(_lib.load().gbrs_hmm_loglik_tables(self._h, c, len(tabs), _lib.ptr(n_trans), _lib.ptr_table(tabs),
                                                      -1 if sample is None else int(sample), _lib.ptr(out)))
        return out

    def loglik_info(self):
        """(device milliseconds of the last loglik / loglik_tables call's kernels, device bytes their buffers hold)."""
        ms, nbytes = C.c_double(), C.c_uint64()
        _lib.check(_lib.load().gbrs_hmm_loglik_info(self._h, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def info(self):
        inf = _lib.HmmInfo()
        _lib.check(_lib.load().gbrs_hmm_info(self._h, C.byref(inf)))
        return inf


def _raise_grid_error(lib, status):
    """The exceptions `gbrs interpolate` raises for the same grid: interp1d's ValueError, numpy's IndexError."""
    if status == _lib.GBRS_ERR_INVALID:
        message = lib.gbrs_last_error()
        if b'interpolation range' in message:
            raise ValueError(message.decode())
        if b'is out of bounds' in message:
            raise IndexError(message.decode())
    _lib.check(status)


def grid_knots(gene_positions, grid):
    """(knots, gene of each knot) of one chromosome, as the grid pass uses them: [0.0, gene positions..., last grid
    point + 1.0] sorted stably, the two end knots carrying the first and the last gene's column
    (postproc.interpolate_arrays).  Host code only."""
    where = np.ascontiguousarray(gene_positions, dtype=np.float64)
    points = np.ascontiguousarray(grid, dtype=np.float64)
    knots = np.empty(len(where) + 2)
    gene = np.empty(len(where) + 2, dtype=np.int32)
    lib = _lib.load()
    _raise_grid_error(lib, lib.gbrs_grid_knots(len(where), _lib.ptr(where), len(points), _lib.ptr(points),
                                               _lib.ptr(knots), _lib.ptr(gene)))
    return knots, gene


def get_chromosome_info(data_dir=None):
    """Chromosome names (cut to 8 characters) -> lengths, in the order of $GBRS_DATA/ref.fa.fai: the
    order in which `gbrs reconstruct` walks the genome (gbrs_utils.py:24-38)."""
    data_dir = os.getenv('GBRS_DATA', '.') if data_dir is None else data_dir
    fai = os.path.join(data_dir, 'ref.fa.fai')
    if not os.path.isfile(fai):
        raise ValueError('Make sure if $GBRS_DATA is set correctly, and that "ref.fa.fai" is in that '
                         f'directory. Currently it is: {data_dir}')
    lengths = OrderedDict()
    with open(fai) as fh:
        for fields in map(str.split, fh):
            if len(fields) >= 2:
                lengths[fields[0][:8]] = int(fields[1])
    return lengths


def read_gene_tpm(expression_file):
    """(haplotype letters, {gene id: row}, TPM matrix [genes x H]) from a `.genes.tpm` report.  The first
    column is the gene id and the last the total; `gbrs reconstruct` assumes there is no notes column,
    i.e. the multiway report (gbrs_utils.py:450-459).  The numbers of the whole file go
    through one C-level parse instead of a float() per cell."""
    with open(expression_file) as fh:
        haplotypes = fh.readline().rstrip().split('\t')[1:-1]
        body = fh.read()
    lines = body.splitlines()
    width = len(haplotypes) + 1
    if lines and len(lines) == body.count('\n') + (0 if body.endswith('\n') else 1):
        # plain table: the library parses the numbers (std::from_chars, ~10 ns each against strtod's ~100)
        raw = body.encode()
        table = np.empty((len(lines), width), dtype=np.float64)
        try:
            status = _lib.load().gbrs_parse_number_table(raw, len(raw), len(lines), width, _lib.ptr(table))
        except (ImportError, OSError):
            status = 1
        if status == 0:
            ids = [line.partition('\t')[0] for line in lines]
            return haplotypes, {g: k for k, g in enumerate(ids)}, table[:, :-1]
    ids, cells = [], []
    for line in lines:
        gid, _, rest = line.rstrip().partition('\t')
        ids.append(gid)
        cells.append(rest)
    flat = np.fromstring('\t'.join(cells), dtype=np.float64, sep='\t') if cells else np.zeros(0)
    if flat.size != len(ids) * width:
        raise ValueError(f'{expression_file}: every line must hold {width} numbers after the gene id')
    table = flat.reshape(len(ids), width)[:, :-1]
    return haplotypes, {g: k for k, g in enumerate(ids)}, table


def read_gene_order(gpos_file):
    """{chromosome: [gene ids in genome order]} from `ref.gene_pos.ordered.npz`, whose arrays hold
    (gene id, position) records with the id as bytes or str (gbrs_utils.py:437-447)."""
    order = {}
    z = FastNpz(gpos_file)
    for c in z.files:
        a = z[c]
        if a.dtype.names:                                   # structured records: first field is the id
            col = a[a.dtype.names[0]]
            order[c] = col.astype('U').tolist()
        else:
            order[c] = [gid.decode() if isinstance(gid, bytes) else str(gid) for gid, *_ in a]
    z.close()
    return order


def read_gene_positions(gpos_file):
    """{chromosome: positions of its genes in genome order, float64} from `ref.gene_pos.ordered.npz`: the second field
    of its (gene id, position) records, which is what `gbrs interpolate` takes (gbrs_utils.py:664)."""
    where = {}
    z = FastNpz(gpos_file)
    for c in z.files:
        a = z[c]
        if a.dtype.names:
            where[c] = a[a.dtype.names[1]].astype(np.float64)
        else:
            where[c] = np.asarray([record[1] for record in a], dtype=np.float64)
    z.close()
    return where


class ReconstructContext:
    """Everything `gbrs reconstruct` reads that does not depend on the sample - genome order, gene order, transition
    tables, specificity blocks, and with `grid_file` the marker grid - and the device handle that holds the tables.
    One command builds one and drops it; a resident process (gbrs_amd.worker) keeps it across samples, so that a sample
    costs its expression rows only."""

    def __init__(self, tprob_file, avec_file=None, gpos_file=None, device=0, grid_file=None, alt_tprob_files=None):
        data_dir = os.getenv('GBRS_DATA', '.')
        self.tprob_file = tprob_file
        self.alt_tprob_files = list(alt_tprob_files or ())     # candidates beside `tprob_file` (--alt-tprob-file)
        self.loglik_launches = 0          # device passes made for likelihoods: reductions + candidate chains
        self.avec_file = avec_file or os.path.join(data_dir, 'avecs.npz')
        self.gpos_file = gpos_file or os.path.join(data_dir, 'ref.gene_pos.ordered.npz')
        self.grid_file = grid_file
        self.device = device
        self.data_dir = data_dir
        self.loaded = False
        self.hmm = None
        self.num_haps = None
        self.grid = None                  # {chromosome: positions} in the grid file's order
        self.grid_uploads = 0             # times the grid went to a device handle
        self.grid_slices = {}             # chromosome on the handle and on the grid -> (handle index, first dosage row, rows)
        self.panel = None                 # (ids, dosage arrays in handle order) of --match-panel (_load_panel)
        self.panel_file = None
        self.panel_uploads = 0            # times the panel went to a device handle, alternative-table handles included
        self._panel_on_handle = False
        self.snps = None                  # read_snp_file's dict of --snp-file (_load_snps)
        self.snp_file = None
        self.snp_uploads = 0              # times the SNPs went to a device handle, alternative-table handles included
        self._snps_on_handle = False

    def load(self, marks=None):
        """The files (the big transition tables inflate on the library's threads while the small files are parsed)."""
        if self.loaded:
            return
        logger.info('Loading chromosome information')
        genome = list(get_chromosome_info(self.data_dir))
        from concurrent.futures import ThreadPoolExecutor
        tprob = FastNpz(self.tprob_file)
        self.chroms = [c for c in genome if c in tprob]              # chromosomes without a table are skipped (:495)
        reader = ThreadPoolExecutor(max_workers=1)
        tables_pending = reader.submit(tprob.read_many, self.chroms)
        self._alts_pending = []
        for f in self.alt_tprob_files:    # behind the base tables on the reader thread
            z = FastNpz(f)
            for c in genome:              # the candidates are compared, and a sample may be run again, on the same chromosomes
                if (c in z) != (c in tprob):
                    reader.shutdown(wait=False, cancel_futures=True)
                    raise RuntimeError(f'{f}: ' + (f'no transition table for chromosome {c}' if c in tprob else
                                                  f'a transition table for chromosome {c}, which {self.tprob_file} lacks'))
            self._alts_pending.append(reader.submit(z.read_many, self.chroms))
        logger.info(f'Loading alignment specificity: {self.avec_file}')
        self.avecs = FastNpz(self.avec_file)
        logger.info(f'Loading gene meta data: {self.gpos_file}')
        self.gene_order = read_gene_order(self.gpos_file)
        if self.grid_file is not None:
            from .postproc import read_grid
            logger.info(f'Loading grid file: {self.grid_file}')
            self.grid = read_grid(self.grid_file)
            self.gene_positions = read_gene_positions(self.gpos_file)
        self._tables_pending, self._reader = tables_pending, reader
        self.loaded = True

    def tables(self):
        if self._tables_pending is not None:
            logger.info(f'Loading transition probabilities: {self.tprob_file}')
            self._tables = self._tables_pending.result()             # stored members: views of the page cache, no copy
            self._reader.shutdown(wait=False)
            self._tables_pending = None
        return self._tables

    def alt_tables(self, num_haps):
        """Per alternative file its tables by handle chromosome, checked against the base: the state count of `num_haps`
        founders and at least n_genes - 1 blocks, else a RuntimeError that names the file and the chromosome.
        `alt_same[a][ci]`: the table is np.array_equal to the base's, so its likelihood is the base run's own."""
        if getattr(self, '_alt_tables', None) is None:
            base = self.tables()
            S = num_haps * (num_haps + 1) // 2
            found, same = [], []
            for f, job in zip(self.alt_tprob_files, self._alts_pending):
                logger.info(f'Loading alternative transition probabilities: {f}')
                tabs = job.result()
                for c, t in zip(self.chroms, tabs):
                    n = len(self.gene_order[c])
                    if t.ndim != 3 or t.shape[1:] != (S, S):
                        raise RuntimeError(f'{f}: the table of chromosome {c} has shape {t.shape}, expected (n, {S}, {S})')
                    if len(t) < n - 1:
                        raise RuntimeError(f'{f}: the table of chromosome {c} has {len(t)} blocks for {n} genes')
                found.append(tabs)
                same.append([np.array_equal(t, b) for t, b in zip(tabs, base)])
            self._alt_tables, self.alt_same, self._alts_pending = found, same, []
        return self._alt_tables

    def alt_context(self, a):
        """The context of alternative file `a`: its own device handle on this context's chromosomes, gene order,
        specificity blocks and grid.  Made at first need and kept until close()."""
        subs = self.__dict__.setdefault('_alt_contexts', {})
        if a not in subs:
            sub = ReconstructContext(self.alt_tprob_files[a], self.avec_file, self.gpos_file, self.device, self.grid_file)
            sub.chroms, sub.gene_order, sub.grid = self.chroms, self.gene_order, self.grid
            sub.gene_positions = getattr(self, 'gene_positions', None)
            sub._spec, sub.num_haps = self._spec, self.num_haps
            sub._tables, sub._tables_pending = self._alt_tables[a], None
            sub.loaded = True
            sub._panel_owner = self
            subs[a] = sub
        if subs[a].panel_file != self.panel_file:
            subs[a].panel, subs[a].panel_file, subs[a]._panel_on_handle = self.panel, self.panel_file, False
        if subs[a].snp_file != self.snp_file:
            subs[a].snps, subs[a].snp_file, subs[a]._snps_on_handle = self.snps, self.snp_file, False
            subs[a].gene_positions = self.gene_positions
        return subs[a]

    def specificity(self, num_haps):
        """Per chromosome (blocks [n, H, H], present flags [n]): sample independent, made once."""
        if getattr(self, '_spec', None) is None or self.num_haps != num_haps:
            spec = []
            for c in self.chroms:
                ids = self.gene_order[c]
                n = len(ids)
                present = np.fromiter((g in self.avecs for g in ids), dtype=np.uint8, count=n)
                blocks = np.zeros((n, num_haps, num_haps), dtype=np.float64)
                have = np.flatnonzero(present)
                if len(have):
                    blocks[have] = self.avecs.stack([ids[k] for k in have], (num_haps, num_haps))
                spec.append((blocks, present))
            self._spec, self.num_haps = spec, num_haps
            self.avecs.close()
        return self._spec

    def handle(self, num_haps):
        """(the device handle for `num_haps` founders, whether this call made it).  A new handle gets the transition
        tables and, with a grid file, the grid; the caller passes the specificity blocks with its first samples."""
        first_use = self.hmm is None or self.hmm.H != num_haps
        if first_use:
            tables = self.tables()
            self.close()
            self.hmm = DiplotypeHMM(num_haps, self.chroms, [len(self.gene_order[c]) for c in self.chroms], tables,
                                    device=self.device)
            if self.grid is not None:
                self.hmm.set_grid(self.gene_positions, {c: self.grid[c] for c in self.chroms if c in self.grid})
                self.grid_uploads += 1
                self.grid_slices = {c: (k, self.hmm.grid_offsets[k], self.hmm.grid_points[k])
                                    for k, c in enumerate(self.chroms) if c in self.grid}
        if self.panel is not None and not self._panel_on_handle:
            self.hmm.set_panel(self.panel[1])
            self._panel_on_handle = True
            self.__dict__.get('_panel_owner', self).panel_uploads += 1
        if self.snps is not None and not self._snps_on_handle:
            by = self.snps['by_chrom']
            self.hmm.set_snps(self.gene_positions, {c: self.snps['cM'][by[c]] for c in self.chroms},
                              {c: self.snps['mask'][by[c]] for c in self.chroms})
            self._snps_on_handle = True
            self.__dict__.get('_panel_owner', self).snp_uploads += 1
        return self.hmm, first_use

    def close(self):
        if self.hmm is not None:
            self.hmm.close()
            self.hmm = None
            self._panel_on_handle = False
            self._snps_on_handle = False
        for sub in self.__dict__.get('_alt_contexts', {}).values():
            sub.close()


def _expression_rows(ctx, expr_row, expr_table, num_haps):
    """A sample's TPM rows per chromosome of the context, in gene order.  KeyError: a gene without TPM."""
    rows = []
    for c in ctx.chroms:
        ids = ctx.gene_order[c]
        r = expr_table[[expr_row[g] for g in ids]] if len(ids) else np.zeros((0, num_haps))
        rows.append(np.ascontiguousarray(r, dtype=np.float64).reshape(len(ids), num_haps))
    return rows


def _collect(ctx, hmm, sample, diplotypes):
    """(posterior, ordered path names, calls) of one sample of the last run, by chromosome name / gene id."""
    posterior, path_names, calls = {}, {}, {}
    for k, c in enumerate(ctx.chroms):
        res = hmm.get(k, sample=sample)
        posterior[c] = res['gamma']
        path_names[c] = [diplotypes[s] for s in res['states']]
        calls.update((gid, diplotypes[s]) for gid, s in zip(ctx.gene_order[c], res['calls']) if s >= 0)
    return posterior, path_names, calls


def _save_reconstruction(stem, posterior, path_names, calls, threads=None):
    """The three files of `gbrs reconstruct` (gbrs_utils.py:600-609)."""
    out_calls, out_post, out_path = f'{stem}.genotypes.tsv', f'{stem}.genoprobs.npz', f'{stem}.genotypes.npz'
    logger.info(f'Saving Reconstructed Genotype Probabilities: {out_post}')
    savez_compressed(out_post, posterior, threads=threads)
    logger.info(f'Saving Reconstructed Genotypes: {out_calls}')
    with open(out_calls, 'w') as out:
        out.write('#Gene_ID\tDiplotype\n')
        out.writelines(f'{gid}\t{calls[gid]}\n' for gid in sorted(calls))
    logger.info(f'Saving Reconstructed Ordered Genotypes: {out_path}')
    savez_compressed(out_path, {c: np.asarray(v) for c, v in path_names.items()}, threads=threads)


def write_dosage_table(path, rows, haplotypes):
    """The text np.savetxt(path, rows, fmt='%.6f', delimiter='\\t', header='\\t'.join(haplotypes)) writes, which is
    `gbrs export`'s file (gbrs_utils.py:931), byte for byte: one format operation for the table instead of one per row
    (64,000 rows per sample, and a cohort's samples are written side by side)."""
    rows = np.asarray(rows, dtype=np.float64)
    line = '\t'.join(['%.6f'] * rows.shape[1]) + '\n'
    with open(path, 'w') as fh:
        fh.write('# ' + '\t'.join(haplotypes) + '\n')
        fh.write((line * rows.shape[0]) % tuple(rows.ravel().tolist()))


def _save_grid(stem, ctx, haplotypes, dosage, gamma_grid, threads=None):
    """A sample's grid files.  `<stem>.interpolated.genoprobs.npz` (only with gamma_grid): what `gbrs interpolate`
    saves - the grid's chromosomes that have gene positions and posteriors, in grid order.
    `<stem>.interpolated.genoprobs.tsv`: what `gbrs export -s <haplotypes>` writes from that file, rows in the grid
    file's order.  A grid chromosome without posteriors ends `export` with a KeyError; so it does here, after the
    .npz."""
    slices = ctx.grid_slices
    on_grid = [c for c in ctx.grid if c in slices]
    if gamma_grid is not None:
        out_npz = f'{stem}.interpolated.genoprobs.npz'
        logger.info(f'Saving interpolate probability file: {out_npz}')
        savez_compressed(out_npz, {c: gamma_grid[slices[c][0]] for c in on_grid}, threads=threads)
    for c in ctx.grid:
        if c not in slices:
            raise KeyError(f'{c} is not a file in the archive')
    rows = np.concatenate([dosage[slices[c][1]:slices[c][1] + slices[c][2]] for c in on_grid], axis=0) \
        if on_grid else np.zeros((0, len(haplotypes)))
    out_tsv = f'{stem}.interpolated.genoprobs.tsv'
    logger.info(f'Saving GBRS quant format: {out_tsv}')
    write_dosage_table(out_tsv, rows, haplotypes)


def change_table(num_haps):
    """uint8 (S x S): founder changes between two diplotypes read as multisets, 2 - |{a,b} n {c,d}| (AA -> AB is 1,
    AB -> CC is 2), states in combinations_with_replacement order."""
    a, b = np.array(list(combinations_with_replacement(range(num_haps), 2))).T
    first = a[:, None] == a[None, :]                  # states are sorted pairs: a <= b
    cross = a[:, None] == b[None, :]
    shared = np.where(first, 1 + (b[:, None] == b[None, :]),
                      np.where(cross, 1 + (b[:, None] == a[None, :]),
                               (b[:, None] == a[None, :]) | (b[:, None] == b[None, :])))
    return (2 - shared).astype(np.uint8)


def check_sim_geno_args(sim_geno, sim_geno_seed=0):
    """`--sim-geno K`: K >= 1, the seed a 64-bit unsigned number.  Refused before a file is read."""
    if sim_geno is None:
        return
    if isinstance(sim_geno, bool) or int(sim_geno) != sim_geno or sim_geno < 1:
        raise RuntimeError('--sim-geno must be at least 1')
    if not 0 <= int(sim_geno_seed) < 1 << 64:
        raise RuntimeError('--sim-geno-seed must be in 0 .. 2^64 - 1')


def viterbi_changes(calls, table):
    """Founder changes along a Viterbi path: the change table over consecutive genes that both have a call (>= 0)."""
    calls = np.asarray(calls, dtype=np.int64)
    both = (calls[:-1] >= 0) & (calls[1:] >= 0)
    return int(table[calls[:-1][both], calls[1:][both]].sum())


def _save_sim_geno(stem, ctx, diplotypes, drawn, seed, stream, threads=None):
    """A sample's two files of `--sim-geno`: `<stem>.sim_geno.npz` (per chromosome the (K x n_c) uint8 state indices of the
    draws, `diplotypes`, `seed`, `stream`) and `<stem>.sim_geno.crossovers.tsv` (per chromosome: genes, the founder changes
    of the Viterbi path, and mean, sd, min, max of the draws' founder changes).  drawn: per chromosome (K x n_c) paths,
    the (K x n_chrom) changes and the Viterbi path's count per chromosome (_draw_paths)."""
    paths, changes, viterbi = drawn
    out_npz, out_tsv = f'{stem}.sim_geno.npz', f'{stem}.sim_geno.crossovers.tsv'
    logger.info(f'Saving Simulated Genotypes: {out_npz}')
    arrays = {c: np.ascontiguousarray(paths[k]) for k, c in enumerate(ctx.chroms)}
    arrays.update(diplotypes=np.asarray(diplotypes), seed=np.uint64(seed), stream=np.uint32(stream))
    savez_compressed(out_npz, arrays, threads=threads)
    logger.info(f'Saving Crossover Counts: {out_tsv}')
    with open(out_tsv, 'w') as out:
        out.write('#Chromosome\tGenes\tViterbi\tMean\tSD\tMin\tMax\n')
        for k, c in enumerate(ctx.chroms):
            x = changes[:, k].astype(np.float64)
            sd = x.std(ddof=1) if len(x) > 1 else float('nan')
            out.write('%s\t%d\t%d\t%.6f\t%.6f\t%d\t%d\n' % (c, paths[k].shape[1], viterbi[k], x.mean(), sd,
                                                             int(x.min()), int(x.max())))


def _draw_paths(hmm, n_draws, seed, streams, sample=None):
    """Per sample of the call (paths per chromosome, changes, the Viterbi path's founder changes per chromosome)."""
    drawn = hmm.sample_paths(n_draws, seed=seed, sample=sample, streams=streams)
    if drawn['degenerate']:
        logger.warning(f"{drawn['degenerate']} draws met a step without a finite positive weight and took its most likely state")
    table = change_table(hmm.H)
    picked = [sample] if sample is not None else list(range(hmm.n_samples))
    out = []
    for j, s in enumerate(picked):
        viterbi = [viterbi_changes(hmm.get(k, sample=s, want=('calls',))['calls'], table) for k in range(len(hmm.chroms))]
        if sample is not None:
            out.append((drawn['paths'], drawn['changes'], viterbi))
        else:
            out.append(([p[j] for p in drawn['paths']], drawn['changes'][j], viterbi))
    return out


def check_diagnostics_args(diagnostics=False, error_lod_threshold=2.0, gene_report=None, cohort=False):
    """`--diagnostics [--error-lod-threshold T] [--gene-report PATH]`: T a finite number; the gene report needs the
    diagnostics and a cohort (`--sample-file`).  Refused before a file is read."""
    try:
        finite = bool(np.isfinite(float(error_lod_threshold)))
    except (TypeError, ValueError):
        finite = False
    if not finite:
        raise RuntimeError('--error-lod-threshold must be a finite number')
    if gene_report is not None and not (diagnostics and cohort):
        raise RuntimeError('--gene-report needs --diagnostics and --sample-file')


def expressed_genes(rows, expr_threshold):
    """bool per gene of a chromosome's TPM rows (n_c x H): the emission's own test - the founders' TPMs added left to
    right are not below the threshold.  A gene that fails it carries the prior as its emission."""
    rows = np.asarray(rows, dtype=np.float64)
    total = np.zeros(rows.shape[0])
    for x in range(rows.shape[1]):
        total = total + rows[:, x]
    return ~(total < expr_threshold)


def _diagnose(hmm, rows_of, expr_threshold, sample=None):
    """Per sample of the call what `--diagnostics` saves: per chromosome the five arrays of DiplotypeHMM.diagnostics and
    the expressed flags of the sample's TPM rows (rows_of[j]: sample j's rows per chromosome), and the Viterbi path's
    founder changes per chromosome."""
    got = hmm.diagnostics(sample=sample)
    table = change_table(hmm.H)
    picked = [sample] if sample is not None else list(range(hmm.n_samples))
    out = []
    for j, s in enumerate(picked):
        per = {k: [a if sample is not None else a[j] for a in got[k]] for k in got}
        per['expressed'] = [expressed_genes(r, expr_threshold) for r in rows_of[j]]
        per['viterbi'] = [viterbi_changes(hmm.get(k, sample=s, want=('calls',))['calls'], table)
                          for k in range(len(hmm.chroms))]
        out.append(per)
    return out


def _no_diagnostics():
    return dict({k: [] for k in DiplotypeHMM.DIAGNOSTICS}, expressed=[], viterbi=[])


def _save_diagnostics(stem, ctx, diplotypes, diag, threshold, threads=None):
    """A sample's two files of `--diagnostics`: `<stem>.diagnostics.npz` (per chromosome c `xo_<c>`, `pswitch_<c>`
    (n_c - 1), `errlod_<c>`, `maxprob_<c>`, `maxmarg_<c>`, `expressed_<c>` (n_c), and `diplotypes`) and
    `<stem>.diagnostics.tsv` (per chromosome and in total: genes, expressed genes, the founder changes of the Viterbi
    path, the expected founder changes, the expressed genes whose error LOD is above the threshold, the largest error LOD
    among the expressed genes and the mean posterior of the most likely diplotype; nan where there is nothing to take
    them over).  Unexpressed genes carry the prior as their emission: their error LOD is saved and counted nowhere."""
    out_npz, out_tsv = f'{stem}.diagnostics.npz', f'{stem}.diagnostics.tsv'
    logger.info(f'Saving Diagnostics: {out_npz}')
    arrays = {}
    for k, c in enumerate(ctx.chroms[:len(diag['errlod'])]):
        for name in DiplotypeHMM.DIAGNOSTICS + ('expressed',):
            arrays[f'{name}_{c}'] = np.ascontiguousarray(diag[name][k])
    arrays['diplotypes'] = np.asarray(diplotypes)
    savez_compressed(out_npz, arrays, threads=threads)
    logger.info(f'Saving Diagnostics Summary: {out_tsv}')

    def line(name, genes, expressed, viterbi, xo, errlod, maxprob):
        lods = errlod[expressed]
        return '%s\t%d\t%d\t%d\t%.6f\t%d\t%.6f\t%.6f\n' % (
            name, genes, int(expressed.sum()), viterbi, float(xo.sum()), int((lods > threshold).sum()),
            float(lods.max()) if len(lods) else float('nan'), float(maxprob.mean()) if genes else float('nan'))

    with open(out_tsv, 'w') as out:
        out.write('#Chromosome\tGenes\tExpressed\tViterbi\tExpectedCrossovers\tFlagged\tMaxErrorLOD\tMeanMaxProb\n')
        n_chrom = len(diag['errlod'])
        for k, c in enumerate(ctx.chroms[:n_chrom]):
            out.write(line(c, len(diag['errlod'][k]), diag['expressed'][k], diag['viterbi'][k], diag['xo'][k],
                           diag['errlod'][k], diag['maxprob'][k]))

        def whole(name, dtype=np.float64):                 # over the chromosomes; a sample without any: empty
            return np.concatenate([np.zeros(0, dtype=dtype)] + [np.asarray(a, dtype=dtype) for a in diag[name]])

        out.write(line('total', len(whole('errlod')), whole('expressed', bool), int(sum(diag['viterbi'])), whole('xo'),
                       whole('errlod'), whole('maxprob')))


class GeneReport:
    """`--gene-report`: per gene of the handle, over the samples of a cohort that ran, how many express it, in how many of
    those its error LOD is above the threshold, and the mean and the largest error LOD among them.  Added up on the host
    from the arrays every launch copies out."""

    def __init__(self, ctx, threshold):
        self.ids = [g for c in ctx.chroms for g in ctx.gene_order[c]]
        self.chrom_of = [c for c in ctx.chroms for _ in ctx.gene_order[c]]
        n = len(self.ids)
        self.threshold = threshold
        self.samples = 0
        self.expressed = np.zeros(n, dtype=np.int64)
        self.flagged = np.zeros(n, dtype=np.int64)
        self.total = np.zeros(n)
        self.largest = np.full(n, -np.inf)

    def add(self, diag):
        if not diag['errlod']:
            return
        lod = np.concatenate(diag['errlod'])
        on = np.concatenate(diag['expressed'])
        self.samples += 1
        self.expressed += on
        self.flagged += on & (lod > self.threshold)
        self.total += np.where(on, lod, 0.0)
        self.largest = np.where(on, np.maximum(self.largest, lod), self.largest)

    def write(self, path):
        logger.info(f'Saving Gene Report: {path}')
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = np.where(self.expressed > 0, self.total / self.expressed, np.nan)
        largest = np.where(self.expressed > 0, self.largest, np.nan)
        with open(path, 'w') as out:
            out.write('#Gene_ID\tChromosome\tSamples\tExpressed\tFlagged\tMeanErrorLOD\tMaxErrorLOD\n')
            for k, gid in enumerate(self.ids):
                out.write('%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\n' % (gid, self.chrom_of[k], self.samples, self.expressed[k],
                                                                self.flagged[k], mean[k], largest[k]))


def choose_tables(total):
    """(index of the first largest total, best minus second best) per sample from float64 (K, n) totals per candidate
    table file.  NaN never wins; all -inf (or NaN) selects candidate 0 with margin 0.0; K = 1 gives margin inf."""
    total = np.asarray(total, dtype=np.float64)
    if total.ndim != 2 or total.shape[0] < 1:
        raise ValueError('total must be (K, n) with K >= 1')
    K, n = total.shape
    key = np.where(np.isnan(total), -np.inf, total)
    best = key.argmax(axis=0)
    at = np.arange(n)
    top = key[best, at]
    if K == 1:
        return best, np.full(n, np.inf)
    rest = key.copy()
    rest[best, at] = -np.inf
    with np.errstate(invalid='ignore'):
        margin = top - rest.max(axis=0)
    return best, np.where(np.isnan(margin), 0.0, margin)


def check_loglik_args(loglik=False, alt_tprob_files=None, model_report=None, cohort=False, tprob_file=None):
    """`--loglik [--alt-tprob-file PATH ...] [--model-report PATH]`: the model report needs a cohort (`--sample-file`) and
    at least one alternative file; an alternative that is the `-t` file or another alternative (by realpath) is refused.
    Refused before a file is read."""
    alts = list(alt_tprob_files or ())
    if model_report is not None and not (cohort and alts):
        raise RuntimeError('--model-report needs --sample-file and at least one --alt-tprob-file')
    seen = {} if tprob_file is None else {os.path.realpath(tprob_file): '-t'}
    for f in alts:
        real = os.path.realpath(f)
        if real in seen:
            raise RuntimeError(f'--alt-tprob-file {f} is the same file as ' +
                               ('-t' if seen[real] == '-t' else f'--alt-tprob-file {seen[real]}'))
        seen[real] = f


def _model_logliks(ctx, hmm, num_haps):
    """float64 (K, n, n_chrom): the last run's data log-likelihood per candidate (`-t` first, then the alternatives as
    given), sample and chromosome.  The base's come from one reduction; an alternative's chromosome whose table equals the
    base's takes the base's value, the others take one forward-only launch per chromosome for all such alternatives."""
    alts = ctx.alt_tables(num_haps) if ctx.alt_tprob_files else []
    base = hmm.loglik()
    ctx.loglik_launches += 1
    per = np.repeat(base[None], 1 + len(alts), axis=0)
    for ci in range(len(ctx.chroms)):
        need = [a for a in range(len(alts)) if not ctx.alt_same[a][ci]]
        if need:
            per[[a + 1 for a in need], :, ci] = hmm.loglik_tables(ci, [alts[a][ci] for a in need])
            ctx.loglik_launches += 1
    return per


def loglik_totals(per):
    """The chromosomes' values added in handle order: (K, n, n_chrom) -> (K, n), or (K, n_chrom) -> (K,)."""
    per = np.asarray(per, dtype=np.float64)
    total = np.zeros(per.shape[:-1])
    for ci in range(per.shape[-1]):
        total = total + per[..., ci]
    return total


def write_loglik_table(path, chroms, n_genes, names, per, selected):
    """`<outbase>.loglik.tsv`: per chromosome its genes and one log-likelihood per candidate (`names`: the table files as
    given; per: (K, n_chrom)), a `total` line and `# selected: <name>`.  Numbers as repr(float)."""
    per = np.asarray(per, dtype=np.float64).reshape(len(names), len(chroms))
    logger.info(f'Saving Log-Likelihoods: {path}')
    with open(path, 'w') as out:
        out.write('chromosome\tgenes\t' + '\t'.join(names) + '\n')
        for ci, c in enumerate(chroms):
            out.write(f'{c}\t{int(n_genes[ci])}\t' + '\t'.join(repr(float(v)) for v in per[:, ci]) + '\n')
        out.write(f'total\t{int(sum(int(g) for g in n_genes))}\t' + '\t'.join(repr(float(v)) for v in loglik_totals(per)) + '\n')
        out.write(f'# selected: {names[selected]}\n')


def write_model_report(path, names, lines):
    """`--model-report`: per sample that ran its outbase, the selected table file, the margin of the choice (best minus
    second best total) and one total per candidate.  lines: (outbase, selected index, margin, totals)."""
    logger.info(f'Saving Model Report: {path}')
    with open(path, 'w') as out:
        out.write('#outbase\tselected\tmargin\t' + '\t'.join(names) + '\n')
        for outbase, selected, margin, totals in lines:
            out.write(f'{outbase}\t{names[selected]}\t{repr(float(margin))}\t' +
                      '\t'.join(repr(float(v)) for v in totals) + '\n')


# ---- matching the samples against a panel of reference genotypes (`--match-panel`) ------------------------

def check_match_args(match_panel=None, match_labels=None, match_expected=None, match_chromosomes=None, match_report=None,
                     match_matrix=None, grid_file=None, cohort=False):
    """`--match-panel FILE [--match-labels FILE | --match-expected ID] [--match-chromosomes LIST] [--match-report PATH]
    [--match-matrix PATH]`: every option needs the panel, the panel needs `--grid-file`; labels, report and matrix belong
    to a cohort (`--sample-file`), the expected id to a single sample (`-e`).  Refused before a file is read."""
    given = {'--match-labels': match_labels, '--match-expected': match_expected, '--match-chromosomes': match_chromosomes,
             '--match-report': match_report, '--match-matrix': match_matrix}
    if match_panel is None:
        for name, value in given.items():
            if value is not None:
                raise RuntimeError(f'{name} needs --match-panel')
        return
    if grid_file is None:
        raise RuntimeError('--match-panel needs --grid-file')
    if cohort and match_expected is not None:
        raise RuntimeError('--match-expected belongs to -e; with --sample-file use --match-labels')
    if not cohort:
        for name in ('--match-labels', '--match-report', '--match-matrix'):
            if given[name] is not None:
                raise RuntimeError(f'{name} needs --sample-file')


def _match_lines(path, what):
    """[(line number, first field, second field)] of a two-column tab separated file; blank and # lines skipped."""
    found = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith('#'):
                continue
            fields = line.split('\t')
            if len(fields) != 2:
                raise RuntimeError(f'{path}, line {number}: expected {what}')
            found.append((number, fields[0], fields[1]))
    return found


def read_match_labels(path):
    """{outbase: panel id} from lines `outbase<TAB>panel id` (`--match-labels`); an outbase given twice is refused."""
    labels, where = {}, {}
    for number, outbase, panel_id in _match_lines(path, 'outbase<TAB>panel id'):
        if outbase in labels:
            raise RuntimeError(f'{path}, line {number}: outbase {outbase} is already on line {where[outbase]}')
        labels[outbase], where[outbase] = panel_id, number
    return labels


def grid_layout(ctx):
    """{chromosome on the handle and on the grid: (handle index, first dosage row, rows)}: ctx.grid_slices, which the
    handle fills in when it gets the grid, worked out from the loaded files for use before there is a handle."""
    if ctx.grid_slices:
        return ctx.grid_slices
    slices, row = {}, 0
    for k, c in enumerate(ctx.chroms):
        if c in ctx.grid:
            slices[c] = (k, row, len(ctx.grid[c]))
            row += len(ctx.grid[c])
    return slices


def read_dosage_table(path, haplotypes, n_rows):
    """The (n_rows x H) numbers of a dosage table in `gbrs export` format (write_dosage_table) whose header names
    `haplotypes`.  RuntimeError naming the file for another header, row count or column count."""
    with open(path) as fh:
        header = fh.readline()
        body = fh.read()
    if header.rstrip('\n') != '# ' + '\t'.join(haplotypes):
        raise RuntimeError(f'{path}: the header {header.rstrip()!r} does not name the haplotypes {",".join(haplotypes)}')
    lines = body.splitlines()
    if len(lines) != n_rows:
        raise RuntimeError(f'{path}: {len(lines)} rows for the {n_rows} grid points of the grid file')
    width = len(haplotypes)
    for number, line in enumerate(lines, 2):
        if line.count('\t') != width - 1:
            raise RuntimeError(f'{path}, line {number}: {line.count(chr(9)) + 1} columns for {width} haplotypes')
    table = np.empty((n_rows, width), dtype=np.float64)
    if n_rows:
        # the library's parser takes `label TAB numbers`: every row gets an empty label
        raw = ('\t' + '\n\t'.join(lines) + '\n').encode()
        try:
            status = _lib.load().gbrs_parse_number_table(raw, len(raw), n_rows, width, _lib.ptr(table))
        except (ImportError, OSError):
            status = 1
        if status != 0:
            try:        # spellings the plain parser leaves to the caller (nan, inf): refused by the upload, not here
                table = np.array([[float(x) for x in line.split('\t')] for line in lines], dtype=np.float64)
            except ValueError as e:
                raise RuntimeError(f'{path}: {e}') from None
    return table


def read_match_panel(path, ctx, haplotypes):
    """(panel ids, one (M x H) dosage array per entry in handle order) from a panel file: tab separated lines
    `id<TAB>path`, blank and # lines skipped, ids unique; each path a dosage table in `gbrs export` format - what
    `--grid-file` writes - with one row per grid point of the context's grid file in that file's order, which is
    permuted here to the handle's (ctx.grid_slices).  KeyError: a grid chromosome that is not on the handle."""
    entries, where = [], {}
    for number, panel_id, table in _match_lines(path, 'id<TAB>path'):
        if panel_id in where:
            raise RuntimeError(f'{path}, line {number}: panel id {panel_id} is already on line {where[panel_id]}')
        where[panel_id] = number
        entries.append((panel_id, table))
    if not entries:
        raise RuntimeError(f'{path}: no panel entries')
    slices = grid_layout(ctx)
    for c in ctx.grid:
        if c not in slices:
            raise KeyError(f'{c} is not a file in the archive')
    first, row = {}, 0
    for c in ctx.grid:
        first[c] = row
        row += len(ctx.grid[c])
    order = [c for c in ctx.chroms if c in slices]
    arrays = []
    for panel_id, table in entries:
        if not os.path.isfile(table):
            raise RuntimeError(f"{path}: the dosage table '{table}' of panel id {panel_id} does not exist")
        rows = read_dosage_table(table, haplotypes, row)
        arrays.append(np.ascontiguousarray(np.concatenate([rows[first[c]:first[c] + slices[c][2]] for c in order], axis=0)
                                           if order else np.zeros((0, len(haplotypes)))))
    return [e[0] for e in entries], arrays


def match_chromosome_mask(chroms, points_per_chrom, names=None):
    """bool per handle chromosome: on the grid and, with `names` (a comma list or a sequence), named there.  An unknown
    name, or a selection without a grid point, is a RuntimeError."""
    points = np.asarray(points_per_chrom, dtype=np.int64)
    use = points > 0
    if names is not None:
        wanted = [x for x in (names.split(',') if isinstance(names, str) else list(names)) if x != '']
        for name in wanted:
            if name not in chroms:
                raise RuntimeError(f'--match-chromosomes: {name} is not a chromosome of the transition tables')
        use = use & np.array([c in wanted for c in chroms], dtype=bool)
    if int(points[use].sum()) == 0:
        raise RuntimeError('--match-panel: the selected chromosomes have no grid points')
    return use


def match_scores(cross, sample_norm, panel_norm, points_per_chrom, use):
    """(distance, similarity), each (..., n_panel), from the device's sums: cross (..., n_chrom, n_panel), sample_norm
    (..., n_chrom), panel_norm (n_panel, n_chrom).  The chromosomes of the mask `use` are added left to right in handle
    order into X, A, B and n grid points; distance = max(A + B - 2 X, 0) / n, the mean squared dosage difference per grid
    point, in [0, 2]; similarity = X / sqrt(A B), 0.0 where A B == 0.  RuntimeError when n == 0."""
    cross = np.asarray(cross, dtype=np.float64)
    sample_norm = np.asarray(sample_norm, dtype=np.float64)
    panel_norm = np.asarray(panel_norm, dtype=np.float64)
    X = np.zeros(cross.shape[:-2] + cross.shape[-1:])
    A = np.zeros(sample_norm.shape[:-1])
    B = np.zeros(panel_norm.shape[0])
    n = 0
    for c in range(cross.shape[-2]):
        if use[c]:
            X = X + cross[..., c, :]
            A = A + sample_norm[..., c]
            B = B + panel_norm[:, c]
            n += int(points_per_chrom[c])
    if n == 0:
        raise RuntimeError('no grid points on the chromosomes that are matched')
    A = A[..., None]
    distance = np.maximum(A + B - 2.0 * X, 0.0) / n
    product = A * B
    with np.errstate(invalid='ignore', divide='ignore'):
        similarity = np.where(product == 0.0, 0.0, X / np.sqrt(product))
    return distance, similarity


def rank_matches(panel_ids, distance, expected=None):
    """The panel entries by ascending distance, ties in panel order, for one sample.  Returns `order` (indices), `best`,
    `best_distance`, `second` ('' for a one-entry panel, its distance and the margin then nan), `margin` = second
    distance - best distance, `expected` ('' if none), `status` - `match` (the expected id is the best), `mismatch` (it is
    not), `unlabelled` (no expected id), `unknown-label` (it is not in the panel) - and `expected_distance` (nan) and
    `expected_rank` (1-based, 0) of an expected id that is in the panel.  No threshold decides anything."""
    distance = np.asarray(distance, dtype=np.float64)
    order = np.argsort(distance, kind='stable')
    best = int(order[0])
    out = {'order': order, 'best': panel_ids[best], 'best_distance': float(distance[best]), 'second': '',
           'second_distance': float('nan'), 'margin': float('nan'), 'expected': '' if expected is None else expected,
           'expected_distance': float('nan'), 'expected_rank': 0}
    if len(order) > 1:
        second = int(order[1])
        out.update(second=panel_ids[second], second_distance=float(distance[second]),
                   margin=float(distance[second]) - float(distance[best]))
    if expected is None:
        out['status'] = 'unlabelled'
    elif expected not in panel_ids:
        out['status'] = 'unknown-label'
    else:
        j = panel_ids.index(expected)
        out.update(status='match' if j == best else 'mismatch', expected_distance=float(distance[j]),
                   expected_rank=int(np.flatnonzero(order == j)[0]) + 1)
    return out


def write_match_table(path, panel_ids, distance, similarity, order):
    """`<outbase>.match.tsv`: one line per panel entry in rank order, numbers as repr(float)."""
    logger.info(f'Saving Panel Matches: {path}')
    with open(path, 'w') as out:
        out.write('#panel_id\tdistance\tsimilarity\n')
        out.writelines(f'{panel_ids[j]}\t{repr(float(distance[j]))}\t{repr(float(similarity[j]))}\n' for j in order)


def write_match_report(path, lines):
    """`--match-report`: one line per sample that ran.  lines: (outbase, rank_matches' dict)."""
    logger.info(f'Saving Match Report: {path}')
    with open(path, 'w') as out:
        out.write('#outbase\texpected\tstatus\tbest\tbest_distance\tsecond\tsecond_distance\tmargin\texpected_distance\t'
                  'expected_rank\n')
        for outbase, r in lines:
            out.write('\t'.join([outbase, r['expected'], r['status'], r['best'], repr(r['best_distance']), r['second'],
                                 repr(r['second_distance']), repr(r['margin']), repr(r['expected_distance']),
                                 str(r['expected_rank'])]) + '\n')


def write_match_matrix(path, outbases, panel_ids, chroms, points, distance, similarity, cross, sample_norm, panel_norm):
    """`--match-matrix`: an .npz with `distance` and `similarity` (N x M), the device's sums per chromosome - `cross`
    (N x n_chrom x M), `sample_norm` (N x n_chrom), `panel_norm` (M x n_chrom) - and `outbases`, `panel_ids`,
    `chromosomes`, `points` (grid points per chromosome)."""
    logger.info(f'Saving Match Matrix: {path}')
    with open(path, 'wb') as out:
        np.savez(out, distance=distance, similarity=similarity, cross=cross, sample_norm=sample_norm, panel_norm=panel_norm,
                 outbases=np.asarray(outbases), panel_ids=np.asarray(panel_ids), chromosomes=np.asarray(chroms),
                 points=np.asarray(points, dtype=np.int64))


def _load_panel(ctx, match_panel, haplotypes, match_chromosomes):
    """The panel of `--match-panel` onto the context (read once per context and panel file) and the chromosome mask and
    grid points per handle chromosome of the sums; every refusal comes from here, before a sample runs."""
    if ctx.panel is None or ctx.panel_file != match_panel:
        logger.info(f'Loading match panel: {match_panel}')
        ctx.panel = read_match_panel(match_panel, ctx, haplotypes)
        ctx.panel_file = match_panel
        ctx._panel_on_handle = False
    slices = grid_layout(ctx)
    points = [slices[c][2] if c in slices else 0 for c in ctx.chroms]
    return match_chromosome_mask(ctx.chroms, points, match_chromosomes), points


# ---- SNP dosages imputed from the founder haplotypes (`--snp-file`) ---------------------------------------

def check_snp_args(snp_file=None, snp_matrix=None, cohort=False):
    """`--snp-file FILE [--snp-matrix PATH]`: the matrix needs the SNP file and belongs to a cohort (`--sample-file`).
    Refused before a file is read."""
    if snp_matrix is None:
        return
    if snp_file is None:
        raise RuntimeError('--snp-matrix needs --snp-file')
    if not cohort:
        raise RuntimeError('--snp-matrix needs --sample-file')


def _grid_bp_cm(grid_file):
    """{chromosome: (bp ascending, cM in that order)} of a grid file, for filling SNP positions."""
    rows = {}
    with open(grid_file) as fh:
        fh.readline()
        for line in fh:
            fields = line.rstrip('\n').split('\t')
            if len(fields) > 3:
                rows.setdefault(fields[1], []).append((float(fields[2]), float(fields[3])))
    table = {}
    for c, pairs in rows.items():
        a = np.asarray(pairs, dtype=np.float64)
        order = np.argsort(a[:, 0], kind='stable')
        table[c] = (a[order, 0], a[order, 1])
    return table


def read_snp_file(path, haplotypes, chroms, grid_file=None):
    """The SNPs of `--snp-file`: one header line, then tab separated `id, chr, bp, cM, pattern` - the grid file's four
    columns and one character per haplotype of `haplotypes`, `1` where that founder carries the alternative allele, else
    `0`.  A cM of `NA` or empty is filled from bp by np.interp over that chromosome's rows of `grid_file` sorted by bp
    (clamped at the ends); without a grid file, or when the grid file lacks the chromosome, the line is refused.  Every
    other line - too few columns, a pattern of another length or with another character, a position that is no number -
    is a ValueError naming the line number and the reason.
    Returns a dict: `snp_id`, `chrom`, `bp`, `cM`, `pattern` (arrays in file order, bp nan where it is NA), `mask`
    (uint32, bit h: haplotype h), `by_chrom` {c: file rows of chromosome c, file order} for the chromosomes of `chroms`,
    `order` (those rows, chromosomes in the order of `chroms`: the handle's SNP order) and `foreign`, the number of
    SNPs on other chromosomes, which one log warning counts."""
    H = len(haplotypes)
    ids, chrom, bp, cm, patterns, fill = [], [], [], [], [], []
    with open(path) as fh:
        fh.readline()
        for number, line in enumerate(fh, 2):
            line = line.rstrip('\r\n')
            if not line:
                continue
            fields = line.split('\t')
            if len(fields) < 5:
                raise ValueError(f'{path}, line {number}: {len(fields)} columns, expected id, chr, bp, cM, pattern')
            pattern = fields[4]
            if len(pattern) != H:
                raise ValueError(f'{path}, line {number}: the pattern {pattern!r} has {len(pattern)} characters for '
                                 f'{H} haplotypes')
            if pattern.strip('01'):
                raise ValueError(f'{path}, line {number}: the pattern {pattern!r} holds a character other than 0 and 1')
            try:
                where = float('nan') if fields[2] in ('NA', '') else float(fields[2])
                x = None if fields[3] in ('NA', '') else float(fields[3])
            except ValueError:
                raise ValueError(f'{path}, line {number}: the position {fields[2]!r} / {fields[3]!r} is not a number') from None
            if x is None:
                if grid_file is None:
                    raise ValueError(f'{path}, line {number}: no cM position; filling it from bp needs --grid-file')
                if where != where:
                    raise ValueError(f'{path}, line {number}: neither a cM nor a bp position')
                fill.append((len(ids), number))
                x = float('nan')
            ids.append(fields[0])
            chrom.append(fields[1])
            bp.append(where)
            cm.append(x)
            patterns.append(pattern)
    chrom = np.asarray(chrom, dtype=str)
    bp, cm = np.asarray(bp, dtype=np.float64), np.asarray(cm, dtype=np.float64)
    if fill:
        table = _grid_bp_cm(grid_file)
        for row, number in fill:
            if chrom[row] not in table:
                raise ValueError(f'{path}, line {number}: no cM position, and {grid_file} has no rows for chromosome '
                                 f'{chrom[row]} to fill it from')
        rows = np.asarray([row for row, _ in fill])
        for c in dict.fromkeys(chrom[rows].tolist()):
            sel = rows[chrom[rows] == c]
            cm[sel] = np.interp(bp[sel], *table[c])
    mask = np.zeros(len(ids), dtype=np.uint32)
    if ids:
        bits = (np.frombuffer(''.join(patterns).encode(), dtype=np.uint8).reshape(len(ids), H) == ord('1'))
        mask = (bits.astype(np.uint32) << np.arange(H, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    by_chrom = {c: np.flatnonzero(chrom == c) for c in chroms}
    order = np.concatenate([by_chrom[c] for c in chroms]) if len(chroms) else np.zeros(0, dtype=np.int64)
    foreign = len(ids) - len(order)
    if foreign:
        logger.warning(f'{path}: {foreign} SNPs on chromosomes without a transition table get nan')
    return {'snp_id': np.asarray(ids, dtype=str), 'chrom': chrom, 'bp': bp, 'cM': cm, 'pattern': np.asarray(patterns, dtype=str),
            'mask': mask, 'by_chrom': by_chrom, 'order': order.astype(np.int64), 'foreign': foreign}


def snp_dosage_in_file_order(snps, imputed):
    """impute()'s columns (handle order) as (..., M) in the SNP file's order, nan for the SNPs of foreign chromosomes."""
    imputed = np.asarray(imputed, dtype=np.float64)
    out = np.full(imputed.shape[:-1] + (len(snps['snp_id']),), np.nan)
    out[..., snps['order']] = imputed
    return out


def write_snp_dosage(path, dosage, snps):
    """`<outbase>.snp_dosage.npz`: `dosage` float64[M], the expected alternative allele counts in SNP file order, and
    `snp_id`."""
    logger.info(f'Saving SNP Dosages: {path}')
    with open(path, 'wb') as out:
        np.savez(out, dosage=np.asarray(dosage, dtype=np.float64), snp_id=snps['snp_id'])


def write_snp_matrix(path, outbases, dosage, snps):
    """`--snp-matrix`: an .npz with `dosage` (samples x M) of the samples that ran, `outbases`, and the SNP file's
    columns `snp_id`, `chrom`, `bp`, `cM` (as used, filled ones included), `pattern`."""
    logger.info(f'Saving SNP Matrix: {path}')
    with open(path, 'wb') as out:
        np.savez(out, dosage=np.asarray(dosage, dtype=np.float64), outbases=np.asarray(outbases, dtype=str),
                 snp_id=snps['snp_id'], chrom=snps['chrom'], bp=snps['bp'], cM=snps['cM'], pattern=snps['pattern'])


def _load_snps(ctx, snp_file, haplotypes):
    """The SNPs of `--snp-file` onto the context (read once per context and file); every refusal of the file comes from
    here, before a sample runs."""
    if ctx.snps is None or ctx.snp_file != snp_file:
        logger.info(f'Loading SNP file: {snp_file}')
        ctx.snps = read_snp_file(snp_file, haplotypes, ctx.chroms, ctx.grid_file)
        ctx.snp_file = snp_file
        ctx._snps_on_handle = False
        if getattr(ctx, 'gene_positions', None) is None:
            ctx.gene_positions = read_gene_positions(ctx.gpos_file)
    return ctx.snps


# ---- the two drivers: one sample (`-e`) and a cohort (`--sample-file`) ---------------------------------------------------

@dataclasses.dataclass(frozen=True)
class ReconstructOptions:
    """The keywords of reconstruct (one sample) and reconstruct_many (a cohort) after `device`, apart from `stage_times`,
    `context` and `grid_file`.  All but `expr_threshold` and `sigma`, the emission model's as in gbrs_utils.reconstruct,
    are extensions; one that is off makes no device pass, no buffer and no file.
    `grid_genoprobs` (with a grid file): beside `<outbase>.interpolated.genoprobs.tsv`, the founder dosages `gbrs export`
    would write after `gbrs interpolate`, `<outbase>.interpolated.genoprobs.npz` holds what `gbrs interpolate` writes.
    `sim_geno` = K: K diplotype paths per chromosome drawn from the joint posterior on the device with
    seed `sim_geno_seed` go to `<outbase>.sim_geno.npz`, their founder changes beside the Viterbi path's to
    `<outbase>.sim_geno.crossovers.tsv`.  The one sample draws on stream 0, a cohort's sample on its 0-based position in
    `expression_files`, so its draws do not depend on the launch it ran in.
    `diagnostics`: the expected founder changes and the switch probability of every gene interval, and per
    gene the error LOD and the most likely diplotype, go to `<outbase>.diagnostics.npz`, a summary per chromosome with the
    expressed genes whose error LOD is above `error_lod_threshold` to `<outbase>.diagnostics.tsv`.  `gene_report` (cohort
    only): one line per gene of the handle over the samples that ran - how many express it, in how many of those its
    error LOD is above the threshold.
    `loglik`: `<outbase>.loglik.tsv` holds the data log-likelihood of the run per chromosome and in total.
    `alt_tprob_files` (implies `loglik`; with a context, the context's): the emissions are also scored under these table
    files on the device.  A sample that one of them explains better than `tprob_file` (the first largest total,
    `tprob_file` first) is run again, alone, under a handle on that file (made at first need, kept with the context), and
    all of its files are the ones a plain single-sample call with that file writes; a cohort's sample keeps its stream.
    `model_report` (cohort only): one line per sample that ran - outbase, selected file, margin, totals per candidate.
    `match_panel` (needs a grid file): the grid dosages are compared on the device with those of every entry
    of the panel file and `<outbase>.match.tsv` lists the entries by distance; a sample that moved to another table file
    is matched under that handle.  `match_chromosomes`: the chromosomes that are compared.  `match_expected` (one sample
    only): the panel id the sample should be, logged with its status.  Cohort only: `match_labels`, a file of lines
    `outbase<TAB>panel id` saying the same per sample; `match_report`, one line per sample that ran with its status, best
    and second entry and margin; `match_matrix`, an .npz with the distances, similarities and the device's sums.
    `snp_file`: the expected number of alternative alleles at every SNP of the file, from the founder
    dosages at the genes around it and the SNP's founder allele pattern, on the device; `<outbase>.snp_dosage.npz` holds
    them in the file's order.  The SNPs go to a handle once.  `snp_matrix` (cohort only): an .npz with the rows of all
    samples that ran and the SNP file's columns.
    `scan_pheno` (cohort only; needs a grid file): a table of phenotypes keyed by outbase.  The grid dosages
    of every sample that ran and has a phenotype row (and, with `scan_covar`, a covariate row) are collected on the device
    in the order of `expression_files`; after the last launch the phenotypes are regressed on them at every grid point
    and `<scan_out>.scan.npz` and `<scan_out>.scan.peaks.tsv` are written (gbrs_amd/scan.py, which documents `scan_rankz`,
    `scan_min_lod` and `scan_lod_matrix`).  `scan_perms`: that many permutations follow the scan on the
    device and both files gain genome-wide thresholds and p-values; the other `scan_perm_*` are scan.perm_options'.
    `scan_snps` (needs `snp_file`, `scan_pheno` and a grid file): every SNP of the file is then tested with one
    degree of freedom on the prepared cohort, and `<scan_out>.scan.snps.npz` and `<scan_out>.scan.snps.peaks.tsv` are written.
    `scan_mediate`: the scan's peaks are mediated by the phenotypes, or by the table of `scan_mediator_file`,
    and `<scan_out>.scan.mediation.npz` and `<scan_out>.scan.mediation.tsv` are written; `scan_mediate_min_lod` and
    `scan_mediate_top` are scan.mediate_options'.
    `scan_effects`, `scan_lod_drop`: the founder effects of the scan's peaks of at least
    `scan_effects_min_lod` go to `<scan_out>.scan.effects.npz` and `<scan_out>.scan.effects.tsv`, named by the samples'
    haplotype header; the peaks' LOD support intervals join the scan's two files (scan.effects_options).
    `scan_kinship`, `scan_kinship_out`: the scan is the linear mixed model's with the cohort's own
    leave-one-chromosome-out or overall kinship (scan.kinship_options); the other scan passes are then refused.
    `scan_kinship_snps` (needs `scan_kinship`): a SNP file in `snp_file`'s format whose SNPs are tested
    with one degree of freedom under the same mixed model after the scan, at the heritabilities it fitted.
    `scan_kinship_effects`, `scan_kinship_effects_min_lod`, `scan_kinship_lod_drop` (need `scan_kinship`):
    `scan_effects`' files and `scan_lod_drop`'s columns under the mixed model (scan.kinship_effects_options).
    `scan_intcovar` (needs `scan_covar`, not with `scan_kinship`): columns of the covariate table, comma
    separated, that also interact with the QTL; their scan follows the others and writes its own two files."""
    expr_threshold: float = 1.5
    sigma: float = 0.12
    grid_genoprobs: bool = False
    sim_geno: int = None
    sim_geno_seed: int = 0
    diagnostics: bool = False
    error_lod_threshold: float = 2.0
    gene_report: str = None
    loglik: bool = False
    alt_tprob_files: list = None
    model_report: str = None
    match_panel: str = None
    match_expected: str = None
    match_chromosomes: object = None
    match_labels: str = None
    match_report: str = None
    match_matrix: str = None
    snp_file: str = None
    snp_matrix: str = None
    scan_pheno: str = None
    scan_covar: str = None
    scan_rankz: bool = False
    scan_out: str = None
    scan_min_lod: float = None
    scan_lod_matrix: bool = False
    scan_perms: int = None
    scan_perm_seed: int = None
    scan_perm_alpha: object = None
    scan_perm_chromosomes: object = None
    scan_perm_pheno: str = None
    scan_snps: bool = False
    scan_mediate: bool = False
    scan_mediate_min_lod: float = None
    scan_mediate_top: int = None
    scan_mediator_file: str = None
    scan_effects: bool = False
    scan_effects_min_lod: float = None
    scan_lod_drop: float = None
    scan_kinship: str = None
    scan_kinship_out: bool = False
    scan_kinship_snps: str = None
    scan_kinship_effects: bool = False
    scan_kinship_effects_min_lod: float = None
    scan_kinship_lod_drop: float = None
    scan_intcovar: str = None

    @classmethod
    def of(cls, keywords):
        """The options among `keywords` (a driver's locals(), a parser's vars(args)), the others at their defaults; a
        context's alternative table files stand in for none given, and alternatives turn `loglik` on."""
        options = cls(**{f.name: keywords[f.name] for f in dataclasses.fields(cls) if f.name in keywords})
        alts, context = options.alt_tprob_files, keywords.get('context')
        if alts is None and context is not None:
            alts = context.alt_tprob_files
        return dataclasses.replace(options, alt_tprob_files=alts, loglik=bool(options.loglik or alts))

    def keywords(self, cohort):
        """The options as keywords of reconstruct_many (cohort) or of reconstruct, which has no `scan_*`."""
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if cohort or not f.name.startswith('scan_')}

    def check(self, cohort, grid_file, tprob_file):
        """Every refusal that needs no file, in the command's order.  cohort: `--sample-file`, not `-e`."""
        from .scan import check_scan_args, check_scan_snp_args
        check_sim_geno_args(self.sim_geno, self.sim_geno_seed)
        check_diagnostics_args(self.diagnostics, self.error_lod_threshold, self.gene_report, cohort=cohort)
        check_loglik_args(self.loglik, self.alt_tprob_files, self.model_report, cohort=cohort, tprob_file=tprob_file)
        check_match_args(self.match_panel, self.match_labels, self.match_expected, self.match_chromosomes, self.match_report,
                         self.match_matrix, grid_file, cohort=cohort)
        check_snp_args(self.snp_file, self.snp_matrix, cohort=cohort)
        check_scan_args(self.scan_pheno, self.scan_covar, self.scan_rankz, self.scan_out, self.scan_min_lod,
                        self.scan_lod_matrix, grid_file, cohort=cohort, scan_perms=self.scan_perms,
                        scan_perm_seed=self.scan_perm_seed, scan_perm_alpha=self.scan_perm_alpha,
                        scan_perm_chromosomes=self.scan_perm_chromosomes, scan_perm_pheno=self.scan_perm_pheno,
                        scan_mediate=self.scan_mediate, scan_mediate_min_lod=self.scan_mediate_min_lod,
                        scan_mediate_top=self.scan_mediate_top, scan_mediator_file=self.scan_mediator_file,
                        scan_effects=self.scan_effects, scan_effects_min_lod=self.scan_effects_min_lod,
                        scan_lod_drop=self.scan_lod_drop, scan_kinship=self.scan_kinship,
                        scan_kinship_out=self.scan_kinship_out, scan_snps=self.scan_snps,
                        scan_kinship_snps=self.scan_kinship_snps, scan_kinship_effects=self.scan_kinship_effects,
                        scan_kinship_effects_min_lod=self.scan_kinship_effects_min_lod,
                        scan_kinship_lod_drop=self.scan_kinship_lod_drop, scan_intcovar=self.scan_intcovar)
        check_scan_snp_args(self.scan_snps, self.snp_file, self.scan_pheno, grid_file, cohort=cohort)


class _Shared:
    """What the launches of one driver call share: the options, the names of the samples' header, what the options had
    read once (panel, SNPs; every refusal of those files comes from here, before a sample runs) and what outlives a
    launch, keyed by the sample's position in `expression_files` (0 for the single-sample command)."""

    def __init__(self, ctx, options, haplotypes, tprob_file, marks, say, handle_key, expected):
        self.ctx, self.options, self.marks = ctx, options, marks
        self.say = say                     # logs a line of the single-sample command; a cohort stays quiet
        self.handle_key = handle_key       # the stage_times key a new handle's seconds go to
        self.haplotypes, self.num_haps = haplotypes, len(haplotypes)
        self.diplotypes = [a + b for a, b in combinations_with_replacement(haplotypes, 2)]
        self.names = [tprob_file] + list(ctx.alt_tprob_files) if options.loglik else None    # the candidates
        self.expected = expected           # sample -> the panel id it should be
        if options.match_panel is not None:
            self.match_use, self.match_points = _load_panel(ctx, options.match_panel, haplotypes, options.match_chromosomes)
        self.snps = _load_snps(ctx, options.snp_file, haplotypes) if options.snp_file is not None else None
        self.choices = {}                  # sample -> (selected candidate, margin, totals per candidate)
        self.scores = {}                   # sample -> its (candidates, chromosomes) log-likelihoods
        self.matches = {}                  # sample -> (cross, sample_norm, distance, similarity, rank_matches' dict)
        self.panel_norm = None
        self.snp_rows = {}                 # sample -> its dosages in SNP file order
        self.scan_keep = set()             # the samples the genome scan takes
        self.scan_held = {}                # sample -> its host dosage rows, until its batch is appended to the scan
        self.report = None                 # the GeneReport, made with the first launch that feeds it

    def spend(self, key, seconds):
        self.marks[key] = self.marks.get(key, 0.0) + seconds


def _pass_grid(job):
    genoprobs = job.options.grid_genoprobs
    got = job.hmm.grid(sample=job.sample, want=('dosage', 'gamma_grid') if genoprobs else ('dosage',))
    if job.sample is not None:
        got = {k: [v] for k, v in got.items()}
    per = [(got['dosage'][s], got['gamma_grid'][s] if genoprobs else None) for s in range(len(job.members))]
    for s in job.stay:
        if job.members[s] in job.shared.scan_keep:
            job.shared.scan_held[job.members[s]] = per[s][0]
    return per


def _pass_match(job):
    shared = job.shared
    got = job.hmm.match(sample=job.sample)
    shared.panel_norm = job.hmm.match_info()['panel_norm']
    cross, norm = (got['cross'], got['sample_norm']) if job.sample is None else (got['cross'][None], got['sample_norm'][None])
    distance, similarity = match_scores(cross, norm, shared.panel_norm, shared.match_points, shared.match_use)
    per = {}
    for s in job.stay:
        k = job.members[s]
        per[s] = shared.matches[k] = (cross[s], norm[s], distance[s], similarity[s],
                                      rank_matches(shared.ctx.panel[0], distance[s], shared.expected.get(k)))
    return per


def _pass_snp(job):
    snps = job.shared.snps
    got = np.atleast_2d(job.hmm.impute(sample=job.sample)) if len(snps['order']) else np.zeros((len(job.members), 0))
    rows = snp_dosage_in_file_order(snps, got)
    for s in job.stay:
        job.shared.snp_rows[job.members[s]] = rows[s]
    return rows


def _pass_sim_geno(job):               # a sample's stream is its position in `expression_files`
    return _draw_paths(job.hmm, job.options.sim_geno, job.options.sim_geno_seed, job.members, sample=job.sample)


def _pass_diagnostics(job):
    shared, options = job.shared, job.options
    got = _diagnose(job.hmm, job.rows, options.expr_threshold, sample=job.sample)
    if options.gene_report is not None:
        if shared.report is None:
            shared.report = GeneReport(shared.ctx, options.error_lod_threshold)
        for s in job.stay:
            shared.report.add(got[s])
    return got


# The optional device passes that follow run(), the likelihoods and the collection of the posteriors, in the order both
# drivers make them.  Each reads what gbrs_hmm_run left and buffers of its own (match: the dosages of the grid pass before
# it), so the order changes no bit.  Per pass: its stage_times key, which is also its key in a sample's bundle; what turns
# it on; the function above that makes it, through DiplotypeHMM.grid / .match and .match_info / .impute / .sample_paths
# (_draw_paths) / .diagnostics (_diagnose); the line the single-sample command logs before it.
_PASSES = (
    ('grid', lambda job: job.on.grid is not None, _pass_grid, 'Converting genotype probability on the grid'),
    ('match', lambda job: job.options.match_panel is not None, _pass_match, 'Matching the sample against the panel'),
    ('snp', lambda job: job.shared.snps is not None, _pass_snp, 'Imputing SNP dosages'),
    ('sim_geno', lambda job: job.options.sim_geno is not None, _pass_sim_geno, 'Drawing {0.sim_geno} paths from the posterior'),
    ('diagnostics', lambda job: job.options.diagnostics, _pass_diagnostics, 'Getting crossover expectations and gene error LODs'),
)


def _launch(on, members, rows, shared, sample=None):
    """The samples `members` (their TPM rows per chromosome in `rows`) through the handle of context `on` - the shared
    context or one of its alternatives - in one launch, then the passes the options ask for.  sample: None asks the handle
    for every sample of the launch (a cohort), 0 for the one sample of the single-sample command.
    Returns ({sample: its bundle - what _save_sample writes}, {alternative: [samples]}): with candidates to weigh (`on` is
    the shared context) the samples that an alternative explains better get no bundle; the caller runs them under it."""
    options, say, clock = shared.options, shared.say, time.perf_counter
    t0 = clock()
    hmm, first_use = on.handle(shared.num_haps)
    spec = on.specificity(shared.num_haps) if first_use else None      # stays on a handle once given
    shared.spend(shared.handle_key, clock() - t0)
    t0 = clock()
    say('Getting forward probability')
    stacked = [np.stack([r[ci] for r in rows]) for ci in range(len(on.chroms))]
    if first_use:
        hmm.set_expression(stacked, [x[0] for x in spec], [x[1] for x in spec], options.expr_threshold, options.sigma)
    else:
        hmm.set_expression(stacked, expr_threshold=options.expr_threshold, sigma=options.sigma)
    say('Getting backward probability')
    hmm.run()
    shared.spend('hmm', clock() - t0)
    moved, stay = {}, list(range(len(members)))
    if options.loglik and on is shared.ctx:
        t0 = clock()
        say('Getting the log-likelihood of the data')
        per = _model_logliks(on, hmm, shared.num_haps)
        totals = loglik_totals(per)
        best, margin = choose_tables(totals)
        for s, k in enumerate(members):
            shared.choices[k] = (int(best[s]), float(margin[s]), totals[:, s].copy())
            shared.scores[k] = per[:, s, :].copy()
            if best[s] != 0:
                moved.setdefault(int(best[s]) - 1, []).append(k)
        stay = [s for s in stay if best[s] == 0]
        shared.spend('loglik', clock() - t0)
    t0 = clock()
    if stay:
        say('Getting forward-backward probability')
    bundles = {s: {'reconstruction': _collect(on, hmm, s, shared.diplotypes), 'stream': members[s],
                   'scores': shared.scores.get(members[s])} for s in stay}
    shared.spend('hmm', clock() - t0)
    job = types.SimpleNamespace(on=on, hmm=hmm, members=members, rows=rows, stay=stay, sample=sample, shared=shared,
                                options=options)
    for key, enabled, make, line in _PASSES:
        if stay and enabled(job):
            t0 = clock()
            say(line.format(options))
            got = make(job)
            for s in stay:
                bundles[s][key] = got[s]
            shared.spend(key, clock() - t0)
    return {members[s]: bundle for s, bundle in bundles.items()}, moved


def _nothing_ran(on, shared, k):
    """The bundle of sample `k` when no chromosome has a transition table: every file the options ask for, empty."""
    options = shared.options
    bundle = {'reconstruction': ({}, {}, {}), 'stream': k}
    if on.grid is not None:
        bundle['grid'] = (np.zeros((0, shared.num_haps)), [] if options.grid_genoprobs else None)
    if options.sim_geno is not None:
        bundle['sim_geno'] = ([], np.zeros((options.sim_geno, 0), dtype=np.int32), [])
    if options.diagnostics:
        bundle['diagnostics'] = _no_diagnostics()
    if options.loglik:
        K = len(shared.names)
        shared.choices[k] = (0, 0.0 if K > 1 else np.inf, np.zeros(K))
        bundle['scores'] = shared.scores[k] = np.zeros((K, 0))
    if shared.snps is not None:
        bundle['snp'] = shared.snp_rows[k] = np.full(len(shared.snps['snp_id']), np.nan)
    return bundle


def _save_loglik(stem, on, shared, k):
    write_loglik_table(f'{stem}.loglik.tsv', on.chroms, [len(on.gene_order[c]) for c in on.chroms], shared.names,
                       shared.scores[k], shared.choices[k][0])


def _save_sample(stem, on, bundle, shared, threads=None):
    """The files of one sample that ran under context `on`, from its bundle.  threads: of the .npz writers; None lets
    them use every core (the single-sample command), a cohort's writer pool gives each sample one."""
    options = shared.options
    _save_reconstruction(stem, *bundle['reconstruction'], threads=threads)
    if 'grid' in bundle:
        _save_grid(stem, on, shared.haplotypes, *bundle['grid'], threads=threads)
    if 'sim_geno' in bundle:
        _save_sim_geno(stem, on, shared.diplotypes, bundle['sim_geno'], options.sim_geno_seed, bundle['stream'], threads=threads)
    if 'diagnostics' in bundle:
        _save_diagnostics(stem, on, shared.diplotypes, bundle['diagnostics'], options.error_lod_threshold, threads=threads)
    if bundle.get('scores') is not None:
        _save_loglik(stem, on, shared, bundle['stream'])
    if 'match' in bundle:
        _, _, distance, similarity, rank = bundle['match']
        write_match_table(f'{stem}.match.tsv', shared.ctx.panel[0], distance, similarity, rank['order'])
        shared.say(f"Panel match: {rank['status']}, best {rank['best']} at {rank['best_distance']!r}")
    if 'snp' in bundle:
        write_snp_dosage(f'{stem}.snp_dosage.npz', bundle['snp'], shared.snps)


def reconstruct(expression_file: str, tprob_file: str, avec_file: str = None, gpos_file: str = None,
                expr_threshold: float = 1.5, sigma: float = 0.12, outbase: str = None,
                device: int = 0, stage_times: dict = None, context: ReconstructContext = None,
                grid_file: str = None, grid_genoprobs: bool = False, sim_geno: int = None,
                sim_geno_seed: int = 0, diagnostics: bool = False, error_lod_threshold: float = 2.0,
                gene_report: str = None, loglik: bool = False, alt_tprob_files=None, model_report: str = None,
                match_panel: str = None, match_expected: str = None, match_chromosomes=None, match_labels: str = None,
                match_report: str = None, match_matrix: str = None, snp_file: str = None, snp_matrix: str = None) -> None:
    """`gbrs reconstruct`: diplotype posteriors and Viterbi calls along every chromosome from
    gene-level TPMs.  Same inputs, defaults and three output files as gbrs_utils.reconstruct
    (gbrs_utils.py:382-609); the emission model and the three recursions run on the device.
    `stage_times` (optional dict) receives wall-clock seconds per stage.  `context` (extension,
    gbrs_amd.worker): the sample-independent inputs and the device handle of an earlier call on the same
    tables - the transition and specificity tables then stay where they are and the sample moves its expression
    rows only.  `grid_file` (extension; with a context, the context's): the posteriors also go onto the marker grid
    on the device.  Every keyword from `grid_genoprobs` on is described on ReconstructOptions
    (DESIGN.md §22-§26); those it marks as cohort only are refused here."""
    options = ReconstructOptions.of(locals())
    options.check(False, grid_file if context is None else context.grid_file, tprob_file)
    clock = time.perf_counter
    marks = stage_times if stage_times is not None else {}
    stem = 'gbrs.reconstructed' if outbase is None else outbase
    ctx = context if context is not None else ReconstructContext(tprob_file, avec_file, gpos_file, device, grid_file,
                                                                 options.alt_tprob_files)
    for label, value in (('Expression File', expression_file), ('Transition Probabilities File', tprob_file),
                         ('Alignment Specificity File', ctx.avec_file), ('Gene Position File', ctx.gpos_file),
                         ('Expression Threshold', expr_threshold), ('Sigma', sigma), ('Outbase', outbase)):
        logger.info(f'{label}: {value}')
    if ctx.grid_file is not None:
        logger.info(f'Grid File: {ctx.grid_file}')

    _lib.warm_up_device_async(device)      # HIP start-up overlaps with reading the files
    t0 = clock()
    # the transition tables are the big read (0.4 GB of deflate streams at DO size): it starts on the library's
    # threads and is collected when the tables are needed, after the small files have been parsed
    ctx.load()
    logger.info(f'Loading expression level data: {expression_file}')
    haplotypes, expr_row, expr_table = read_gene_tpm(expression_file)
    rows = _expression_rows(ctx, expr_row, expr_table, len(haplotypes))
    ctx.specificity(len(haplotypes))       # what a new handle takes is read here, not while it is made
    ctx.tables()
    if options.loglik and ctx.alt_tprob_files:
        ctx.alt_tables(len(haplotypes))    # a file that does not fit is refused before the sample runs
    spent = {}                             # the launch's seconds: they replace, not add to, an earlier call's
    shared = _Shared(ctx, options, haplotypes, tprob_file, spent, logger.info, 'tables_to_device',
                     {} if match_expected is None else {0: match_expected})
    marks['load'] = clock() - t0

    moved = {}
    try:
        if ctx.chroms:
            bundles, moved = _launch(ctx, [0], [rows], shared, sample=0)
            marks.update(spent)
        else:
            bundles = {0: _nothing_ran(ctx, shared, 0)}
        for a in moved:
            # the sample goes through a handle on the better-fitting file: what a plain call with that file does
            logger.info(f'Selected {shared.names[a + 1]}: running the sample under it')
            reconstruct(expression_file, shared.names[a + 1], outbase=outbase, device=device, stage_times=marks,
                        context=ctx.alt_context(a),
                        **dataclasses.replace(options, loglik=False, alt_tprob_files=None).keywords(cohort=False))
    finally:
        if context is None:
            ctx.close()                    # the device is free before the seconds spent writing files
    if moved:
        _save_loglik(stem, ctx, shared, 0)
        return
    t0 = clock()
    _save_sample(stem, ctx, bundles[0], shared)
    marks['save'] = clock() - t0
    logger.info('Done')


def read_sample_file(sample_file):
    """[(genes.tpm, outbase)] from a file of tab separated lines `genes.tpm<TAB>outbase`; blank lines and lines that
    start with # are skipped."""
    return [(tpm, outbase) for _, tpm, outbase in _match_lines(sample_file, 'genes.tpm<TAB>outbase')]


def reconstruct_many(expression_files, outbases, tprob_file: str, avec_file: str = None, gpos_file: str = None,
                     expr_threshold: float = 1.5, sigma: float = 0.12, device: int = 0, batch_size: int = 64,
                     grid_file: str = None, grid_genoprobs: bool = False, stage_times: dict = None,
                     context: ReconstructContext = None, sim_geno: int = None, sim_geno_seed: int = 0,
                     diagnostics: bool = False, error_lod_threshold: float = 2.0, gene_report: str = None,
                     loglik: bool = False, alt_tprob_files=None, model_report: str = None,
                     match_panel: str = None, match_labels: str = None, match_chromosomes=None, match_report: str = None,
                     match_matrix: str = None, match_expected: str = None, snp_file: str = None,
                     snp_matrix: str = None, scan_pheno: str = None, scan_covar: str = None, scan_rankz: bool = False,
                     scan_out: str = None, scan_min_lod: float = None, scan_lod_matrix: bool = False,
                     scan_perms: int = None, scan_perm_seed: int = None, scan_perm_alpha=None, scan_perm_chromosomes=None,
                     scan_perm_pheno: str = None, scan_snps: bool = False, scan_mediate: bool = False,
                     scan_mediate_min_lod: float = None, scan_mediate_top: int = None, scan_mediator_file: str = None,
                     scan_effects: bool = False, scan_effects_min_lod: float = None, scan_lod_drop: float = None,
                     scan_kinship: str = None, scan_kinship_out: bool = False, scan_kinship_snps: str = None,
                     scan_kinship_effects: bool = False, scan_kinship_effects_min_lod: float = None,
                     scan_kinship_lod_drop: float = None, scan_intcovar: str = None) -> list:
    """`gbrs reconstruct` for a cohort whose genes.tpm files exist (extension): one context, the tables on the device
    once, the samples through the HMM in launches of up to `batch_size`, and every pass the options ask for once per
    launch.  Every sample gets the files the single-sample call writes for its outbase.  All samples must carry the same
    haplotype header (RuntimeError before anything runs otherwise).  A sample whose file cannot be read or lacks a gene
    is logged and left out, and the others go on.  Returns one dict per sample: its outbase and, if it failed,
    `error`.  `stage_times`, `context` and `grid_file` as in reconstruct; every other keyword from `expr_threshold` on is
    described on ReconstructOptions, with what it means for a cohort."""
    options = ReconstructOptions.of(locals())
    options.check(True, grid_file if context is None else context.grid_file, tprob_file)
    from . import scan as scan_mod
    scan_perm = scan_mod.perm_options(scan_perms, scan_perm_seed, scan_perm_alpha, scan_perm_chromosomes, scan_perm_pheno)
    scan_med = scan_mod.mediate_options(scan_mediate, scan_mediate_min_lod, scan_mediate_top, scan_mediator_file)
    scan_eff = scan_mod.effects_options(scan_effects, scan_effects_min_lod, scan_lod_drop)
    scan_kin_eff = scan_mod.kinship_effects_options(scan_kinship_effects, scan_kinship_effects_min_lod, scan_kinship_lod_drop,
                                                    scan_kinship)
    with_effects = any(e is not None and e['min_lod'] is not None for e in (scan_eff, scan_kin_eff))
    scan_kin = scan_mod.kinship_options(scan_kinship, scan_kinship_out, scan_perms, scan_snps, scan_mediate, scan_effects,
                                        scan_lod_drop)
    scan_int = scan_mod.intcovar_options(scan_intcovar, scan_covar, scan_kinship)
    clock = time.perf_counter
    marks = stage_times if stage_times is not None else {}
    if len(expression_files) != len(outbases):
        raise ValueError('one outbase per expression file')
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1')
    done = [{'outbase': o} for o in outbases]

    def failed(k, error):
        logger.error(f'{expression_files[k]}: {error}')
        done[k]['error'] = f'{type(error).__name__}: {error}'

    headers = {}
    for k, f in enumerate(expression_files):
        try:
            with open(f) as fh:
                headers[k] = tuple(fh.readline().rstrip().split('\t')[1:-1])
        except OSError as e:
            failed(k, e)
    if len(set(headers.values())) > 1:
        raise RuntimeError('the samples do not carry the same haplotypes: ' +
                           ' / '.join(','.join(h) for h in sorted(set(headers.values()))))
    if not headers:
        return done
    haplotypes = list(next(iter(headers.values())))
    num_haps = len(haplotypes)
    ctx = context if context is not None else ReconstructContext(tprob_file, avec_file, gpos_file, device, grid_file,
                                                                 options.alt_tprob_files)
    _lib.warm_up_device_async(device)
    t0 = clock()
    ctx.load()
    if options.loglik and ctx.alt_tprob_files and ctx.chroms:
        ctx.alt_tables(num_haps)           # a file that does not fit is refused before any sample runs
    labels = read_match_labels(match_labels) if match_labels is not None else {}
    shared = _Shared(ctx, options, haplotypes, tprob_file, marks, lambda line: None, 'hmm',
                     {k: labels[o] for k, o in enumerate(outbases) if o in labels})
    scan = scan_ids = None                 # the cohort's GenomeScan (made with the first launch) and its samples' outbases
    scan_held = shared.scan_held
    if scan_pheno is not None:
        scan_tables = (scan_mod.read_scan_pheno(scan_pheno),
                       scan_mod.read_scan_covar(scan_covar) if scan_covar is not None else None)
        scan_ids = []
        scan_unsaved = set()               # samples whose files could not be written: reported once, left out of the scan
        shared.scan_keep = set(scan_mod.scan_design(outbases, *scan_tables)[0])
        if scan_perm is not None:          # a name the table or the grid does not have is refused before a sample runs
            scan_mod.perm_plan(scan_perm, scan_tables[0][0], [str(c) for c in ctx.chroms])
        if scan_int is not None:           # a name the covariate table does not have, likewise
            scan_mod.intcovar_plan(scan_int, scan_tables[1][0])
        if scan_med is not None and scan_med['mediator_file'] is not None:      # a table that cannot be read, likewise
            scan_med['table'] = scan_mod.read_scan_pheno(scan_med['mediator_file'])
        if scan_kinship_snps is not None:  # the mixed model's own SNP file, by --snp-file's parser, likewise
            scan_kin_snps = read_snp_file(scan_kinship_snps, haplotypes, ctx.chroms, ctx.grid_file)
    marks['load'] = clock() - t0
    for key in ('read', 'hmm', 'grid', 'save') + (('loglik',) if options.loglik else ()) + \
            (('match',) if match_panel is not None else ()) + (('snp',) if snp_file is not None else ()) + \
            (('scan',) if scan_pheno is not None else ()) + (('scan_perm',) if scan_perm is not None else ()) + \
            (('scan_snps',) if scan_snps or scan_kinship_snps is not None else ()) + (('mediate',) if scan_med is not None else ()) + \
            (('effects',) if with_effects else ()):
        marks[key] = 0.0
    from concurrent.futures import ThreadPoolExecutor
    writers = ThreadPoolExecutor(max_workers=min(16, batch_size))
    pending = []

    def write_out(on, bundles):
        t0 = clock()
        for k, bundle in bundles.items():
            pending.append((k, writers.submit(_save_sample, outbases[k], on, bundle, shared, 1)))
        marks['save'] += clock() - t0

    try:
        order = sorted(headers)
        for lo in range(0, len(order), batch_size):
            t0 = clock()
            members, rows = [], []
            for k in order[lo:lo + batch_size]:
                try:
                    _, expr_row, expr_table = read_gene_tpm(expression_files[k])
                    rows.append(_expression_rows(ctx, expr_row, expr_table, num_haps))
                    members.append(k)
                except Exception as e:   # noqa: BLE001 - one bad sample does not end the cohort
                    failed(k, e)
            marks['read'] += clock() - t0
            if not members or not ctx.chroms:
                write_out(ctx, {k: _nothing_ran(ctx, shared, k) for k in members})
                continue
            bundles, moved = _launch(ctx, members, rows, shared)
            write_out(ctx, bundles)
            # The samples an alternative explains better, under a handle on that file: each in a launch of its own, which
            # is the single-sample command's launch, so its files do not depend on who else moved or on the batch size.
            for k, a in sorted((k, a) for a in moved for k in moved[a]):
                write_out(ctx.alt_context(a), _launch(ctx.alt_context(a), [k], [rows[members.index(k)]], shared)[0])
            if scan_pheno is not None and scan_held:
                # A sample that failed is left out, and a sample has not succeeded before its files are written: the
                # batch's writes are waited for here (with the scan they do not overlap the next launch).  Then the
                # batch's samples in file order: device to device when the whole launch goes in (no sample moved to
                # another handle, failed or lacks a row), else the rows the grid pass already brought to the host - the
                # same bits either way.
                t0 = clock()
                for k, job in pending:
                    if k in scan_held:
                        try:
                            job.result()
                        except Exception as e:   # noqa: BLE001
                            failed(k, e)
                            scan_unsaved.add(k)
                            del scan_held[k]
                marks['save'] += clock() - t0
            if scan_pheno is not None and scan_held:
                t0 = clock()
                if scan is None:
                    scan = scan_mod.GenomeScan(num_haps, ctx.hmm.grid_points, device=ctx.device)
                if not moved and sorted(scan_held) == members:
                    scan.append_from(ctx.hmm)
                else:
                    scan.append(np.stack([scan_held[k] for k in sorted(scan_held)]))
                scan_ids += [outbases[k] for k in sorted(scan_held)]
                scan_held.clear()
                marks['scan'] += clock() - t0
        t0 = clock()
        for k, job in pending:
            if scan_pheno is not None and k in scan_unsaved:
                continue
            try:
                job.result()
            except Exception as e:   # noqa: BLE001
                failed(k, e)
        if gene_report is not None:
            (shared.report if shared.report is not None else GeneReport(ctx, error_lod_threshold)).write(gene_report)
        if model_report is not None:
            write_model_report(model_report, shared.names, [(outbases[k],) + shared.choices[k] for k in sorted(shared.choices)])
        if match_panel is not None:
            matches, ran = shared.matches, sorted(shared.matches)
            if match_report is not None:
                write_match_report(match_report, [(outbases[k], matches[k][4]) for k in ran])
            if match_matrix is not None:
                M, nc = len(ctx.panel[0]), len(ctx.chroms)
                stack = lambda i, shape: np.stack([matches[k][i] for k in ran]) if ran else np.zeros(shape)
                write_match_matrix(match_matrix, [outbases[k] for k in ran], ctx.panel[0], ctx.chroms, shared.match_points,
                                   stack(2, (0, M)), stack(3, (0, M)), stack(0, (0, nc, M)), stack(1, (0, nc)),
                                   shared.panel_norm if shared.panel_norm is not None else np.zeros((M, nc)))
        if snp_matrix is not None:
            ran = sorted(shared.snp_rows)
            write_snp_matrix(snp_matrix, [outbases[k] for k in ran],
                             np.stack([shared.snp_rows[k] for k in ran]) if ran else np.zeros((0, len(shared.snps['snp_id']))),
                             shared.snps)
        marks['save'] += clock() - t0
        if scan_pheno is not None:
            t0 = clock()
            if scan is None:
                raise RuntimeError('scan: no sample that ran has a phenotype row')
            slices = sorted((v[1], v[2], c) for c, v in ctx.grid_slices.items())
            scan_mod.finish_scan(scan, scan_out if scan_out is not None else 'gbrs', scan_ids, scan_tables[0], scan_tables[1],
                                 scan_rankz, np.concatenate([[c] * m for _, m, c in slices]),
                                 np.concatenate([np.asarray(ctx.grid[c], dtype=np.float64) for _, _, c in slices]),
                                 list(ctx.chroms), scan_min_lod, scan_lod_matrix, perm=scan_perm, stage_times=marks,
                                 snps=shared.snps if scan_snps else None, snp_grid=ctx.grid, mediate=scan_med,
                                 effects=scan_eff, founders=haplotypes, kinship=scan_kin,
                                 kinship_snps=scan_kin_snps if scan_kinship_snps is not None else None,
                                 kinship_effects=scan_kin_eff, intcovar=scan_int)
            marks['scan'] += clock() - t0 - (marks['scan_perm'] if scan_perm is not None else 0.0) - \
                (marks['scan_snps'] if scan_snps or scan_kinship_snps is not None else 0.0) - (marks['mediate'] if scan_med is not None else 0.0) - \
                (marks['effects'] if with_effects else 0.0)
    finally:
        writers.shutdown(wait=True)
        if scan is not None:
            scan.close()
        if context is None:
            ctx.close()
    logger.info('Done')
    return done


