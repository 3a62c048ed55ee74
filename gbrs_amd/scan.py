"""Genome scan of phenotypes on founder dosages (extension): `gbrs reconstruct --scan-pheno` and
`gbrs scan`.  Haley-Knott regression with additive covariates on the device (gbrs_scan_*, gbrs_amd/csrc/scan.hip); the
host side here is the covariates' QR, the file readers and the writers.  `--scan-kinship loco|overall`: the
linear mixed model with a kinship of the cohort's own dosages (gbrs_scan_kinship, gbrs_scan_lmm_prepare, gbrs_scan_lmm_run);
the host side is the kinships' eigendecomposition; `--scan-kinship-snps FILE`: the 1-df test of founder
SNPs under that model, after the scan and at its heritabilities (gbrs_scan_lmm_snps).  `--scan-snps` / `gbrs scan
--snp-file`: the 1-df test of founder SNPs on the same prepared cohort (gbrs_scan_set_snps, gbrs_scan_snps).
`--scan-mediate`: the scan's peaks conditioned on every other phenotype in turn (gbrs_scan_mediate).
`--scan-effects`, `--scan-lod-drop`: the founder effects at the scan's peaks with their standard errors
(gbrs_scan_effects) and the peaks' LOD support intervals (gbrs_scan_run_support); `--scan-kinship-effects`,
`--scan-kinship-lod-drop`: both under the mixed model (gbrs_scan_lmm_effects, gbrs_scan_lmm_run_support).
`--scan-intcovar NAME[,NAME...]`: the scan with interactive covariates, QTL x covariate, on a preparation
of its own (gbrs_scan_int_prepare, gbrs_scan_int_run)."""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _lib

logger = logging.getLogger('gbrs')

COVARIATE_RANK_TOL = 1e-10        # a covariate column whose |R_jj| is below this share of its norm depends on the columns before it
LOD_MATRIX_LIMIT = 1 << 27        # P x M up to which <out>.scan.npz holds the LOD matrix without being asked
DEFAULT_PERM_ALPHA = (0.05, 0.1)  # the levels of --scan-perm-alpha
DEFAULT_MEDIATE_MIN_LOD = 6.0     # --scan-mediate-min-lod: the peaks that are mediated; a convention, not a threshold
DEFAULT_MEDIATE_TOP = 5           # --scan-mediate-top: the mediators listed per peak
MEDIATE_MAX_TOP = 64              # the places gbrs_scan_mediate's top list has
DEFAULT_EFFECTS_MIN_LOD = DEFAULT_MEDIATE_MIN_LOD     # --scan-effects-min-lod: the peaks whose founder effects are formed
KINSHIP_MODES = ('loco', 'overall')                   # --scan-kinship
LMM_MAX_COVARIATES = 16                               # covariate columns of the mixed model, the intercept included


class GenomeScan:
    """Device handle of one cohort on one grid.  append / append_from collect the samples' grid dosages in order,
    prepare(covariates) builds the phenotype-independent part once, run(pheno) scans any number of phenotypes;
    set_snps + run_snps(pheno) test founder SNPs with one degree of freedom on the same cohort;
    mediate(target, point, mediator) conditions peaks on mediators; effects(pheno, column, point) gives
    the founder effects at chosen points and run(pheno, lod_drop=d) the peaks' LOD support intervals;
    kinship() gives the cohort's kinship matrices, prepare_lmm(covariates, kinship) + run_lmm(pheno) scan under the linear
    mixed model, independent of prepare / run."""

    def __init__(self, num_haps, points_per_chrom, device=0):
        self.H = int(num_haps)
        self.points = np.ascontiguousarray(points_per_chrom, dtype=np.int32)
        self.M = int(self.points.sum())
        self.n = 0
        self.prepared = False
        self.lmm_prepared = False
        self.int_prepared = False
        self.eig_of_chrom = None
        self._dosage_total = 1.0
        h = C.c_void_p()
        _lib.check(_lib.load().gbrs_scan_create(int(device), len(self.points), _lib.ptr(self.points), self.H, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None) is not None:
            _lib.load().gbrs_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, dosage):
        """[n, M, H] (or [M, H]) founder dosages, rows as `DiplotypeHMM.grid()['dosage']` has them."""
        d = np.ascontiguousarray(dosage, dtype=np.float64)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1:] != (self.M, self.H):
            raise ValueError(f'dosage has shape {np.shape(dosage)}, expected (n, {self.M}, {self.H})')
        _lib.check(_lib.load().gbrs_scan_append(self._h, len(d), _lib.ptr(d)))
        if self.n == 0 and len(d):
            self._dosage_total = float(np.round(d[0, 0].sum(), 12))     # 1.0 for rows that add up to 1 within rounding
        self.n += len(d)
        self.prepared = False
        self.lmm_prepared = False
        self.int_prepared = False

    def append_from(self, hmm, sample=None):
        """The grid dosages of `hmm`'s last run, device to device: every sample of the run, or the one given."""
        _lib.check(_lib.load().gbrs_scan_append_hmm(self._h, hmm._h, -1 if sample is None else int(sample)))
        self.n += hmm.n_samples if sample is None else 1
        self.prepared = False
        self.lmm_prepared = False
        self.int_prepared = False

    def prepare(self, covariates=None, names=None):
        """covariates: [n, c] with the intercept (a column of ones) first, or None for the intercept alone."""
        z = np.ones((self.n, 1)) if covariates is None else np.ascontiguousarray(covariates, dtype=np.float64)
        if z.ndim != 2 or z.shape[0] != self.n:
            raise ValueError(f'covariates have shape {z.shape} for {self.n} samples')
        qz = covariate_basis(z, names)
        self.prepared = False
        _lib.check(_lib.load().gbrs_scan_prepare(self._h, qz.shape[1], _lib.ptr(qz)))
        self.prepared = True

    def run(self, pheno, want_lod=True, lod_drop=None):
        """pheno: [n, P] (or [n]).  Returns `peak_lod` [P, n_chrom], `peak_index` [P, n_chrom] and, with want_lod, `lod`
        [P, M].  A column whose values are all equal lies in the intercept's span: it goes to the device as zeros, so its
        rss0 is exactly 0 and its LODs are 0.0 whatever the rounding of the projection.  With lod_drop (a number that is
        not negative) the same pass also returns `support_lo` and `support_hi` [P, n_chrom]: the nearest
        grid points on either side of a peak whose LOD is at most the peak's minus lod_drop, the chromosome's ends where
        there is none, -1 for a chromosome without points."""
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n or y.shape[1] < 1:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        if self.n:
            y[:, (y == y[0]).all(axis=0)] = 0.0
        P, nc = y.shape[1], len(self.points)
        lod = np.empty((P, self.M)) if want_lod else None
        peak, index = np.empty((P, nc)), np.empty((P, nc), dtype=np.int64)
        if lod_drop is None:
            _lib.check(_lib.load().gbrs_scan_run(self._h, P, _lib.ptr(y), _lib.ptr(lod), _lib.ptr(peak), _lib.ptr(index)))
            out = {'peak_lod': peak, 'peak_index': index}
        else:
            lo, hi = np.empty((P, nc), dtype=np.int64), np.empty((P, nc), dtype=np.int64)
            _lib.check(_lib.load().gbrs_scan_run_support(self._h, P, _lib.ptr(y), float(lod_drop), _lib.ptr(lod), _lib.ptr(peak),
                                                         _lib.ptr(index), _lib.ptr(lo), _lib.ptr(hi)))
            out = {'peak_lod': peak, 'peak_index': index, 'support_lo': lo, 'support_hi': hi}
        if want_lod:
            out['lod'] = lod
        return out

    def permute(self, pheno, n_perm, seed=0, chromosomes=None, want_index=False):
        """Permutation maxima of the prepared cohort (Freedman-Lane: the residuals of the covariate model
        are permuted).  pheno: [n, P] (or [n]), with run()'s constant-column-to-zeros step; chromosomes: a mask [n_chrom]
        of the chromosomes the maximum is taken over (default: all).  Returns `perm_max` [P, n_perm] and, with
        want_index, `perm_index` [n_perm, n] - the permutations, which depend on (seed, permutation, n) alone."""
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        if self.n:
            y[:, (y == y[0]).all(axis=0)] = 0.0
        P, B = y.shape[1], int(n_perm)
        mask = None
        if chromosomes is not None:
            mask = np.ascontiguousarray(chromosomes, dtype=bool).astype(np.uint8)
            if mask.shape != (len(self.points),):
                raise ValueError(f'the chromosome mask has shape {mask.shape} for {len(self.points)} chromosomes')
        perm_max = np.empty((P, max(B, 0)))
        index = np.empty((max(B, 0), self.n), dtype=np.int32) if want_index else None
        _lib.check(_lib.load().gbrs_scan_permute(self._h, P, _lib.ptr(y), B, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(mask),
                                                 _lib.ptr(perm_max), _lib.ptr(index)))
        out = {'perm_max': perm_max}
        if want_index:
            out['perm_index'] = index
        return out

    def perm_info(self):
        raw = _lib.ScanPermInfo()
        _lib.check(_lib.load().gbrs_scan_perm_info(self._h, C.byref(raw)))
        return {'P': raw.P, 'B': raw.B, 'permute_ms': raw.last_permute_ms, 'product_ms': raw.last_product_ms,
                'peak_device_bytes': raw.peak_device_bytes}

    def set_snps(self, grid_pos, snp_pos, masks):
        """The SNPs of the handle, per chromosome in the handle's order: grid_pos[c] the positions of
        the chromosome's grid points, snp_pos[c] the SNP positions in the same units (None or empty: it has none),
        masks[c] their founder patterns as uint32, bit h set when founder h carries the alternative allele.  The SNPs
        are numbered chromosome after chromosome, each in the order given.  All empty drops the SNPs.  Independent of
        prepare; appending samples keeps them."""
        nc = len(self.points)
        if len(grid_pos) != nc or len(snp_pos) != nc or len(masks) != nc:
            raise ValueError(f'{len(grid_pos)} grids, {len(snp_pos)} SNP position arrays and {len(masks)} pattern arrays for '
                             f'{nc} chromosomes')
        grid = [np.zeros(0) if g is None else np.ascontiguousarray(g, dtype=np.float64) for g in grid_pos]
        where = [np.zeros(0) if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in snp_pos]
        bits = [np.zeros(0, dtype=np.uint32) if m is None else np.ascontiguousarray(m, dtype=np.uint32) for m in masks]
        for c, (g, x, m) in enumerate(zip(grid, where, bits)):
            if g.shape != (int(self.points[c]),):
                raise ValueError(f'chromosome {c}: {g.shape} grid positions for {int(self.points[c])} grid points')
            if x.shape != m.shape or x.ndim != 1:
                raise ValueError(f'chromosome {c}: {x.shape} SNP positions and {m.shape} patterns')
        n_snps = np.asarray([len(x) for x in where], dtype=np.int64)
        _lib.check(_lib.load().gbrs_scan_set_snps(self._h, _lib.ptr_table(grid), _lib.ptr(n_snps), _lib.ptr_table(where),
                                                  _lib.ptr_table(bits)))
        self.snp_points = [int(m) for m in n_snps]
        self.M_snp = int(n_snps.sum())

    def snp_dosage(self, first=0, count=None):
        """x_s of the SNPs first .. first + count - 1 (default: to the last) in handle order: [n, count]."""
        total = self.snp_info()['M_snp']
        count = total - int(first) if count is None else int(count)
        out = np.empty((self.n, max(count, 0)))
        _lib.check(_lib.load().gbrs_scan_snp_dosage(self._h, int(first), count, _lib.ptr(out)))
        return out

    def run_snps(self, pheno, want_lod=True):
        """The 1-df test of every SNP of the handle on the prepared cohort.  pheno: [n, P] (or [n]), with run()'s
        constant-column-to-zeros step.  Returns `used` [M_snp] (bool), `peak_lod` [P, n_chrom], `peak_index`
        [P, n_chrom] (the SNP's index in handle order; NaN and -1 without a used SNP) and, with want_lod, `lod`
        [P, M_snp]."""
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        if self.n:
            y[:, (y == y[0]).all(axis=0)] = 0.0
        P, nc, M_snp = y.shape[1], len(self.points), self.snp_info()['M_snp']
        lod = np.empty((P, M_snp)) if want_lod else None
        used = np.zeros(M_snp, dtype=np.uint8)
        peak, index = np.empty((P, nc)), np.empty((P, nc), dtype=np.int64)
        _lib.check(_lib.load().gbrs_scan_snps(self._h, P, _lib.ptr(y), _lib.ptr(lod), _lib.ptr(used), _lib.ptr(peak),
                                              _lib.ptr(index)))
        out = {'used': used.astype(bool), 'peak_lod': peak, 'peak_index': index}
        if want_lod:
            out['lod'] = lod
        return out

    def snp_info(self):
        raw = _lib.ScanSnpInfo()
        _lib.check(_lib.load().gbrs_scan_snp_info(self._h, C.byref(raw)))
        return {'M_snp': raw.M_snp, 'chunk': raw.chunk, 'P': raw.P, 'pass_ms': raw.last_pass_ms, 'row_ms': raw.last_row_ms,
                'product_ms': raw.last_product_ms, 'device_bytes': raw.device_bytes,
                'peak_device_bytes': raw.peak_device_bytes, 'staged': bool(raw.staged)}

    def mediate(self, target, point, mediator, top=5, want_lod=False):
        """Mediation of the targets' LODs by every mediator on the prepared cohort.  target: [n, T] (or
        [n]) phenotype columns, point: [T] grid point indices (a target's peak), mediator: [n, Q] (or [n]); both tables
        with run()'s constant-column-to-zeros step.  Returns `lod0` [T], `n_used`, `mean`, `sd` [T] over the used
        mediators, `best_index`, `best_lod` [T, top] - the used mediators with the lowest mediated LOD in ascending
        (LOD, index) order, -1 / NaN in the missing places - and, with want_lod, `lod_med` [T, Q] and `used` [T, Q]
        (bool)."""
        tables = []
        for what, table in (('targets', target), ('mediators', mediator)):
            y = np.array(table, dtype=np.float64, order='C')
            if y.ndim == 1:
                y = y[:, None]
            if y.ndim != 2 or y.shape[0] != self.n:
                raise ValueError(f'{what} have shape {np.shape(table)} for {self.n} samples')
            if self.n:
                y[:, (y == y[0]).all(axis=0)] = 0.0
            tables.append(y)
        y, z = tables
        T, Q, K = y.shape[1], z.shape[1], int(top)
        at = np.ascontiguousarray(np.atleast_1d(point), dtype=np.int64)
        if at.shape != (T,):
            raise ValueError(f'{at.shape} grid points for {T} targets')
        lod0, mean, sd, count = np.empty(T), np.empty(T), np.empty(T), np.empty(T, dtype=np.int64)
        best, index = np.empty((T, max(K, 0))), np.empty((T, max(K, 0)), dtype=np.int64)
        lod = np.empty((T, Q)) if want_lod else None
        used = np.empty((T, Q), dtype=np.uint8) if want_lod else None
        _lib.check(_lib.load().gbrs_scan_mediate(self._h, T, _lib.ptr(y), _lib.ptr(at), Q, _lib.ptr(z), K, _lib.ptr(lod0),
                                                 _lib.ptr(lod), _lib.ptr(used), _lib.ptr(best), _lib.ptr(index), _lib.ptr(mean),
                                                 _lib.ptr(sd), _lib.ptr(count)))
        out = {'lod0': lod0, 'n_used': count, 'mean': mean, 'sd': sd, 'best_index': index, 'best_lod': best}
        if want_lod:
            out['lod_med'] = lod
            out['used'] = used.astype(bool)
        return out

    def mediate_info(self):
        raw = _lib.ScanMediateInfo()
        _lib.check(_lib.load().gbrs_scan_mediate_info(self._h, C.byref(raw)))
        return {'T': raw.T, 'Q': raw.Q, 'pass_ms': raw.last_pass_ms, 'product_ms': raw.last_product_ms,
                'peak_device_bytes': raw.peak_device_bytes}

    def effects(self, pheno, column, point):
        """Founder effects at chosen points of the prepared cohort.  pheno: [n, P] (or [n]), with run()'s
        constant-column-to-zeros step; column: [T] phenotype columns; point: [T] grid point indices (a column's peak).
        Returns `effect` and `se` [T, H] - the zero-sum effects of all H founders and their standard errors -, `lod` [T]
        (within rounding of run()'s LOD at the point), `sigma2` [T] (the residual variance) and `rank` [T]."""
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        if self.n:
            y[:, (y == y[0]).all(axis=0)] = 0.0
        col = np.ascontiguousarray(np.atleast_1d(column), dtype=np.int64)
        at = np.ascontiguousarray(np.atleast_1d(point), dtype=np.int64)
        if col.ndim != 1 or at.shape != col.shape:
            raise ValueError(f'{col.shape} phenotype columns and {at.shape} grid points')
        P, T = y.shape[1], len(col)
        effect, se = np.empty((T, self.H)), np.empty((T, self.H))
        lod, sigma2, rank = np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
        _lib.check(_lib.load().gbrs_scan_effects(self._h, P, _lib.ptr(y), T, _lib.ptr(col), _lib.ptr(at), _lib.ptr(effect),
                                                 _lib.ptr(se), _lib.ptr(lod), _lib.ptr(sigma2), _lib.ptr(rank)))
        return {'effect': effect, 'se': se, 'lod': lod, 'sigma2': sigma2, 'rank': rank}

    def effects_info(self):
        raw = _lib.ScanEffectsInfo()
        _lib.check(_lib.load().gbrs_scan_effects_info(self._h, C.byref(raw)))
        return {'T': raw.T, 'P': raw.P, 'pass_ms': raw.last_pass_ms, 'peak_device_bytes': raw.peak_device_bytes}

    def kinship(self, leave_out=None, scale=None):
        """The cohort's kinship [n, n] from its dosages on the device: scale x (sum over the chromosomes
        other than `leave_out` - an index, None: all of them - of A_c A_c') / (their grid points).  scale: default
        2 / t^2 with t the total of a grid point's dosages (R/qtl2's doubled kinship of allele probabilities): the first
        appended sample's first grid point, rounded at the twelfth decimal; 1 for a cohort appended from an HMM handle."""
        t = self._dosage_total
        scale = 2.0 / (t * t) if scale is None else float(scale)
        out = np.empty((self.n, self.n))
        _lib.check(_lib.load().gbrs_scan_kinship(self._h, -1 if leave_out is None else int(leave_out), scale, _lib.ptr(out)))
        return out

    def prepare_lmm(self, covariates=None, kinship='loco', names=None):
        """The mixed model's phenotype-independent part.  covariates: as for prepare(), at most 16 columns.
        kinship: 'loco' (one matrix per chromosome, from the other chromosomes), 'overall' (one, from all), an [n, n]
        array (the caller's, for every chromosome) or a list of one array per chromosome.  The matrices are factored here
        (numpy.linalg.eigh); one whose smallest eigenvalue is not above 1e-10 of its largest is refused.  Returns the
        matrices that were used, in the order of their decompositions; `eig_of_chrom` maps the chromosomes to them."""
        z = np.ones((self.n, 1)) if covariates is None else np.ascontiguousarray(covariates, dtype=np.float64)
        if z.ndim != 2 or z.shape[0] != self.n:
            raise ValueError(f'covariates have shape {z.shape} for {self.n} samples')
        if z.shape[1] > LMM_MAX_COVARIATES:
            raise ValueError(f'the mixed model takes at most {LMM_MAX_COVARIATES} covariate columns (the intercept included), '
                             f'got {z.shape[1]}')
        covariate_basis(z, names)               # its checks: finite values, the intercept first, full column rank
        nc = len(self.points)
        if isinstance(kinship, str):
            if kinship not in KINSHIP_MODES:
                raise ValueError(f'kinship must be one of {", ".join(KINSHIP_MODES)}, an array or a list of arrays, got {kinship}')
            if kinship == 'loco':
                matrices, eig_of_chrom = [self.kinship(leave_out=c) for c in range(nc)], list(range(nc))
            else:
                matrices, eig_of_chrom = [self.kinship()], [0] * nc
        elif isinstance(kinship, (list, tuple)):
            if len(kinship) != nc:
                raise ValueError(f'{len(kinship)} kinship matrices for {nc} chromosomes')
            matrices, eig_of_chrom = [np.asarray(k, dtype=np.float64) for k in kinship], list(range(nc))
        else:
            matrices, eig_of_chrom = [np.asarray(kinship, dtype=np.float64)], [0] * nc
        vectors, values = [], []
        for e, k in enumerate(matrices):
            if k.shape != (self.n, self.n):
                raise ValueError(f'kinship {e} has shape {k.shape} for {self.n} samples')
            if not np.isfinite(k).all():
                raise ValueError(f'kinship {e} holds a value that is not finite')
            lam, u = np.linalg.eigh(k)
            vectors.append(np.ascontiguousarray(u))
            values.append(np.ascontiguousarray(lam))
        mapping = np.asarray(eig_of_chrom, dtype=np.int32)
        _lib.check(_lib.load().gbrs_scan_lmm_prepare(self._h, z.shape[1], _lib.ptr(z), len(matrices), _lib.ptr_table(vectors),
                                                     _lib.ptr_table(values), _lib.ptr(mapping)))
        self.lmm_prepared = True
        self.eig_of_chrom = mapping
        return matrices

    def _lmm_inputs(self, pheno, hsq):
        """What a pass under the mixed model uploads: (y [n, P] with every column's mean subtracted and a constant column as
        zeros, hsq per decomposition [P, n_eig] or None, n_eig)."""
        if not self.lmm_prepared:
            raise _lib.GbrsHipError(_lib.GBRS_ERR_INVALID, 'no mixed model on the handle: call prepare_lmm first')
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n or y.shape[1] < 1:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        constant = (y == y[0]).all(axis=0)
        if np.isfinite(y).all():        # a column's mean from the column alone, whatever stands beside it: its own contiguous row
            y = np.ascontiguousarray(y - np.ascontiguousarray(y.T).sum(axis=1) / self.n)
        y[:, constant] = 0.0
        P, nc, mapping = y.shape[1], len(self.points), self.eig_of_chrom
        n_eig = int(mapping.max()) + 1
        given = None
        if hsq is not None:
            by_chrom = np.asarray(hsq, dtype=np.float64)
            if by_chrom.shape != (P, nc):
                raise ValueError(f'hsq has shape {by_chrom.shape}, expected ({P}, {nc})')
            first = [int(np.flatnonzero(mapping == e)[0]) for e in range(n_eig)]
            given = np.ascontiguousarray(by_chrom[:, first])
        return y, given, n_eig

    def run_snps_lmm(self, pheno, want_lod=True, hsq=None):
        """The 1-df test of every SNP of the handle under the prepared mixed model (R/qtl2's scan1snps
        with kinship).  pheno and hsq as for run_lmm, centred by the same code; hsq is [P, n_chrom], for instance what
        run_lmm fitted, so that both passes use the same heritability per chromosome.  Returns `peak_lod`, `peak_index`
        (the SNP's index in handle order; NaN and -1 without a used SNP) and `n_used` [P, n_chrom], `hsq` and `sigma2`
        [P, n_chrom] and, with want_lod, `lod` [P, M_snp] and `used` [P, M_snp] (bool: the weights, and so the test's
        threshold, depend on the phenotype)."""
        y, given, n_eig = self._lmm_inputs(pheno, hsq)
        P, nc, mapping, M_snp = y.shape[1], len(self.points), self.eig_of_chrom, self.snp_info()['M_snp']
        lod = np.empty((P, M_snp)) if want_lod else None
        used = np.zeros((P, M_snp), dtype=np.uint8) if want_lod else None
        peak, index, count = np.empty((P, nc)), np.empty((P, nc), dtype=np.int64), np.empty((P, nc), dtype=np.int64)
        fitted, sigma2 = np.empty((P, n_eig)), np.empty((P, n_eig))
        _lib.check(_lib.load().gbrs_scan_lmm_snps(self._h, P, _lib.ptr(y), _lib.ptr(given), _lib.ptr(lod), _lib.ptr(used),
                                                  _lib.ptr(peak), _lib.ptr(index), _lib.ptr(count), _lib.ptr(fitted),
                                                  _lib.ptr(sigma2)))
        out = {'peak_lod': peak, 'peak_index': index, 'n_used': count, 'hsq': fitted[:, mapping], 'sigma2': sigma2[:, mapping]}
        if want_lod:
            out['lod'] = lod
            out['used'] = used.astype(bool)
        return out

    def lmm_snp_info(self):
        raw = _lib.ScanLmmSnpInfo()
        _lib.check(_lib.load().gbrs_scan_lmm_snp_info(self._h, C.byref(raw)))
        return {'M_snp': raw.M_snp, 'chunk': raw.chunk, 'P': raw.P, 'pass_ms': raw.last_pass_ms, 'null_ms': raw.last_null_ms,
                'rotate_ms': raw.last_rotate_ms, 'product_ms': raw.last_product_ms, 'column_bytes': raw.column_bytes,
                'peak_device_bytes': raw.peak_device_bytes}

    def run_lmm(self, pheno, want_lod=True, hsq=None, lod_drop=None):
        """pheno: [n, P] (or [n]) under the prepared mixed model.  Every column's mean is subtracted before the upload (the
        intercept absorbs it) and a constant column goes as zeros: hsq 0 and LODs 0.0.  hsq: [P, n_chrom] heritabilities
        in [0, 1] to scan with instead of fitting them (chromosomes that share a decomposition must agree; the first
        one's value is taken).  Returns `peak_lod`, `peak_index` [P, n_chrom], `hsq` and `sigma2` [P, n_chrom] (per
        chromosome, through `eig_of_chrom`), `rank_min`, `rank_max` [P] and, with want_lod, `lod` [P, M].  lod_drop: with
        a number the pass also forms every peak's LOD support interval by run()'s rule and the dict gains
        `support_lo` and `support_hi` [P, n_chrom], grid indices, -1 for a chromosome without points; everything else is
        the same bits."""
        y, given, n_eig = self._lmm_inputs(pheno, hsq)
        P, nc, mapping = y.shape[1], len(self.points), self.eig_of_chrom
        lod = np.empty((P, self.M)) if want_lod else None
        peak, index = np.empty((P, nc)), np.empty((P, nc), dtype=np.int64)
        fitted, sigma2 = np.empty((P, n_eig)), np.empty((P, n_eig))
        if lod_drop is None:
            _lib.check(_lib.load().gbrs_scan_lmm_run(self._h, P, _lib.ptr(y), _lib.ptr(given), _lib.ptr(lod), _lib.ptr(peak),
                                                     _lib.ptr(index), _lib.ptr(fitted), _lib.ptr(sigma2)))
        else:
            lo, hi = np.empty((P, nc), dtype=np.int64), np.empty((P, nc), dtype=np.int64)
            _lib.check(_lib.load().gbrs_scan_lmm_run_support(self._h, P, _lib.ptr(y), _lib.ptr(given), float(lod_drop),
                                                             _lib.ptr(lod), _lib.ptr(peak), _lib.ptr(index), _lib.ptr(fitted),
                                                             _lib.ptr(sigma2), _lib.ptr(lo), _lib.ptr(hi)))
        rank_min, rank_max = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
        _lib.check(_lib.load().gbrs_scan_lmm_ranks(self._h, _lib.ptr(rank_min), _lib.ptr(rank_max)))
        out = {'peak_lod': peak, 'peak_index': index, 'hsq': fitted[:, mapping], 'sigma2': sigma2[:, mapping],
               'rank_min': rank_min, 'rank_max': rank_max}
        if want_lod:
            out['lod'] = lod
        if lod_drop is not None:
            out['support_lo'], out['support_hi'] = lo, hi
        return out

    def effects_lmm(self, pheno, column, point, hsq=None):
        """Founder effects at chosen points under the prepared mixed model.  pheno and hsq as for run_lmm,
        centred by the same code; hsq is [P, n_chrom], for instance what run_lmm fitted.  column: [T] phenotype columns;
        point: [T] grid point indices (a column's peak).  Returns `effect` and `se` [T, H] - the generalised-least-squares
        effects of all H founders and their standard errors -, `lod` [T] (run_lmm's bits at the point), `sigma2` [T] (the
        residual variance on the whitened scale), `hsq` [T] (the heritability the target was formed with) and `rank` [T]."""
        y, given, n_eig = self._lmm_inputs(pheno, hsq)
        col = np.ascontiguousarray(np.atleast_1d(column), dtype=np.int64)
        at = np.ascontiguousarray(np.atleast_1d(point), dtype=np.int64)
        if col.ndim != 1 or at.shape != col.shape:
            raise ValueError(f'{col.shape} phenotype columns and {at.shape} grid points')
        P, T = y.shape[1], len(col)
        effect, se = np.empty((T, self.H)), np.empty((T, self.H))
        lod, sigma2, fitted, rank = np.empty(T), np.empty(T), np.empty(T), np.empty(T, dtype=np.int32)
        _lib.check(_lib.load().gbrs_scan_lmm_effects(self._h, P, _lib.ptr(y), _lib.ptr(given), T, _lib.ptr(col), _lib.ptr(at),
                                                     _lib.ptr(effect), _lib.ptr(se), _lib.ptr(lod), _lib.ptr(sigma2),
                                                     _lib.ptr(rank), _lib.ptr(fitted)))
        return {'effect': effect, 'se': se, 'lod': lod, 'sigma2': sigma2, 'hsq': fitted, 'rank': rank}

    def lmm_effects_info(self):
        raw = _lib.ScanLmmEffectsInfo()
        _lib.check(_lib.load().gbrs_scan_lmm_effects_info(self._h, C.byref(raw)))
        return {'T': raw.T, 'P': raw.P, 'columns': raw.columns, 'pass_ms': raw.last_pass_ms, 'null_ms': raw.last_null_ms,
                'target_ms': raw.last_target_ms, 'peak_device_bytes': raw.peak_device_bytes}

    def lmm_info(self):
        raw = _lib.ScanLmmInfo()
        _lib.check(_lib.load().gbrs_scan_lmm_info(self._h, C.byref(raw)))
        return {'cz': raw.cz, 'n_eig': raw.n_eig, 'P': raw.P, 'kinship_ms': raw.last_kinship_ms, 'rotate_ms': raw.last_rotate_ms,
                'null_ms': raw.last_null_ms, 'point_ms': raw.last_point_ms, 'run_ms': raw.last_run_ms,
                'device_bytes': raw.device_bytes, 'peak_device_bytes': raw.peak_device_bytes}

    def prepare_int(self, covariates, interactive, names=None):
        """The phenotype-independent part of the scan with interactive covariates (R/qtl2's scan1 with
        intcovar).  covariates: as for prepare(), [n, c] with the intercept first; interactive: indices of the columns of
        `covariates` that also interact with the QTL - not 0, the intercept, and none twice.  As in qtl2 the interactive
        covariates are additive covariates too: they are taken from `covariates`, as given and not centred.  Independent
        of prepare() and prepare_lmm()."""
        z = np.ascontiguousarray(covariates, dtype=np.float64)
        if z.ndim != 2 or z.shape[0] != self.n:
            raise ValueError(f'covariates have shape {z.shape} for {self.n} samples')
        which = [int(j) for j in np.atleast_1d(interactive)]
        if not which:
            raise ValueError('no interactive covariate was named')
        for j in which:
            if j == 0:
                raise ValueError('the intercept (column 0) cannot be an interactive covariate')
            if not 0 < j < z.shape[1]:
                raise ValueError(f'interactive covariate {j} is not a column of the {z.shape[1]} covariates')
        if len(set(which)) != len(which):
            raise ValueError(f'an interactive covariate is named twice: {which}')
        qz = covariate_basis(z, names)
        zint = np.ascontiguousarray(z[:, which])
        self.int_prepared = False
        _lib.check(_lib.load().gbrs_scan_int_prepare(self._h, qz.shape[1], _lib.ptr(qz), len(which), _lib.ptr(zint)))
        self.int_prepared = True

    def run_int(self, pheno, want_lod=True):
        """pheno: [n, P] (or [n]) under the prepared interaction model, with run()'s constant-column-to-zeros step.  Returns
        `peak_full`, `peak_full_index` [P, n_chrom] (the peaks of the full model's LOD, additive + interaction columns
        against the covariates), `peak_full_add` (the additive model's LOD at that index), `peak_int`, `peak_int_index`
        (the peaks of the interaction's LOD, full against additive) and, with want_lod, `lod_full`, `lod_add` and `lod_int`
        [P, M].  `lod_add` carries the bits of run()'s `lod` after prepare() with the same covariates; `lod_int` is never
        negative."""
        y = np.array(pheno, dtype=np.float64, order='C')
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.n or y.shape[1] < 1:
            raise ValueError(f'phenotypes have shape {np.shape(pheno)} for {self.n} samples')
        if self.n:
            y[:, (y == y[0]).all(axis=0)] = 0.0
        P, nc = y.shape[1], len(self.points)
        full, add, inter = (np.empty((P, self.M)) if want_lod else None for _ in range(3))
        peak_full, peak_add, peak_int = np.empty((P, nc)), np.empty((P, nc)), np.empty((P, nc))
        index_full, index_int = np.empty((P, nc), dtype=np.int64), np.empty((P, nc), dtype=np.int64)
        _lib.check(_lib.load().gbrs_scan_int_run(self._h, P, _lib.ptr(y), _lib.ptr(full), _lib.ptr(add), _lib.ptr(inter),
                                                 _lib.ptr(peak_full), _lib.ptr(index_full), _lib.ptr(peak_add),
                                                 _lib.ptr(peak_int), _lib.ptr(index_int)))
        out = {'peak_full': peak_full, 'peak_full_index': index_full, 'peak_full_add': peak_add, 'peak_int': peak_int,
               'peak_int_index': index_int}
        if want_lod:
            out.update(lod_full=full, lod_add=add, lod_int=inter)
        return out

    def int_info(self):
        raw = _lib.ScanIntInfo()
        _lib.check(_lib.load().gbrs_scan_int_info(self._h, C.byref(raw), None, None))
        rank_full = rank_add = None
        if raw.c > 0:
            rank_full, rank_add = np.empty(raw.M, dtype=np.int32), np.empty(raw.M, dtype=np.int32)
            _lib.check(_lib.load().gbrs_scan_int_info(self._h, None, _lib.ptr(rank_full), _lib.ptr(rank_add)))
        return {'n': raw.n, 'M': raw.M, 'H': raw.H, 'c': raw.c, 'k': raw.k, 'HPI': raw.HPI, 'rank_full': rank_full,
                'rank_add': rank_add, 'prepare_ms': raw.last_prepare_ms, 'run_ms': raw.last_run_ms,
                'product_ms': raw.last_product_ms, 'device_bytes': raw.device_bytes}

    def info(self):
        raw = _lib.ScanInfo()
        _lib.check(_lib.load().gbrs_scan_info(self._h, C.byref(raw), None))
        rank = None
        if raw.c > 0:
            rank = np.empty(raw.M, dtype=np.int32)
            _lib.check(_lib.load().gbrs_scan_info(self._h, None, _lib.ptr(rank)))
        return {'n': raw.n, 'M': raw.M, 'H': raw.H, 'c': raw.c, 'rank': rank, 'prepare_ms': raw.last_prepare_ms,
                'run_ms': raw.last_run_ms, 'product_ms': raw.last_product_ms, 'device_bytes': raw.device_bytes}


def covariate_basis(z, names=None):
    """The orthonormal basis Qz [n, c] of the covariates (numpy QR; c is small).  The first column must be the intercept.
    A value that is not finite is refused naming the entry; a column that depends on the ones before it - |R_jj| at most
    COVARIATE_RANK_TOL times the column's norm - is refused by name."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    label = lambda j: f'{j}' if names is None else f'{j} ({names[j]})'
    bad = np.argwhere(~np.isfinite(z))
    if len(bad):
        raise ValueError(f'covariate column {label(int(bad[0][1]))} holds a value that is not finite (sample {int(bad[0][0])})')
    if z.shape[1] < 1 or not (z[:, 0] == 1.0).all():
        raise ValueError('the first covariate column must be the intercept (all ones)')
    if z.shape[0] < z.shape[1]:
        raise ValueError(f'{z.shape[0]} samples are too few for {z.shape[1]} covariate columns')
    q, r = np.linalg.qr(z)
    norms = np.sqrt((z * z).sum(axis=0))
    for j in range(z.shape[1]):
        if abs(r[j, j]) <= COVARIATE_RANK_TOL * norms[j]:
            raise ValueError(f'covariate column {label(j)} is a linear combination of the columns before it: '
                             'the covariates do not have full column rank')
    return np.ascontiguousarray(q)


def rankz(y):
    """Rank-based inverse normal transform of one phenotype: Phi^-1((r - 1/2) / n) of the 1-based ranks r, ties sharing
    the average of their ranks."""
    from statistics import NormalDist
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    order = np.argsort(y, kind='stable')
    ranks = np.empty(n)
    sorted_y = y[order]
    lo = 0
    while lo < n:
        hi = lo
        while hi + 1 < n and sorted_y[hi + 1] == sorted_y[lo]:
            hi += 1
        ranks[order[lo:hi + 1]] = 0.5 * (lo + hi) + 1.0
        lo = hi + 1
    inv = NormalDist().inv_cdf
    return np.array([inv((r - 0.5) / n) for r in ranks])


def perm_thresholds(perm_max, alphas):
    """threshold[p][a]: the ceil((1 - alpha_a) B)-th smallest of perm_max[p][:], an order statistic without
    interpolation.  (1 - alpha) B is rounded at the ninth decimal before the ceiling, so that 0.95 x 20 is 19."""
    import math
    pm = np.asarray(perm_max, dtype=np.float64)
    if pm.ndim != 2 or pm.shape[1] < 1:
        raise ValueError(f'perm_max has shape {pm.shape}, expected (phenotypes, permutations >= 1)')
    B = pm.shape[1]
    ordered = np.sort(pm, axis=1)
    out = np.empty((pm.shape[0], len(alphas)))
    for a, alpha in enumerate(alphas):
        if not 0.0 < alpha < 1.0:
            raise ValueError(f'a level must lie in (0, 1), got {alpha}')
        k = min(max(math.ceil(round((1.0 - alpha) * B, 9)), 1), B)
        out[:, a] = ordered[:, k - 1]
    return out


def perm_pvalues(perm_max, peak_lod, selected=None):
    """(1 + #{b : perm_max[p][b] >= x}) / (B + 1) for every observed peak x = peak_lod[p][...]; +inf compares as numpy
    compares it.  NaN for a peak that is NaN (a chromosome without points) and, with `selected` (a mask over peak_lod's
    last axis), for the chromosomes the permutations did not look at."""
    pm = np.asarray(perm_max, dtype=np.float64)
    peak = np.asarray(peak_lod, dtype=np.float64)
    if pm.ndim != 2 or peak.shape[:1] != pm.shape[:1]:
        raise ValueError(f'perm_max has shape {pm.shape}, the peaks {peak.shape}')
    flat = peak.reshape(len(pm), -1)
    with np.errstate(invalid='ignore'):
        count = (pm[:, None, :] >= flat[:, :, None]).sum(axis=2)
    p = np.where(np.isnan(flat), np.nan, (1.0 + count) / (pm.shape[1] + 1.0)).reshape(peak.shape)
    if selected is not None:
        p[..., ~np.asarray(selected, dtype=bool)] = np.nan
    return p


# ---- files ---------------------------------------------------------------------------------------------------------------

def perm_options(scan_perms=None, scan_perm_seed=None, scan_perm_alpha=None, scan_perm_chromosomes=None,
                 scan_perm_pheno=None):
    """`--scan-perms B [--scan-perm-seed S] [--scan-perm-alpha 0.05,0.1] [--scan-perm-chromosomes 1,2,...]
    [--scan-perm-pheno FILE]` as one dict, or None without `--scan-perms`; the other options are then refused.  Levels
    and chromosome names come as the command's comma separated text or as sequences.  Refused before a file is read."""
    if scan_perms is None:
        for name, value in (('--scan-perm-seed', scan_perm_seed), ('--scan-perm-alpha', scan_perm_alpha),
                            ('--scan-perm-chromosomes', scan_perm_chromosomes), ('--scan-perm-pheno', scan_perm_pheno)):
            if value is not None:
                raise RuntimeError(f'{name} needs --scan-perms')
        return None
    if int(scan_perms) != scan_perms or scan_perms < 1:
        raise RuntimeError(f'--scan-perms must be a whole number of at least 1, got {scan_perms}')
    seed = 0 if scan_perm_seed is None else int(scan_perm_seed)
    if not 0 <= seed < 1 << 64:
        raise RuntimeError(f'--scan-perm-seed must lie in 0 .. 2^64 - 1, got {scan_perm_seed}')
    split = lambda v: [x.strip() for x in v.split(',')] if isinstance(v, str) else list(v)
    try:
        alphas = [float(a) for a in split(DEFAULT_PERM_ALPHA if scan_perm_alpha is None else scan_perm_alpha)]
    except ValueError:
        raise RuntimeError(f'--scan-perm-alpha must be numbers separated by commas, got {scan_perm_alpha}') from None
    if not alphas or not all(0.0 < a < 1.0 for a in alphas):
        raise RuntimeError(f'--scan-perm-alpha: every level must lie in (0, 1), got {scan_perm_alpha}')
    chromosomes = None
    if scan_perm_chromosomes is not None:
        chromosomes = [str(c) for c in split(scan_perm_chromosomes)]
        if not chromosomes or '' in chromosomes:
            raise RuntimeError(f'--scan-perm-chromosomes must be names separated by commas, got {scan_perm_chromosomes}')
    return {'n_perm': int(scan_perms), 'seed': seed, 'alphas': alphas, 'chromosomes': chromosomes, 'pheno_file': scan_perm_pheno}


def perm_plan(perm, phenotypes, chrom_names=None):
    """(columns of `phenotypes` that are permuted, mask over `chrom_names`) of perm_options' dict: the names of
    `--scan-perm-pheno` (one per line; default: every phenotype) in the table's order and the chromosomes of
    `--scan-perm-chromosomes` (default: all).  A name the table or the grid does not have is refused.  Without
    chrom_names only the phenotypes are looked at and the mask is None."""
    columns = list(range(len(phenotypes)))
    if perm['pheno_file'] is not None:
        with open(perm['pheno_file']) as fh:
            wanted = [line.strip() for line in fh if line.strip()]
        unknown = [w for w in wanted if w not in phenotypes]
        if unknown:
            raise RuntimeError(f'{perm["pheno_file"]}: {unknown[0]} is no phenotype of the table')
        if not wanted:
            raise RuntimeError(f'{perm["pheno_file"]}: no phenotype is named')
        columns = [p for p, name in enumerate(phenotypes) if name in set(wanted)]
    if chrom_names is None:
        return columns, None
    mask = np.ones(len(chrom_names), dtype=bool)
    if perm['chromosomes'] is not None:
        unknown = [c for c in perm['chromosomes'] if c not in chrom_names]
        if unknown:
            raise RuntimeError(f'--scan-perm-chromosomes: {unknown[0]} is no chromosome of the grid '
                               f'({", ".join(str(c) for c in chrom_names)})')
        mask = np.array([str(c) in perm['chromosomes'] for c in chrom_names])
    return columns, mask


def mediate_options(scan_mediate=False, scan_mediate_min_lod=None, scan_mediate_top=None, scan_mediator_file=None):
    """`--scan-mediate [--scan-mediate-min-lod X] [--scan-mediate-top K] [--scan-mediator-file FILE]` as one dict, or None
    without `--scan-mediate`; the other options are then refused.  Refused before a file is read."""
    if not scan_mediate:
        for name, value in (('--scan-mediate-min-lod', scan_mediate_min_lod), ('--scan-mediate-top', scan_mediate_top),
                            ('--scan-mediator-file', scan_mediator_file)):
            if value is not None:
                raise RuntimeError(f'{name} needs --scan-mediate')
        return None
    min_lod = DEFAULT_MEDIATE_MIN_LOD if scan_mediate_min_lod is None else float(scan_mediate_min_lod)
    if not min_lod >= 0.0:
        raise RuntimeError(f'--scan-mediate-min-lod must be a number that is not negative, got {scan_mediate_min_lod}')
    top = DEFAULT_MEDIATE_TOP if scan_mediate_top is None else scan_mediate_top
    if int(top) != top or not 1 <= top <= MEDIATE_MAX_TOP:
        raise RuntimeError(f'--scan-mediate-top must be a whole number in 1 .. {MEDIATE_MAX_TOP}, got {scan_mediate_top}')
    return {'min_lod': min_lod, 'top': int(top), 'mediator_file': scan_mediator_file}


def effects_options(scan_effects=False, scan_effects_min_lod=None, scan_lod_drop=None):
    """`--scan-effects [--scan-effects-min-lod X]` and `--scan-lod-drop X` as one dict `{'min_lod': X or None without
    --scan-effects, 'lod_drop': X or None}`, or None with neither; `--scan-effects-min-lod` alone is refused.  Refused
    before a file is read."""
    if not scan_effects and scan_effects_min_lod is not None:
        raise RuntimeError('--scan-effects-min-lod needs --scan-effects')
    min_lod = None
    if scan_effects:
        min_lod = DEFAULT_EFFECTS_MIN_LOD if scan_effects_min_lod is None else float(scan_effects_min_lod)
        if not min_lod >= 0.0:
            raise RuntimeError(f'--scan-effects-min-lod must be a number that is not negative, got {scan_effects_min_lod}')
    drop = None
    if scan_lod_drop is not None:
        drop = float(scan_lod_drop)
        if not (drop >= 0.0 and np.isfinite(drop)):
            raise RuntimeError(f'--scan-lod-drop must be a finite number that is not negative, got {scan_lod_drop}')
    if min_lod is None and drop is None:
        return None
    return {'min_lod': min_lod, 'lod_drop': drop}


def kinship_options(scan_kinship=None, scan_kinship_out=False, scan_perms=None, scan_snps=False, scan_mediate=False,
                    scan_effects=False, scan_lod_drop=None):
    """`--scan-kinship loco|overall [--scan-kinship-out]` as one dict, or None without `--scan-kinship`;
    `--scan-kinship-out` alone is refused.  The passes that work on the unweighted W are refused next to the mixed model,
    one line each.  Refused before a file is read."""
    if scan_kinship is None:
        if scan_kinship_out:
            raise RuntimeError('--scan-kinship-out needs --scan-kinship')
        return None
    if scan_kinship not in KINSHIP_MODES:
        raise RuntimeError(f'--scan-kinship must be one of {", ".join(KINSHIP_MODES)}, got {scan_kinship}')
    for name, value in (('--scan-perms', scan_perms), ('--scan-snps', scan_snps or None), ('--scan-mediate', scan_mediate or None),
                        ('--scan-effects', scan_effects or None), ('--scan-lod-drop', scan_lod_drop)):
        if value is not None:
            raise RuntimeError(f'{name} cannot be combined with --scan-kinship: its pass uses the unweighted scan')
    return {'mode': scan_kinship, 'out': bool(scan_kinship_out)}


def kinship_snp_options(scan_kinship_snps=None, scan_kinship=None):
    """`--scan-kinship-snps FILE` needs `--scan-kinship`.  Refused before a file is read."""
    if scan_kinship_snps is not None and scan_kinship is None:
        raise RuntimeError('--scan-kinship-snps needs --scan-kinship: without a kinship the SNP pass is --scan-snps')
    return scan_kinship_snps


def kinship_effects_options(scan_kinship_effects=False, scan_kinship_effects_min_lod=None, scan_kinship_lod_drop=None,
                            scan_kinship=None):
    """`--scan-kinship-effects [--scan-kinship-effects-min-lod X]` and `--scan-kinship-lod-drop X` as one
    dict `{'min_lod': X or None without --scan-kinship-effects, 'lod_drop': X or None}`, or None with neither.  Both need
    `--scan-kinship`; `--scan-kinship-effects-min-lod` alone is refused.  Refused before a file is read."""
    if scan_kinship is None:
        for name, value in (('--scan-kinship-effects', scan_kinship_effects or None),
                            ('--scan-kinship-effects-min-lod', scan_kinship_effects_min_lod),
                            ('--scan-kinship-lod-drop', scan_kinship_lod_drop)):
            if value is not None:
                raise RuntimeError(f'{name} needs --scan-kinship: without a kinship the pass is {name.replace("-kinship", "")}')
    if not scan_kinship_effects and scan_kinship_effects_min_lod is not None:
        raise RuntimeError('--scan-kinship-effects-min-lod needs --scan-kinship-effects')
    min_lod = None
    if scan_kinship_effects:
        min_lod = DEFAULT_EFFECTS_MIN_LOD if scan_kinship_effects_min_lod is None else float(scan_kinship_effects_min_lod)
        if not (min_lod >= 0.0 and np.isfinite(min_lod)):
            raise RuntimeError(f'--scan-kinship-effects-min-lod must be a finite number that is not negative, got '
                               f'{scan_kinship_effects_min_lod}')
    drop = None
    if scan_kinship_lod_drop is not None:
        drop = float(scan_kinship_lod_drop)
        if not (drop >= 0.0 and np.isfinite(drop)):
            raise RuntimeError(f'--scan-kinship-lod-drop must be a finite number that is not negative, got {scan_kinship_lod_drop}')
    if min_lod is None and drop is None:
        return None
    return {'min_lod': min_lod, 'lod_drop': drop}


def intcovar_options(scan_intcovar=None, scan_covar=None, scan_kinship=None):
    """`--scan-intcovar NAME[,NAME...]` as the list of names, or None without it.  It needs `--scan-covar`
    (qtl2 adds intcovar to addcovar: an interactive covariate is a column of the covariate table), names no column twice
    and cannot stand beside `--scan-kinship`.  Refused before a file is read; whether the table has the names is
    intcovar_plan's question, asked as soon as the table's header is known."""
    if scan_intcovar is None:
        return None
    if scan_covar is None:
        raise RuntimeError('--scan-intcovar needs --scan-covar: the interactive covariates are columns of the covariate table')
    if scan_kinship is not None:
        raise RuntimeError('--scan-intcovar cannot be combined with --scan-kinship: the mixed model with interactions is not '
                           'part of the scan')
    names = [x.strip() for x in str(scan_intcovar).split(',')]
    if any(not x for x in names):
        raise RuntimeError(f'--scan-intcovar must be covariate names separated by commas, got {scan_intcovar!r}')
    for x in names:
        if names.count(x) > 1:
            raise RuntimeError(f'--scan-intcovar names {x} twice')
    return names


def intcovar_plan(intcovar, covar_names):
    """The columns of scan_design's Z (intercept first) that `intcovar` names among the covariate table's `covar_names`; a
    name the table does not have is refused before a dosage is read or the device runs."""
    for x in intcovar:
        if x not in covar_names:
            raise RuntimeError(f'--scan-intcovar: {x} is not a column of --scan-covar (its columns: {", ".join(covar_names)})')
    return [1 + list(covar_names).index(x) for x in intcovar]


def check_scan_args(scan_pheno=None, scan_covar=None, scan_rankz=False, scan_out=None, scan_min_lod=None,
                    scan_lod_matrix=False, grid_file=None, cohort=False, scan_perms=None, scan_perm_seed=None,
                    scan_perm_alpha=None, scan_perm_chromosomes=None, scan_perm_pheno=None, scan_mediate=False,
                    scan_mediate_min_lod=None, scan_mediate_top=None, scan_mediator_file=None, scan_effects=False,
                    scan_effects_min_lod=None, scan_lod_drop=None, scan_kinship=None, scan_kinship_out=False, scan_snps=False,
                    scan_kinship_snps=None, scan_kinship_effects=False, scan_kinship_effects_min_lod=None,
                    scan_kinship_lod_drop=None, scan_intcovar=None):
    """`--scan-pheno FILE [--scan-covar FILE] [--scan-rankz] [--scan-out PREFIX] [--scan-min-lod X] [--scan-lod-matrix]`,
    the `--scan-perm*` options (perm_options), the `--scan-mediat*` options (mediate_options), `--scan-effects`,
    `--scan-effects-min-lod`, `--scan-lod-drop` (effects_options) and `--scan-kinship`, `--scan-kinship-out`
    (kinship_options) with `--scan-kinship-snps` (kinship_snp_options), `--scan-kinship-effects`,
    `--scan-kinship-effects-min-lod` and `--scan-kinship-lod-drop` (kinship_effects_options) and `--scan-intcovar`
    (intcovar_options):
    every option needs the phenotypes, the phenotypes need `--grid-file` and a cohort (`--sample-file`): one sample
    cannot be scanned.  Refused before a file is read."""
    given = {'--scan-covar': scan_covar, '--scan-rankz': scan_rankz or None, '--scan-out': scan_out,
             '--scan-min-lod': scan_min_lod, '--scan-lod-matrix': scan_lod_matrix or None, '--scan-perms': scan_perms,
             '--scan-perm-seed': scan_perm_seed, '--scan-perm-alpha': scan_perm_alpha,
             '--scan-perm-chromosomes': scan_perm_chromosomes, '--scan-perm-pheno': scan_perm_pheno,
             '--scan-mediate': scan_mediate or None, '--scan-mediate-min-lod': scan_mediate_min_lod,
             '--scan-mediate-top': scan_mediate_top, '--scan-mediator-file': scan_mediator_file,
             '--scan-effects': scan_effects or None, '--scan-effects-min-lod': scan_effects_min_lod,
             '--scan-lod-drop': scan_lod_drop, '--scan-kinship': scan_kinship, '--scan-kinship-out': scan_kinship_out or None,
             '--scan-kinship-snps': scan_kinship_snps, '--scan-kinship-effects': scan_kinship_effects or None,
             '--scan-kinship-effects-min-lod': scan_kinship_effects_min_lod, '--scan-kinship-lod-drop': scan_kinship_lod_drop,
             '--scan-intcovar': scan_intcovar}
    perm_options(scan_perms, scan_perm_seed, scan_perm_alpha, scan_perm_chromosomes, scan_perm_pheno)
    mediate_options(scan_mediate, scan_mediate_min_lod, scan_mediate_top, scan_mediator_file)
    effects_options(scan_effects, scan_effects_min_lod, scan_lod_drop)
    kinship_options(scan_kinship, scan_kinship_out, scan_perms, scan_snps, scan_mediate, scan_effects, scan_lod_drop)
    kinship_snp_options(scan_kinship_snps, scan_kinship)
    kinship_effects_options(scan_kinship_effects, scan_kinship_effects_min_lod, scan_kinship_lod_drop, scan_kinship)
    intcovar_options(scan_intcovar, scan_covar, scan_kinship)
    if scan_pheno is None:
        for name, value in given.items():
            if value is not None:
                raise RuntimeError(f'{name} needs --scan-pheno')
        return
    if not cohort:
        raise RuntimeError('--scan-pheno needs --sample-file: one sample (-e) cannot be scanned')
    if grid_file is None:
        raise RuntimeError('--scan-pheno needs --grid-file')
    if scan_min_lod is not None and not scan_min_lod >= 0.0:
        raise RuntimeError('--scan-min-lod must be a number that is not negative')


def check_scan_snp_args(scan_snps=False, snp_file=None, scan_pheno=None, grid_file=None, cohort=False):
    """`--scan-snps` needs `--snp-file`, `--scan-pheno`, `--grid-file` and a cohort (`--sample-file`).  Refused before a
    file is read and before any device work."""
    if not scan_snps:
        return
    for name, value in (('--snp-file', snp_file), ('--scan-pheno', scan_pheno), ('--grid-file', grid_file),
                        ('--sample-file', cohort or None)):
        if value is None:
            raise RuntimeError(f'--scan-snps needs {name}')


def read_number_table(path, what):
    """(column names, {id: row of floats}) of a tab separated table with the header `id<TAB>name...`; blank and # lines
    after the header are skipped; an id given twice, a short row and a field that is no number are refused by line."""
    with open(path) as fh:
        header = fh.readline().rstrip('\n').split('\t')
        if len(header) < 2 or header[0] != 'id':
            raise RuntimeError(f'{path}: the header must be id<TAB>{what} name...')
        names = header[1:]
        if len(set(names)) != len(names):
            raise RuntimeError(f'{path}: a {what} is named twice in the header')
        rows, where = {}, {}
        for number, line in enumerate(fh, 2):
            line = line.rstrip('\n')
            if not line.strip() or line.startswith('#'):
                continue
            fields = line.split('\t')
            if len(fields) != len(header):
                raise RuntimeError(f'{path}, line {number}: {len(fields) - 1} values for {len(names)} {what}s')
            if fields[0] in rows:
                raise RuntimeError(f'{path}, line {number}: id {fields[0]} is already on line {where[fields[0]]}')
            try:
                rows[fields[0]] = np.array([float(x) for x in fields[1:]])
            except ValueError as e:
                raise RuntimeError(f'{path}, line {number}: {e}') from None
            where[fields[0]] = number
    return names, rows


def read_scan_pheno(path):
    """`--scan-pheno`: rows keyed by the sample's outbase, one column per phenotype."""
    return read_number_table(path, 'phenotype')


def read_scan_covar(path):
    """`--scan-covar`: rows keyed by the sample's outbase, one numeric column per covariate.  The intercept is not in
    the file: scan_design adds it."""
    return read_number_table(path, 'covariate')


def scan_design(ids, pheno, covar=None, use_rankz=False):
    """(kept positions in `ids`, Y [n, P], Z [n, c] with the intercept first, covariate names) for the ids that have a
    phenotype row and, with covariates, a covariate row; the others are logged and left out."""
    kept = []
    for k, i in enumerate(ids):
        if i not in pheno[1]:
            logger.warning(f'scan: {i} has no phenotype row and is left out')
        elif covar is not None and i not in covar[1]:
            logger.warning(f'scan: {i} has no covariate row and is left out')
        else:
            kept.append(k)
    P = len(pheno[0])
    y = np.array([pheno[1][ids[k]] for k in kept]).reshape(len(kept), P)
    if use_rankz:
        y = np.column_stack([rankz(y[:, p]) for p in range(P)]) if len(kept) else y
    names = ['intercept'] + (list(covar[0]) if covar is not None else [])
    z = np.ones((len(kept), len(names)))
    if covar is not None and kept:
        z[:, 1:] = np.array([covar[1][ids[k]] for k in kept])
    return kept, y, z, names


def write_scan(prefix, phenotypes, samples, covariates, chrom, pos, chrom_names, result, rank, min_lod=0.0, perm=None,
               lod_drop=None, kinship_mode=None):
    """`<prefix>.scan.npz` and `<prefix>.scan.peaks.tsv`.  chrom / pos: per grid point, in the scan's point order;
    chrom_names: the scan's chromosomes, as peak_lod's columns.  perm (with `--scan-perms`): `perm_max` [Pp, B] of the
    phenotypes `columns`, `alphas`, `seed` and `mask` over chrom_names; the .npz gains the perm_* arrays and the peaks
    file the columns `pvalue` and `threshold_<first level>`, NA where nothing was permuted.  Without it both files are
    what they were before the permutations existed.  lod_drop (with `--scan-lod-drop`; result then holds `support_lo`
    and `support_hi`): the .npz gains both and `lod_drop`, the peaks file the columns `support_lo` and `support_hi` - the
    positions of the interval's ends - after every other column.  kinship_mode (with `--scan-kinship`; result is
    GenomeScan.run_lmm's and rank is None): the .npz holds `hsq`, `sigma2`, `rank_min`, `rank_max` and `kinship_mode`
    instead of `rank`, and the peaks file gains the column `hsq`, the heritability the chromosome was scanned with; with
    lod_drop (`--scan-kinship-lod-drop`) the support columns follow `hsq`."""
    if kinship_mode is not None:
        write_scan_lmm(prefix, phenotypes, samples, covariates, chrom, pos, chrom_names, result, min_lod, kinship_mode, lod_drop)
        return
    arrays = dict(phenotypes=np.array(phenotypes), samples=np.array(samples), covariates=np.array(covariates),
                  chrom=np.array(chrom), pos=np.asarray(pos, dtype=np.float64), rank=np.asarray(rank),
                  peak_lod=result['peak_lod'], peak_index=result['peak_index'])
    if 'lod' in result:
        arrays['lod'] = result['lod']
    peak, index = result['peak_lod'], result['peak_index']
    if lod_drop is None:
        ends, ends_header = lambda p, c: '', ''
    else:
        arrays.update(support_lo=result['support_lo'], support_hi=result['support_hi'], lod_drop=np.float64(lod_drop))
        ends = lambda p, c: (f'\t{repr(float(pos[result["support_lo"][p, c]]))}'
                             f'\t{repr(float(pos[result["support_hi"][p, c]]))}')
        ends_header = '\tsupport_lo\tsupport_hi'
    if perm is not None:
        write_scan_perm(prefix, phenotypes, pos, chrom_names, peak, index, min_lod, perm, arrays, ends, ends_header)
        return
    np.savez(f'{prefix}.scan.npz', **arrays)
    with open(f'{prefix}.scan.peaks.tsv', 'w') as out:
        out.write(f'#phenotype\tchromosome\tposition\tlod\tgenome_wide_max{ends_header}\n')
        for p, name in enumerate(phenotypes):
            on = [c for c in range(len(chrom_names)) if index[p, c] >= 0]
            top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
            for c in on:
                if peak[p, c] >= min_lod:
                    out.write(f'{name}\t{chrom_names[c]}\t{repr(float(pos[index[p, c]]))}\t{repr(float(peak[p, c]))}\t'
                              f'{int(c == top)}{ends(p, c)}\n')


def write_scan_lmm(prefix, phenotypes, samples, covariates, chrom, pos, chrom_names, result, min_lod, kinship_mode,
                   lod_drop=None):
    """write_scan's two files for the mixed model.  lod_drop (result then holds `support_lo` and `support_hi`): the .npz
    gains both and `lod_drop`, the peaks file the columns `support_lo` and `support_hi` (positions) after `hsq`."""
    arrays = dict(phenotypes=np.array(phenotypes), samples=np.array(samples), covariates=np.array(covariates),
                  chrom=np.array(chrom), pos=np.asarray(pos, dtype=np.float64), peak_lod=result['peak_lod'],
                  peak_index=result['peak_index'], hsq=result['hsq'], sigma2=result['sigma2'], rank_min=result['rank_min'],
                  rank_max=result['rank_max'], kinship_mode=np.array(kinship_mode))
    if 'lod' in result:
        arrays['lod'] = result['lod']
    if lod_drop is None:
        ends, ends_header = lambda p, c: '', ''
    else:
        arrays.update(support_lo=result['support_lo'], support_hi=result['support_hi'], lod_drop=np.float64(lod_drop))
        ends = lambda p, c: (f'\t{repr(float(pos[result["support_lo"][p, c]]))}'
                             f'\t{repr(float(pos[result["support_hi"][p, c]]))}')
        ends_header = '\tsupport_lo\tsupport_hi'
    np.savez(f'{prefix}.scan.npz', **arrays)
    peak, index, hsq = result['peak_lod'], result['peak_index'], result['hsq']
    with open(f'{prefix}.scan.peaks.tsv', 'w') as out:
        out.write(f'#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\thsq{ends_header}\n')
        for p, name in enumerate(phenotypes):
            on = [c for c in range(len(chrom_names)) if index[p, c] >= 0]
            top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
            for c in on:
                if peak[p, c] >= min_lod:
                    out.write(f'{name}\t{chrom_names[c]}\t{repr(float(pos[index[p, c]]))}\t{repr(float(peak[p, c]))}\t'
                              f'{int(c == top)}\t{repr(float(hsq[p, c]))}{ends(p, c)}\n')


def write_scan_kinship(prefix, samples, chrom_names, matrices, eig_of_chrom, kinship_mode):
    """`<prefix>.scan.kinship.npz` (`--scan-kinship-out`): `kinship` [k, n, n], the matrix of each chromosome
    (`kinship_of_chromosome`, over `chromosomes`), the sample ids and the mode."""
    np.savez(f'{prefix}.scan.kinship.npz', kinship=np.stack(matrices), kinship_of_chromosome=np.asarray(eig_of_chrom, dtype=np.int32),
             chromosomes=np.array([str(c) for c in chrom_names]), samples=np.array(samples), kinship_mode=np.array(kinship_mode))


def write_scan_perm(prefix, phenotypes, pos, chrom_names, peak, index, min_lod, perm, arrays, ends=lambda p, c: '',
                    ends_header=''):
    """write_scan's two files with the permutation results in them; ends / ends_header: write_scan's support columns."""
    columns, mask, alphas = list(perm['columns']), np.asarray(perm['mask'], dtype=bool), list(perm['alphas'])
    threshold = perm_thresholds(perm['perm_max'], alphas)
    pvalue = perm_pvalues(perm['perm_max'], peak[columns], selected=mask)
    arrays.update(perm_max=perm['perm_max'], perm_phenotypes=np.array([phenotypes[p] for p in columns]),
                  perm_alpha=np.array(alphas), perm_threshold=threshold, perm_seed=np.uint64(perm['seed']),
                  perm_chromosomes=np.array([str(c) for c, on in zip(chrom_names, mask) if on]))
    np.savez(f'{prefix}.scan.npz', **arrays)
    row_of = {p: k for k, p in enumerate(columns)}
    with open(f'{prefix}.scan.peaks.tsv', 'w') as out:
        out.write(f'#phenotype\tchromosome\tposition\tlod\tgenome_wide_max\tpvalue\tthreshold_{repr(float(alphas[0]))}'
                  f'{ends_header}\n')
        for p, name in enumerate(phenotypes):
            on = [c for c in range(len(chrom_names)) if index[p, c] >= 0]
            top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
            for c in on:
                if peak[p, c] >= min_lod:
                    judged = p in row_of and mask[c]
                    out.write(f'{name}\t{chrom_names[c]}\t{repr(float(pos[index[p, c]]))}\t{repr(float(peak[p, c]))}\t'
                              f'{int(c == top)}\t{repr(float(pvalue[row_of[p], c])) if judged else "NA"}\t'
                              f'{repr(float(threshold[row_of[p], 0])) if judged else "NA"}{ends(p, c)}\n')


def snp_plan(snps, chrom_names, points, grid):
    """The SNPs of read_snp_file's dict (read with `chrom_names` as its chromosomes) as GenomeScan.set_snps takes them:
    (grid positions, SNP positions, patterns - each per chromosome of the scan -, file rows in handle order).  grid:
    {chromosome: positions}.  The cM column is in the grid's position units.  A chromosome of the scan without grid
    points takes no SNPs: its SNPs, like those of chromosomes the scan does not have, stay out of the handle."""
    grid_pos, snp_pos, masks, rows = [], [], [], []
    pointless = 0
    for c, k in zip(chrom_names, points):
        by = snps['by_chrom'][c]
        if k == 0:
            pointless += len(by)
            by = by[:0]
        grid_pos.append(np.asarray(grid[c], dtype=np.float64) if k else np.zeros(0))
        snp_pos.append(snps['cM'][by])
        masks.append(snps['mask'][by])
        rows.append(by)
    if pointless:
        logger.warning(f'scan: {pointless} SNPs on chromosomes without grid points are not tested')
    return grid_pos, snp_pos, masks, np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)


def snps_in_file_order(result, rows, n_file):
    """GenomeScan.run_snps' dict (handle order) in the SNP file's order: `used` [n_file] (False for SNPs that are not on
    the handle), `peak_lod`, `peak_snp` [P, n_chrom] (the SNP's file row, -1 without a used SNP) and, if present, `lod`
    [P, n_file], NaN for the SNPs that are not on the handle."""
    used = np.zeros(n_file, dtype=bool)
    used[rows] = result['used']
    index = result['peak_index']
    out = {'used': used, 'peak_lod': result['peak_lod'],
           'peak_snp': np.where(index >= 0, rows[np.maximum(index, 0)] if len(rows) else -1, -1).astype(np.int64)}
    if 'lod' in result:
        out['lod'] = np.full((len(result['lod']), n_file), np.nan)
        out['lod'][:, rows] = result['lod']
    return out


def write_scan_snps(prefix, phenotypes, samples, covariates, snps, chrom_names, result, min_lod=0.0):
    """`<prefix>.scan.snps.npz` and `<prefix>.scan.snps.peaks.tsv` from snps_in_file_order's dict: everything per SNP in
    the SNP file's order; one peaks line per (phenotype, chromosome of the scan) whose peak reaches min_lod."""
    arrays = dict(phenotypes=np.array(phenotypes), samples=np.array(samples), covariates=np.array(covariates),
                  snp_id=snps['snp_id'], chrom=snps['chrom'], bp=snps['bp'], cM=snps['cM'], pattern=snps['pattern'],
                  used=result['used'], peak_lod=result['peak_lod'], peak_snp=result['peak_snp'])
    if 'lod' in result:
        arrays['lod'] = result['lod']
    np.savez(f'{prefix}.scan.snps.npz', **arrays)
    peak, at = result['peak_lod'], result['peak_snp']
    with open(f'{prefix}.scan.snps.peaks.tsv', 'w') as out:
        out.write('#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max\n')
        for p, name in enumerate(phenotypes):
            on = [c for c in range(len(chrom_names)) if at[p, c] >= 0]
            top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
            for c in on:
                if peak[p, c] >= min_lod:
                    j = at[p, c]
                    out.write(f'{name}\t{chrom_names[c]}\t{snps["snp_id"][j]}\t{repr(float(snps["bp"][j]))}\t'
                              f'{repr(float(snps["cM"][j]))}\t{snps["pattern"][j]}\t{repr(float(peak[p, c]))}\t{int(c == top)}\n')


def finish_scan_snps(scan, prefix, ids, phenotypes, covariates, y, snps, chrom_names, grid, min_lod=None, lod_matrix=False,
                     stage_times=None):
    """The SNP association pass on the prepared cohort `scan` holds and its two files.  y: the
    phenotypes as the scan saw them (after `--scan-rankz`).  Its wall-clock seconds go to stage_times['scan_snps']."""
    import time
    t0 = time.perf_counter()
    grid_pos, snp_pos, masks, rows = snp_plan(snps, chrom_names, scan.points, grid)
    n_file = len(snps['snp_id'])
    if len(rows):
        scan.set_snps(grid_pos, snp_pos, masks)
        got = scan.run_snps(y, want_lod=bool(lod_matrix) or y.shape[1] * len(rows) <= LOD_MATRIX_LIMIT)
        timing = scan.snp_info()
        logger.info(f'scan: {len(rows)} SNPs, {y.shape[1]} phenotypes; {timing["pass_ms"]:.1f} ms on the device, '
                    f'{timing["row_ms"]:.1f} ms of them in the row kernel and {timing["product_ms"]:.1f} ms in the product kernel')
    else:
        logger.warning('scan: no SNP of the file lies on a chromosome with grid points')
        nc = len(chrom_names)
        got = {'used': np.zeros(0, dtype=bool), 'peak_lod': np.full((y.shape[1], nc), np.nan),
               'peak_index': np.full((y.shape[1], nc), -1, dtype=np.int64), 'lod': np.zeros((y.shape[1], 0))}
    write_scan_snps(prefix, phenotypes, ids, covariates, snps, [str(c) for c in chrom_names],
                    snps_in_file_order(got, rows, n_file), 0.0 if min_lod is None else min_lod)
    if stage_times is not None:
        stage_times['scan_snps'] = stage_times.get('scan_snps', 0.0) + time.perf_counter() - t0


def snps_lmm_in_file_order(result, rows, n_file):
    """GenomeScan.run_snps_lmm's dict (handle order) in the SNP file's order: `peak_lod`, `peak_snp` (the SNP's file row,
    -1 without a used SNP), `n_used`, `hsq` [P, n_chrom] and, if present, `lod` [P, n_file] (NaN for the SNPs that are not
    on the handle) with `used` [P, n_file] (False for those) beside it."""
    index = result['peak_index']
    out = {'peak_lod': result['peak_lod'], 'n_used': result['n_used'], 'hsq': result['hsq'],
           'peak_snp': np.where(index >= 0, rows[np.maximum(index, 0)] if len(rows) else -1, -1).astype(np.int64)}
    if 'lod' in result:
        P = len(result['lod'])
        out['lod'], out['used'] = np.full((P, n_file), np.nan), np.zeros((P, n_file), dtype=bool)
        out['lod'][:, rows] = result['lod']
        out['used'][:, rows] = result['used']
    return out


def write_scan_snps_lmm(prefix, phenotypes, samples, covariates, snps, chrom_names, result, min_lod, kinship_mode):
    """`<prefix>.scan.snps.npz` and `<prefix>.scan.snps.peaks.tsv` of the SNP pass under the mixed model
    from snps_lmm_in_file_order's dict: write_scan_snps' members plus `hsq`, `n_used` and `kinship_mode`; `used` depends
    on the phenotype here and goes in only beside the LOD matrix; the peaks file gains the column hsq."""
    arrays = dict(phenotypes=np.array(phenotypes), samples=np.array(samples), covariates=np.array(covariates),
                  snp_id=snps['snp_id'], chrom=snps['chrom'], bp=snps['bp'], cM=snps['cM'], pattern=snps['pattern'],
                  peak_lod=result['peak_lod'], peak_snp=result['peak_snp'], hsq=result['hsq'], n_used=result['n_used'],
                  kinship_mode=np.array(kinship_mode))
    if 'lod' in result:
        arrays['lod'], arrays['used'] = result['lod'], result['used']
    np.savez(f'{prefix}.scan.snps.npz', **arrays)
    peak, at, hsq = result['peak_lod'], result['peak_snp'], result['hsq']
    with open(f'{prefix}.scan.snps.peaks.tsv', 'w') as out:
        out.write('#phenotype\tchromosome\tsnp_id\tbp\tcM\tpattern\tlod\tgenome_wide_max\thsq\n')
        for p, name in enumerate(phenotypes):
            on = [c for c in range(len(chrom_names)) if at[p, c] >= 0]
            top = max(on, key=lambda c: (peak[p, c], -c)) if on else None
            for c in on:
                if peak[p, c] >= min_lod:
                    j = at[p, c]
                    out.write(f'{name}\t{chrom_names[c]}\t{snps["snp_id"][j]}\t{repr(float(snps["bp"][j]))}\t'
                              f'{repr(float(snps["cM"][j]))}\t{snps["pattern"][j]}\t{repr(float(peak[p, c]))}\t{int(c == top)}\t'
                              f'{repr(float(hsq[p, c]))}\n')


def finish_scan_snps_lmm(scan, prefix, ids, phenotypes, covariates, y, snps, chrom_names, grid, hsq, kinship_mode, min_lod=None,
                         lod_matrix=False, stage_times=None):
    """The SNP association pass under the mixed model `scan` holds and its two files.  y: the phenotypes
    as the scan saw them; hsq: [P, n_chrom], what the grid scan fitted, so that both passes use the same heritability per
    chromosome.  Its wall-clock seconds go to stage_times['scan_snps']."""
    import time
    t0 = time.perf_counter()
    grid_pos, snp_pos, masks, rows = snp_plan(snps, chrom_names, scan.points, grid)
    n_file, nc = len(snps['snp_id']), len(chrom_names)
    if len(rows):
        scan.set_snps(grid_pos, snp_pos, masks)
        got = scan.run_snps_lmm(y, want_lod=bool(lod_matrix) or y.shape[1] * len(rows) <= LOD_MATRIX_LIMIT, hsq=hsq)
        timing = scan.lmm_snp_info()
        logger.info(f'scan: {len(rows)} SNPs, {y.shape[1]} phenotypes under the mixed model; {timing["pass_ms"]:.1f} ms on the '
                    f'device, null fits {timing["null_ms"]:.1f} ms, dosages and rotation {timing["rotate_ms"]:.1f} ms, product '
                    f'kernel {timing["product_ms"]:.1f} ms')
    else:
        logger.warning('scan: no SNP of the file lies on a chromosome with grid points')
        P = y.shape[1]
        got = {'peak_lod': np.full((P, nc), np.nan), 'peak_index': np.full((P, nc), -1, dtype=np.int64),
               'n_used': np.zeros((P, nc), dtype=np.int64), 'hsq': np.asarray(hsq, dtype=np.float64), 'lod': np.zeros((P, 0)),
               'used': np.zeros((P, 0), dtype=bool)}
    write_scan_snps_lmm(prefix, phenotypes, ids, covariates, snps, [str(c) for c in chrom_names],
                        snps_lmm_in_file_order(got, rows, n_file), 0.0 if min_lod is None else min_lod, kinship_mode)
    if stage_times is not None:
        stage_times['scan_snps'] = stage_times.get('scan_snps', 0.0) + time.perf_counter() - t0


def mediation_targets(peak_lod, peak_index, min_lod):
    """(phenotype, chromosome) of every peak of the scan with a LOD of at least min_lod, phenotype after phenotype: [T, 2]."""
    with np.errstate(invalid='ignore'):
        on = (np.asarray(peak_index) >= 0) & (np.asarray(peak_lod) >= min_lod)
    return np.argwhere(on).astype(np.int64).reshape(-1, 2)


def write_scan_mediation(prefix, phenotypes, mediators, samples, covariates, chrom_names, pos, targets, points, result,
                         min_lod):
    """`<prefix>.scan.mediation.npz` and `<prefix>.scan.mediation.tsv` from GenomeScan.mediate's dict.  targets: [T, 2]
    (phenotype, chromosome) indices, points: [T] grid points.  One line per (target, rank) whose place is filled; drop is
    lod - lod_mediated and z is (lod_mediated - mean) / sd over the target's used mediators, NA without a spread."""
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
    arrays = dict(phenotypes=np.array(phenotypes), mediators=np.array(mediators), samples=np.array(samples),
                  covariates=np.array(covariates), targets=np.array([phenotypes[p] for p in targets[:, 0]], dtype=np.str_),
                  target_phenotype=targets[:, 0], target_chromosome=np.array([chrom_names[c] for c in targets[:, 1]], dtype=np.str_),
                  points=np.asarray(points, dtype=np.int64), position=np.asarray(pos, dtype=np.float64)[np.asarray(points, dtype=np.int64)],
                  min_lod=np.float64(min_lod))
    for key in ('lod0', 'best_index', 'best_lod', 'mean', 'sd', 'n_used', 'lod_med', 'used'):
        if key in result:
            arrays[key] = result[key]
    np.savez(f'{prefix}.scan.mediation.npz', **arrays)
    with open(f'{prefix}.scan.mediation.tsv', 'w') as out:
        out.write('#phenotype\tchromosome\tposition\tlod\tmediator\tlod_mediated\tdrop\tz\n')
        for t, (p, c) in enumerate(targets):
            lod0, mean, sd = float(result['lod0'][t]), float(result['mean'][t]), float(result['sd'][t])
            for q, v in zip(result['best_index'][t], result['best_lod'][t]):
                if q < 0:
                    break
                v = float(v)
                z = repr((v - mean) / sd) if sd > 0.0 else 'NA'
                out.write(f'{phenotypes[p]}\t{chrom_names[c]}\t{repr(float(arrays["position"][t]))}\t{repr(lod0)}\t{mediators[q]}\t'
                          f'{repr(v)}\t{repr(lod0 - v)}\t{z}\n')


def mediator_table(mediate, ids, pheno, y, use_rankz):
    """(names, values [n, Q]) of the mediators: the phenotypes as the scan saw them, or the table of `--scan-mediator-file`
    (mediate['table'] when it was read before, else read here) with `--scan-rankz` applied like the phenotypes'.  Every
    sample of the scan needs a row."""
    if mediate.get('mediator_file') is None:
        return list(pheno[0]), y
    table = mediate['table'] if mediate.get('table') is not None else read_scan_pheno(mediate['mediator_file'])
    missing = [i for i in ids if i not in table[1]]
    if missing:
        raise RuntimeError(f'{mediate["mediator_file"]}: {missing[0]} has no row: the mediators need the ids of the phenotypes')
    return list(table[0]), scan_design(ids, table, None, use_rankz)[1]


def finish_scan_mediation(scan, prefix, ids, pheno, covariates, y, mediate, result, chrom_names, pos, lod_matrix=False,
                          stage_times=None):
    """The mediation pass on the prepared cohort `scan` holds and its two files.  y: the phenotypes as the
    scan saw them; result: GenomeScan.run's dict, whose peaks of at least mediate['min_lod'] are the targets.  Its
    wall-clock seconds go to stage_times['mediate']."""
    import time
    t0 = time.perf_counter()
    names, z = mediator_table(mediate, ids, pheno, y, mediate.get('rankz', False))
    targets = mediation_targets(result['peak_lod'], result['peak_index'], mediate['min_lod'])
    points = result['peak_index'][targets[:, 0], targets[:, 1]]
    T, Q, K = len(targets), len(names), mediate['top']
    want_lod = bool(lod_matrix) or T * Q <= LOD_MATRIX_LIMIT
    if T:
        got = scan.mediate(y[:, targets[:, 0]], points, z, top=K, want_lod=want_lod)
        timing = scan.mediate_info()
        logger.info(f'scan: {T} peaks mediated by {Q} mediators; {timing["pass_ms"]:.1f} ms on the device, '
                    f'{timing["product_ms"]:.1f} ms of them in the product kernel')
    else:
        logger.warning(f'scan: no peak reaches a LOD of {mediate["min_lod"]}: nothing to mediate')
        got = {'lod0': np.zeros(0), 'n_used': np.zeros(0, dtype=np.int64), 'mean': np.zeros(0), 'sd': np.zeros(0),
               'best_index': np.zeros((0, K), dtype=np.int64), 'best_lod': np.zeros((0, K)), 'lod_med': np.zeros((0, Q)),
               'used': np.zeros((0, Q), dtype=bool)}
    write_scan_mediation(prefix, pheno[0], names, ids, covariates, [str(c) for c in chrom_names], pos, targets, points, got,
                         mediate['min_lod'])
    if stage_times is not None:
        stage_times['mediate'] = stage_times.get('mediate', 0.0) + time.perf_counter() - t0


def write_scan_effects(prefix, phenotypes, founders, samples, covariates, chrom_names, pos, targets, points, result, min_lod,
                       kinship_mode=None):
    """`<prefix>.scan.effects.npz` and `<prefix>.scan.effects.tsv` from GenomeScan.effects' dict.  targets: [T, 2]
    (phenotype, chromosome) indices, points: [T] grid points, founders: the H labels.  One line per peak: phenotype,
    chromosome, position, lod, rank, then effect_<founder> and se_<founder> per founder.  kinship_mode (with
    `--scan-kinship-effects`; result is GenomeScan.effects_lmm's): the .npz gains `hsq` and `kinship_mode`, the table the
    column `hsq` after `rank`."""
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
    points = np.asarray(points, dtype=np.int64)
    founders = [str(f) for f in founders]
    arrays = dict(phenotypes=np.array(phenotypes), founders=np.array(founders, dtype=np.str_), samples=np.array(samples),
                  covariates=np.array(covariates), targets=np.array([phenotypes[p] for p in targets[:, 0]], dtype=np.str_),
                  target_phenotype=targets[:, 0], target_chromosome=np.array([chrom_names[c] for c in targets[:, 1]], dtype=np.str_),
                  points=points, position=np.asarray(pos, dtype=np.float64)[points], min_lod=np.float64(min_lod))
    for key in ('effect', 'se', 'lod', 'sigma2', 'rank'):
        arrays[key] = result[key]
    mixed = kinship_mode is not None
    if mixed:
        arrays.update(hsq=result['hsq'], kinship_mode=np.array(kinship_mode))
    np.savez(f'{prefix}.scan.effects.npz', **arrays)
    with open(f'{prefix}.scan.effects.tsv', 'w') as out:
        out.write('#phenotype\tchromosome\tposition\tlod\trank' + ('\thsq' if mixed else '') +
                  ''.join(f'\teffect_{f}\tse_{f}' for f in founders) + '\n')
        for t, (p, c) in enumerate(targets):
            out.write(f'{phenotypes[p]}\t{chrom_names[c]}\t{repr(float(arrays["position"][t]))}\t{repr(float(result["lod"][t]))}\t'
                      f'{int(result["rank"][t])}' + (f'\t{repr(float(result["hsq"][t]))}' if mixed else '') +
                      ''.join(f'\t{repr(float(e))}\t{repr(float(s))}' for e, s in zip(result['effect'][t], result['se'][t])) + '\n')


def finish_scan_effects(scan, prefix, ids, pheno, covariates, y, min_lod, result, chrom_names, pos, founders=None,
                        stage_times=None):
    """The effects pass on the prepared cohort `scan` holds and its two files.  y: the phenotypes as the
    scan saw them; result: GenomeScan.run's dict, whose peaks of at least min_lod are the targets (mediation_targets);
    founders: their labels, the founder's index without them.  Its wall-clock seconds go to stage_times['effects']."""
    import time
    t0 = time.perf_counter()
    targets = mediation_targets(result['peak_lod'], result['peak_index'], min_lod)
    points = result['peak_index'][targets[:, 0], targets[:, 1]]
    T, H = len(targets), scan.H
    if T:
        got = scan.effects(y, targets[:, 0], points)
        logger.info(f'scan: founder effects at {T} peaks; {scan.effects_info()["pass_ms"]:.1f} ms on the device')
    else:
        logger.warning(f'scan: no peak reaches a LOD of {min_lod}: no founder effects')
        got = {'effect': np.zeros((0, H)), 'se': np.zeros((0, H)), 'lod': np.zeros(0), 'sigma2': np.zeros(0),
               'rank': np.zeros(0, dtype=np.int32)}
    write_scan_effects(prefix, pheno[0], list(range(H)) if founders is None else founders, ids, covariates,
                       [str(c) for c in chrom_names], pos, targets, points, got, min_lod)
    if stage_times is not None:
        stage_times['effects'] = stage_times.get('effects', 0.0) + time.perf_counter() - t0


def finish_scan_effects_lmm(scan, prefix, ids, pheno, covariates, y, min_lod, result, chrom_names, pos, kinship_mode,
                            founders=None, stage_times=None):
    """The effects pass under the mixed model `scan` holds and its two files.  y: the phenotypes as the
    scan saw them; result: GenomeScan.run_lmm's dict, whose peaks of at least min_lod are the targets
    (mediation_targets) and whose heritabilities the pass is given.  Its wall-clock seconds go to stage_times['effects']."""
    import time
    t0 = time.perf_counter()
    targets = mediation_targets(result['peak_lod'], result['peak_index'], min_lod)
    points = result['peak_index'][targets[:, 0], targets[:, 1]]
    T, H = len(targets), scan.H
    if T:
        got = scan.effects_lmm(y, targets[:, 0], points, hsq=result['hsq'])
        timing = scan.lmm_effects_info()
        logger.info(f'scan: founder effects under the mixed model at {T} peaks of {timing["columns"]} phenotypes; '
                    f'{timing["pass_ms"]:.1f} ms on the device, {timing["null_ms"]:.1f} ms of them in the null fits')
    else:
        logger.warning(f'scan: no peak reaches a LOD of {min_lod}: no founder effects')
        got = {'effect': np.zeros((0, H)), 'se': np.zeros((0, H)), 'lod': np.zeros(0), 'sigma2': np.zeros(0),
               'hsq': np.zeros(0), 'rank': np.zeros(0, dtype=np.int32)}
    write_scan_effects(prefix, pheno[0], list(range(H)) if founders is None else founders, ids, covariates,
                       [str(c) for c in chrom_names], pos, targets, points, got, min_lod, kinship_mode=kinship_mode)
    if stage_times is not None:
        stage_times['effects'] = stage_times.get('effects', 0.0) + time.perf_counter() - t0


def write_scan_int(prefix, phenotypes, samples, covariates, intcovar, chrom, pos, chrom_names, result, rank_full, rank_add,
                   min_lod=0.0):
    """`<prefix>.scan.int.npz` and `<prefix>.scan.int.peaks.tsv`.  result: GenomeScan.run_int's dict and
    `peak_full_int` [P, n_chrom], lod_int at the full model's peak.  The .npz holds the names, chrom / pos per grid point,
    `rank_full` and `rank_add`, the five peak arrays and, where result has them, `lod_full`, `lod_add` and `lod_int`.  The
    peaks file has one line per full-model peak of at least min_lod: the peak's position, `lod_full`, `lod_add` and
    `lod_int` at it, the degrees of freedom of the two models there (the kept columns) and the chromosome's own
    interaction peak, its position and LOD."""
    arrays = dict(phenotypes=np.array(phenotypes), samples=np.array(samples), covariates=np.array(covariates),
                  intcovar=np.array(intcovar), chrom=np.array(chrom), pos=np.asarray(pos, dtype=np.float64),
                  rank_full=np.asarray(rank_full), rank_add=np.asarray(rank_add))
    for key in ('peak_full', 'peak_full_index', 'peak_full_add', 'peak_int', 'peak_int_index', 'lod_full', 'lod_add', 'lod_int'):
        if key in result:
            arrays[key] = result[key]
    np.savez(f'{prefix}.scan.int.npz', **arrays)
    peak, index, at_int = result['peak_full'], result['peak_full_index'], result['peak_full_int']
    number = lambda v: repr(float(v))
    with open(f'{prefix}.scan.int.peaks.tsv', 'w') as out:
        out.write('#phenotype\tchromosome\tposition\tlod_full\tlod_add\tlod_int\tdf_full\tdf_add\tint_peak_position\tint_peak_lod\n')
        for p, name in enumerate(phenotypes):
            for c in range(len(chrom_names)):
                if index[p, c] >= 0 and peak[p, c] >= min_lod:
                    m = index[p, c]
                    out.write(f'{name}\t{chrom_names[c]}\t{number(pos[m])}\t{number(peak[p, c])}\t'
                              f'{number(result["peak_full_add"][p, c])}\t{number(at_int[p, c])}\t{int(rank_full[m])}\t'
                              f'{int(rank_add[m])}\t{number(pos[result["peak_int_index"][p, c]])}\t'
                              f'{number(result["peak_int"][p, c])}\n')


def finish_scan_int(scan, prefix, ids, phenotypes, covariates, z, interactive, y, chrom, pos, chrom_names, min_lod=None,
                    lod_matrix=False):
    """prepare_int + run_int + write_scan_int for the cohort `scan` holds.  The three matrices go to the
    .npz under write_scan's rule (`--scan-lod-matrix`, or P x M up to LOD_MATRIX_LIMIT); without them the phenotypes pass
    in blocks of columns whose matrices are dropped once lod_int at the full model's peaks is read from them - a phenotype's
    numbers are the same bits in any block."""
    scan.prepare_int(z, interactive, covariates)
    P, nc = y.shape[1], len(chrom_names)
    want_lod = bool(lod_matrix) or P * scan.M <= LOD_MATRIX_LIMIT
    block = P if want_lod else max(1, LOD_MATRIX_LIMIT // scan.M)
    parts = []
    for p0 in range(0, P, block):
        got = scan.run_int(y[:, p0:p0 + block])
        rows, at = np.arange(got['lod_int'].shape[0])[:, None], got['peak_full_index']
        got['peak_full_int'] = np.where(at >= 0, got['lod_int'][rows, np.maximum(at, 0)], np.nan)
        if not want_lod:
            for key in ('lod_full', 'lod_add', 'lod_int'):
                del got[key]
        parts.append(got)
    result = {key: np.concatenate([g[key] for g in parts]) for key in parts[0]}
    info = scan.int_info()
    write_scan_int(prefix, phenotypes, ids, covariates, [covariates[j] for j in interactive], chrom, pos, chrom_names, result,
                   info['rank_full'], info['rank_add'], 0.0 if min_lod is None else min_lod)
    logger.info(f'scan: {len(interactive)} interactive covariates ({", ".join(covariates[j] for j in interactive)}), '
                f'{info["HPI"]} rows per grid point; prepare {info["prepare_ms"]:.1f} ms, run {info["run_ms"]:.1f} ms on the device')


def finish_scan(scan, prefix, ids, pheno, covar, use_rankz, chrom, pos, chrom_names, min_lod=None, lod_matrix=False,
                perm=None, stage_times=None, snps=None, snp_grid=None, mediate=None, effects=None, founders=None, kinship=None,
                kinship_snps=None, kinship_effects=None, intcovar=None):
    """prepare + run + the two files for the cohort `scan` holds, whose samples are `ids` in append order (every one with
    its rows in the tables).  perm: perm_options' dict, or None; with it the permutation pass runs after the scan on the
    phenotypes and chromosomes it names and its wall-clock seconds go to stage_times['scan_perm'].  mediate:
    mediate_options' dict, or None; with it the scan's peaks are mediated after everything else (finish_scan_mediation).
    effects: effects_options' dict, or None; its lod_drop makes the run form the support intervals, its min_lod makes
    the founder effects of the peaks follow (finish_scan_effects), named by `founders`.
    kinship: kinship_options' dict, or None; with it the scan is the mixed model's and none of the other
    passes runs, except that of kinship_snps (read_snp_file's dict of `--scan-kinship-snps`, or None): the SNP association
    under the same mixed model, at the heritabilities the scan fitted, and those of kinship_effects
    (kinship_effects_options' dict, or None): its lod_drop makes the run form the support intervals, its min_lod makes the
    founder effects of the peaks follow under the same mixed model and heritabilities.
    intcovar: intcovar_options' list of names, or None; with it the scan with those interactive covariates follows every
    other pass on a preparation of its own (finish_scan_int) and the other files are what they were.
    Returns GenomeScan.info() after the run."""
    kept, y, z, names = scan_design(ids, pheno, covar, use_rankz)
    assert len(kept) == len(ids) == scan.n
    if kinship is not None:
        matrices = scan.prepare_lmm(z, kinship['mode'], names)
        lod_drop = kinship_effects['lod_drop'] if kinship_effects is not None else None
        want_lod = bool(lod_matrix) or y.shape[1] * scan.M <= LOD_MATRIX_LIMIT
        result = scan.run_lmm(y, want_lod=want_lod, lod_drop=lod_drop)
        write_scan(prefix, pheno[0], ids, names, chrom, pos, chrom_names, result, None, 0.0 if min_lod is None else min_lod,
                   lod_drop=lod_drop, kinship_mode=kinship['mode'])
        if kinship['out']:
            write_scan_kinship(prefix, ids, chrom_names, matrices, scan.eig_of_chrom, kinship['mode'])
        if kinship_snps is not None:        # read_snp_file's dict: the SNP pass under the same kinship and heritabilities
            finish_scan_snps_lmm(scan, prefix, ids, pheno[0], names, y, kinship_snps, chrom_names, snp_grid, result['hsq'],
                                 kinship['mode'], min_lod, lod_matrix, stage_times)
        if kinship_effects is not None and kinship_effects['min_lod'] is not None:
            finish_scan_effects_lmm(scan, prefix, ids, pheno, names, y, kinship_effects['min_lod'], result, chrom_names, pos,
                                    kinship['mode'], founders, stage_times)
        timing = scan.lmm_info()
        logger.info(f'scan: {len(ids)} samples, {y.shape[1]} phenotypes, {scan.M} grid points under the mixed model '
                    f'({kinship["mode"]} kinship); kinship {timing["kinship_ms"]:.1f} ms, rotation {timing["rotate_ms"]:.1f} ms, '
                    f'null fits {timing["null_ms"]:.1f} ms, weighted scan {timing["point_ms"]:.1f} ms on the device')
        return scan.info()
    if perm is not None:
        columns, mask = perm_plan(perm, pheno[0], [str(c) for c in chrom_names])     # refused before the device runs
    if intcovar is not None:
        interactive = intcovar_plan(intcovar, names[1:])                             # likewise
    scan.prepare(z, names)
    want_lod = bool(lod_matrix) or y.shape[1] * scan.M <= LOD_MATRIX_LIMIT
    lod_drop = effects['lod_drop'] if effects is not None else None
    result = scan.run(y, want_lod=want_lod, lod_drop=lod_drop)
    info = scan.info()
    done = None
    if perm is not None:
        import time
        t0 = time.perf_counter()
        got = scan.permute(y[:, columns], perm['n_perm'], seed=perm['seed'], chromosomes=mask)
        if stage_times is not None:
            stage_times['scan_perm'] = stage_times.get('scan_perm', 0.0) + time.perf_counter() - t0
        done = {'perm_max': got['perm_max'], 'columns': columns, 'mask': mask, 'alphas': perm['alphas'], 'seed': perm['seed']}
        timing = scan.perm_info()
        logger.info(f'scan: {perm["n_perm"]} permutations of {len(columns)} phenotypes; {timing["permute_ms"]:.1f} ms on the '
                    f'device, {timing["product_ms"]:.1f} ms of them in the product kernel')
    write_scan(prefix, pheno[0], ids, names, chrom, pos, chrom_names, result, info['rank'],
               0.0 if min_lod is None else min_lod, perm=done, lod_drop=lod_drop)
    logger.info(f'scan: {len(ids)} samples, {y.shape[1]} phenotypes, {scan.M} grid points; prepare '
                f'{info["prepare_ms"]:.1f} ms, run {info["run_ms"]:.1f} ms on the device')
    if snps is not None:        # read_snp_file's dict: the SNP association pass follows on the same preparation
        finish_scan_snps(scan, prefix, ids, pheno[0], names, y, snps, chrom_names, snp_grid, min_lod, lod_matrix, stage_times)
    if mediate is not None:     # mediate_options' dict: the scan's peaks are mediated on the same preparation
        finish_scan_mediation(scan, prefix, ids, pheno, names, y, dict(mediate, rankz=use_rankz), result, chrom_names, pos,
                              lod_matrix, stage_times)
    if effects is not None and effects['min_lod'] is not None:      # effects_options' dict: the peaks' founder effects
        finish_scan_effects(scan, prefix, ids, pheno, names, y, effects['min_lod'], result, chrom_names, pos, founders,
                            stage_times)
    if intcovar is not None:    # intcovar_options' names: the interaction scan on a preparation of its own
        finish_scan_int(scan, prefix, ids, pheno[0], names, z, interactive, y, chrom, pos, chrom_names, min_lod, lod_matrix)
    return info


def scan_tables(dosage_list, grid_file, pheno_file, covar_file=None, use_rankz=False, out=None, min_lod=None,
                lod_matrix=False, device=0, scan_perms=None, scan_perm_seed=None, scan_perm_alpha=None,
                scan_perm_chromosomes=None, scan_perm_pheno=None, stage_times=None, snp_file=None, scan_mediate=False,
                scan_mediate_min_lod=None, scan_mediate_top=None, scan_mediator_file=None, scan_effects=False,
                scan_effects_min_lod=None, scan_lod_drop=None, scan_kinship=None, scan_kinship_out=False, scan_kinship_snps=None,
                scan_kinship_effects=False, scan_kinship_effects_min_lod=None, scan_kinship_lod_drop=None, scan_intcovar=None):
    """`gbrs scan`: the cohort from dosage tables in `gbrs export` format (lines `id<TAB>dosage table`), rows in the grid
    file's order, without the HMM.  snp_file (`--snp-file`): the SNP association pass follows the scan;
    the haplotypes of the patterns are those of the dosage tables' header.  scan_mediate (`--scan-mediate`): the scan's
    peaks are mediated by the phenotypes or by the table of scan_mediator_file.  scan_effects
    (`--scan-effects`) and scan_lod_drop (`--scan-lod-drop`): the peaks' founder effects, named by the dosage tables'
    header, and their LOD support intervals.  scan_kinship (`--scan-kinship loco|overall`): the scan is the
    linear mixed model's; scan_kinship_out writes the kinship matrices; scan_kinship_snps
    (`--scan-kinship-snps FILE`): the SNP association pass under the mixed model follows the scan;
    scan_kinship_effects, scan_kinship_effects_min_lod and scan_kinship_lod_drop: the peaks' founder effects and support
    intervals under the mixed model.  scan_intcovar (`--scan-intcovar NAME[,NAME...]`): the scan with those
    columns of the covariate table as interactive covariates follows."""
    from .hmm import _match_lines, read_dosage_table, read_snp_file
    from .postproc import read_grid
    if min_lod is not None and not min_lod >= 0.0:
        raise RuntimeError('--scan-min-lod must be a number that is not negative')
    perm = perm_options(scan_perms, scan_perm_seed, scan_perm_alpha, scan_perm_chromosomes, scan_perm_pheno)
    mediate = mediate_options(scan_mediate, scan_mediate_min_lod, scan_mediate_top, scan_mediator_file)
    effects = effects_options(scan_effects, scan_effects_min_lod, scan_lod_drop)
    kinship = kinship_options(scan_kinship, scan_kinship_out, scan_perms, snp_file is not None, scan_mediate, scan_effects,
                              scan_lod_drop)
    kinship_snp_options(scan_kinship_snps, scan_kinship)
    kinship_effects = kinship_effects_options(scan_kinship_effects, scan_kinship_effects_min_lod, scan_kinship_lod_drop,
                                              scan_kinship)
    intcovar = intcovar_options(scan_intcovar, covar_file, scan_kinship)
    grid = read_grid(grid_file)
    chrom_names = list(grid)
    points = [len(grid[c]) for c in chrom_names]
    entries, seen = [], set()
    for number, sample_id, path in _match_lines(dosage_list, 'id<TAB>dosage table'):
        if sample_id in seen:
            raise RuntimeError(f'{dosage_list}, line {number}: id {sample_id} is given twice')
        seen.add(sample_id)
        entries.append((sample_id, path))
    pheno = read_scan_pheno(pheno_file)
    covar = read_scan_covar(covar_file) if covar_file is not None else None
    if mediate is not None and mediate['mediator_file'] is not None:
        mediate['table'] = read_scan_pheno(mediate['mediator_file'])      # refused before a dosage table is read
    if perm is not None:
        perm_plan(perm, pheno[0], [str(c) for c in chrom_names])          # refused before a dosage table is read
    if intcovar is not None:
        intcovar_plan(intcovar, covar[0])                                 # likewise
    kept, _, _, _ = scan_design([i for i, _ in entries], pheno, covar)
    if not kept:
        raise RuntimeError('scan: no sample of the dosage list has a phenotype row')
    with open(entries[kept[0]][1]) as fh:
        haplotypes = fh.readline().rstrip('\n')[2:].split('\t')
    snps = read_snp_file(snp_file, haplotypes, chrom_names, grid_file) if snp_file is not None else None
    kinship_snps = read_snp_file(scan_kinship_snps, haplotypes, chrom_names, grid_file) if scan_kinship_snps is not None else None
    scan = GenomeScan(len(haplotypes), points, device=device)
    try:
        for k in kept:
            scan.append(read_dosage_table(entries[k][1], haplotypes, sum(points)))
        chrom = np.repeat(chrom_names, points)
        pos = np.concatenate([np.asarray(grid[c], dtype=np.float64) for c in chrom_names])
        return finish_scan(scan, out if out is not None else 'gbrs', [entries[k][0] for k in kept], pheno, covar, use_rankz,
                           chrom, pos, chrom_names, min_lod, lod_matrix, perm=perm, stage_times=stage_times, snps=snps,
                           snp_grid=grid, mediate=mediate, effects=effects, founders=haplotypes, kinship=kinship,
                           kinship_snps=kinship_snps, kinship_effects=kinship_effects, intcovar=intcovar)
    finally:
        scan.close()
