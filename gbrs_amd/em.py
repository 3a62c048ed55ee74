"""EMfactory: the reference's EM driver interface backed by libgbrs_hip.so.

Same constructor, method names, argument meaning, printed progress table and error behaviour as
emase/EMfactory.py:15-392 for the paths that `gbrs quantify` drives
(gbrs/emase_utils.py:282-316): Model 4, and models 1-3 (`-M 1|2|3`, which need gene groups).  All
arithmetic of prepare / run happens in HIP kernels through the C ABI in include/gbrs_hip.h; this
module never computes an EM quantity on the host and has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib


class EMfactory:
    """A class that coordinates Expectation-Maximization (MI355X HIP path)."""

    def __init__(self, alignments, device: int = 0, merge_identical_rows: bool = False,
                 csc_layout: bool = False, extra_flags: int = 0, deterministic: bool = False,
                 one_shot: bool = False, grouped_models: bool = False, keep_posterior: bool = False,
                 resample: bool = False):
        self.probability = alignments
        # GBRS_EM_DETERMINISTIC=1 in the environment: the bit-reproducible E-step for every handle on the tile layout
        deterministic = deterministic or (os.getenv('GBRS_EM_DETERMINISTIC') == '1' and not csc_layout)
        self.grp_conv_mat = None          # kept for attribute parity; groups live in probability
        self.t2t_mat = None               # Models 1-3 (EMfactory.py:48-59): the device holds the groups instead
        self.target_lengths = None
        self.device = device
        self.flags = (_lib.GBRS_EM_MERGE_IDENTICAL_ROWS if merge_identical_rows else 0) | \
                     (_lib.GBRS_EM_LAYOUT_CSC if csc_layout else 0) | \
                     (_lib.GBRS_EM_DETERMINISTIC if deterministic else 0) | \
                     (_lib.GBRS_EM_ONE_SHOT if one_shot else 0) | \
                     (_lib.GBRS_EM_GROUPED_MODELS if grouped_models else 0) | \
                     (_lib.GBRS_EM_POSTERIOR if keep_posterior else 0) | \
                     (_lib.GBRS_EM_RESAMPLE if resample else 0) | int(extra_flags)   # tuning switches of gbrs_hip.h
        self._h = None
        self._theta = None                # host copy of allelic_expression (H x L)
        self._theta_dirty = False         # host copy edited, device not yet updated
        self.num_iters = 0
        self.err_history = []

    # ------------------------------------------------------------------ handle management
    def _create(self):
        lib = _lib.load()
        apm = self.probability
        L, H, R = apm.shape
        tab_p = _lib.ptr_table(apm.indptr)
        tab_i = _lib.ptr_table(apm.indices)
        h = C.c_void_p()
        eff = None
        if self.target_lengths is not None:
            eff = np.ascontiguousarray(self.target_lengths, dtype=np.float64)
        cnt = None if apm.count is None else np.ascontiguousarray(apm.count, dtype=np.float64)
        vals = getattr(apm, 'values', None)
        flags = self.flags | (_lib.GBRS_EM_KEEP_CSC if vals is not None else 0)
        allowed = getattr(apm, 'haplotype_mask', None)      # `-G`: the device drops the masked columns
        if allowed is not None:
            allowed = np.ascontiguousarray(allowed, dtype=np.uint32)
            _lib.check(lib.gbrs_em_create_masked(R, L, H, tab_p, tab_i, _lib.ptr(cnt), _lib.ptr(eff),
                                                 _lib.ptr(allowed), self.device, flags, C.byref(h)))
        else:
            _lib.check(lib.gbrs_em_create(R, L, H, tab_p, tab_i, _lib.ptr(cnt), _lib.ptr(eff),
                                          self.device, flags, C.byref(h)))
        self._h = h
        if vals is not None:
            # the file stores alignment values: they fix the starting point (EMfactory.py:95-98)
            vals = [np.ascontiguousarray(v, dtype=np.float64) for v in vals]
            _lib.check(lib.gbrs_em_set_initial_values(h, _lib.ptr_table(vals)))
        if (self.flags & _lib.GBRS_EM_GROUPED_MODELS) and apm.num_groups:
            gptr, mem = apm.group_csr()
            _lib.check(lib.gbrs_em_set_groups(h, int(apm.num_groups), _lib.ptr(gptr), _lib.ptr(mem)))

    def close(self):
        if self._h is not None:
            _lib.load().gbrs_em_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        inf = _lib.EmInfo()
        _lib.check(_lib.load().gbrs_em_info(self._h, C.byref(inf)))
        return inf

    # ------------------------------------------------------------------ reference interface
    def prepare(self, pseudocount: float = 0.0, lenfile: str = None, read_length: int = 100) -> None:
        """Initializes the probability of read origin according to the alignment profile
        (EMfactory.py:27-111)."""
        apm = self.probability
        if lenfile is not None:
            self.set_target_lengths(read_length_file(apm, lenfile, read_length))
        self.close()
        self._create()
        _lib.check(_lib.load().gbrs_em_prepare(self._h, float(pseudocount)))
        self._theta = None
        self._theta_dirty = False

    def set_target_lengths(self, lengths):
        """Effective lengths (H x L) as read_length_file returns them, with prepare()'s check (EMfactory.py:88-90)."""
        self.target_lengths = lengths
        if not np.all(self.target_lengths > 0.0):
            raise RuntimeError('There exist transcripts missing length information.')

    def _require(self):
        if self._h is None:
            raise RuntimeError('prepare() has not been called.')

    def _push(self):
        if self._theta_dirty:
            _lib.check(_lib.load().gbrs_em_set_theta(self._h, _lib.ptr(np.ascontiguousarray(self._theta))))
            self._theta_dirty = False

    @property
    def allelic_expression(self):
        self._require()
        if self._theta is None:
            L, H, R = self.probability.shape
            out = np.empty((H, L), dtype=np.float64)
            _lib.check(_lib.load().gbrs_em_get(self._h, _lib.ptr(out), None))
            self._theta = out
        return self._theta

    @allelic_expression.setter
    def allelic_expression(self, value):
        self._require()
        L, H, R = self.probability.shape
        self._theta = np.ascontiguousarray(value, dtype=np.float64).reshape(H, L)
        self._theta_dirty = True

    def expected_read_counts(self):
        """probability.sum(axis=READ) of the last E-step (EMfactory.py:302), (H x L)."""
        self._require()
        L, H, R = self.probability.shape
        out = np.empty((H, L), dtype=np.float64)
        _lib.check(_lib.load().gbrs_em_get(self._h, None, _lib.ptr(out)))
        return out

    def posterior(self, hid: int) -> np.ndarray:
        """float64[nnz_h]: the posterior of every stored entry of haplotype `hid` in the last E-step - what the
        reference's probability.data[hid] holds after a step - in the order of the (masked) indices[hid].  Needs
        keep_posterior=True and at least one step since prepare()."""
        self._require()
        apm = self.probability
        hid = int(hid)
        if not 0 <= hid < apm.num_haplotypes:
            raise RuntimeError(f'Haplotype {hid} is out of range: the matrix has {apm.num_haplotypes}.')
        ptr = apm.indptr[hid]
        mask = apm.haplotype_mask
        if mask is None:
            nnz = int(ptr[-1])
        else:               # a pending `-G` mask: the device dropped the columns, the host arrays still hold them
            keep = ((mask >> np.uint32(hid)) & 1).astype(bool)
            nnz = int(np.diff(ptr.astype(np.int64))[keep].sum())
        out = np.empty(nnz, dtype=np.float64)
        _lib.check(_lib.load().gbrs_em_posterior(self._h, hid, _lib.ptr(out), nnz))
        return out

    # ------------------------------------------------------------------ bootstrap replicates (extension)
    def resample(self, seed: int, replicate: int) -> None:
        """Draws the row weights of bootstrap replicate `replicate` on the device (Poisson(count[r]) per row, a function
        of (seed, replicate, row id, count) alone) and installs them on the handle; replicate=_lib.GBRS_RESAMPLE_BASE puts
        the base weights back.  Needs resample=True.  reprepare() and run() come next."""
        self._require()
        _lib.check(_lib.load().gbrs_em_resample(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate) & 0xFFFFFFFF))
        self._theta = None
        self._theta_dirty = False

    def weights(self) -> np.ndarray:
        """float64[R]: the current row weights of a resampling handle, in file row order."""
        self._require()
        out = np.empty(self.probability.shape[2], dtype=np.float64)
        _lib.check(_lib.load().gbrs_em_weights(self._h, _lib.ptr(out)))
        return out

    def reprepare(self, pseudocount: float = 0.0) -> None:
        """prepare()'s starting point again on the handle as it stands (after resample()), without rebuilding it."""
        self._require()
        _lib.check(_lib.load().gbrs_em_prepare(self._h, float(pseudocount)))
        self._theta = None
        self._theta_dirty = False

    def bootstrap_begin(self) -> None:
        """Clears the replicate statistics on the device; gene level when the alignments carry groups."""
        self._require()
        apm = self.probability
        if apm.num_groups:
            gptr, mem = apm.group_csr()
            _lib.check(_lib.load().gbrs_em_bootstrap_begin(self._h, int(apm.num_groups), _lib.ptr(gptr), _lib.ptr(mem)))
        else:
            _lib.check(_lib.load().gbrs_em_bootstrap_begin(self._h, 0, None, None))

    def bootstrap_add(self, keep: bool = False):
        """Folds the handle's current result into the statistics as one more replicate.  keep: returns this replicate's
        values as they were folded in, {'tpm', 'expected_read_counts'} (H x L) and with groups {'gene_tpm',
        'gene_expected_read_counts'} (H x G)."""
        self._require()
        self._push()
        apm = self.probability
        L, H, R = apm.shape
        G = int(apm.num_groups or 0)
        out = {}
        if keep:
            out['tpm'] = np.empty((H, L))
            out['expected_read_counts'] = np.empty((H, L))
            if G:
                out['gene_tpm'] = np.empty((H, G))
                out['gene_expected_read_counts'] = np.empty((H, G))
        _lib.check(_lib.load().gbrs_em_bootstrap_add(self._h, _lib.ptr(out.get('tpm')), _lib.ptr(out.get('expected_read_counts')),
                                                     _lib.ptr(out.get('gene_tpm')), _lib.ptr(out.get('gene_expected_read_counts'))))
        return out if keep else None

    def bootstrap_get(self, grp_wise: bool = False) -> dict:
        """Means and standard deviations (B - 1 in the denominator) over the replicates added so far: tpm_mean, tpm_sd,
        count_mean, count_sd (H x n), tpm_total_mean, tpm_total_sd, count_total_mean, count_total_sd (n), num_replicates."""
        self._require()
        apm = self.probability
        H = apm.num_haplotypes
        n = int(apm.num_groups) if grp_wise else apm.num_loci
        if grp_wise and not n:
            raise RuntimeError('No group information is available.')
        res = {k: np.empty((H, n)) for k in ('tpm_mean', 'tpm_sd', 'count_mean', 'count_sd')}
        res.update({k: np.empty(n) for k in ('tpm_total_mean', 'tpm_total_sd', 'count_total_mean', 'count_total_sd')})
        nrep = C.c_uint32(0)
        _lib.check(_lib.load().gbrs_em_bootstrap_get(
            self._h, 1 if grp_wise else 0, C.byref(nrep), _lib.ptr(res['tpm_mean']), _lib.ptr(res['tpm_sd']),
            _lib.ptr(res['count_mean']), _lib.ptr(res['count_sd']), _lib.ptr(res['tpm_total_mean']),
            _lib.ptr(res['tpm_total_sd']), _lib.ptr(res['count_total_mean']), _lib.ptr(res['count_total_sd'])))
        res['num_replicates'] = int(nrep.value)
        return res

    def bootstrap(self, model: int, replicates: int, seed: int = 0, pseudocount: float = 0.0, tol: float = 0.001,
                  max_iters: int = 999, keep: bool = False) -> dict:
        """`replicates` bootstrap refits: resample -> prepare -> run -> accumulate for b = 0 .. replicates - 1, everything on
        the device.  Returns {'isoforms': statistics, 'genes': statistics (with groups), 'num_iters': int32[B]} and, with
        keep, 'tpm' / 'expected_read_counts' (B x H x L) and 'gene_tpm' / 'gene_expected_read_counts' (B x H x G).  The
        base weights are back on the handle when it returns."""
        np.seterr(all='raise', under='ignore')
        self._check_model(model)
        self._require()
        if not (self.flags & _lib.GBRS_EM_RESAMPLE):
            raise RuntimeError('bootstrap() needs an EMfactory built with resample=True.')
        B = int(replicates)
        if B < 1:
            raise RuntimeError('The number of bootstrap replicates must be positive.')
        self._ready_for_resampling(model)
        lib = _lib.load()
        self.bootstrap_begin()
        num_iters = np.zeros(B, dtype=np.int32)
        kept = {}
        n_it = C.c_int(0)
        try:
            for b in range(B):
                self.resample(seed, b)
                self.reprepare(pseudocount)
                _lib.check(lib.gbrs_em_run(self._h, int(model), float(tol), int(max_iters), C.byref(n_it), None, 0, None))
                num_iters[b] = n_it.value
                vals = self.bootstrap_add(keep=keep)
                if keep:
                    for k, v in vals.items():
                        kept.setdefault(k, []).append(v)
        finally:
            self.resample(seed, _lib.GBRS_RESAMPLE_BASE)
        self.num_iters = int(num_iters[-1])
        res = {'isoforms': self.bootstrap_get(False), 'num_iters': num_iters}
        if self.probability.num_groups:
            res['genes'] = self.bootstrap_get(True)
        for k, v in kept.items():
            res[k] = np.stack(v)
        return res

    def _ready_for_resampling(self, model):
        if model != 4 and not (self.flags & _lib.GBRS_EM_GROUPED_MODELS):
            self.flags |= _lib.GBRS_EM_GROUPED_MODELS
            self.close()
            self._create()

    def _group_sums(self, which):
        apm = self.probability
        if not apm.num_groups:
            raise RuntimeError('No group information is available.')
        self._push()
        gptr, mem = apm.group_csr()
        H = apm.num_haplotypes
        out = np.empty((H, apm.num_groups), dtype=np.float64)
        _lib.check(_lib.load().gbrs_em_group_sums(self._h, apm.num_groups, _lib.ptr(gptr), _lib.ptr(mem),
                                                  which, _lib.ptr(out)))
        # scipy hands the reference this product as the transpose of a C-ordered (G x H) array;
        # keep that memory order so a later full `.sum()` adds in the same sequence
        return np.asfortranarray(out)

    def get_allelic_expression(self, at_group_level: bool = False):
        if at_group_level:
            return self._group_sums(0)
        return self.allelic_expression.copy()

    def update_allelic_expression(self, model: int = 4) -> None:
        """A single EM step (EMfactory.py:214-232)."""
        self._check_model(model)
        self._require()
        self._ready_for(model)
        self._push()
        lib = _lib.load()
        _lib.check(lib.gbrs_em_step(self._h, 1, None) if model == 4 else lib.gbrs_em_step_model(self._h, int(model), 1, None))
        self._theta = None

    def _check_model(self, model):
        if model not in (1, 2, 3, 4):
            raise RuntimeError('The read normalization model should be 1, 2, 3, or 4.')
        if model != 4 and not self.probability.num_groups:
            # the reference's normalize_reads raises the first part (AlignmentPropertyMatrix.py:348)
            raise RuntimeError(f'Group information matrix is missing: multiread model {model} is not implemented '
                               'without gene groups.')

    def _ready_for(self, model):
        """Models 1-3 step on the grouped layout: a handle built without it is rebuilt once, theta carried over."""
        if model == 4 or (self.flags & _lib.GBRS_EM_GROUPED_MODELS):
            return
        theta = self.allelic_expression.copy()
        self.flags |= _lib.GBRS_EM_GROUPED_MODELS
        self.close()
        self._create()
        self.allelic_expression = theta

    def run(self, model: int, tol: float = 0.001, max_iters: int = 999, verbose: bool = True) -> None:
        """Runs EM iterations (EMfactory.py:234-287): the whole loop, stopping rule included, executes
        on the device (gbrs_em_run); the host sees it once per batch of 8 iterations."""
        np.seterr(all='raise', under='ignore')      # the state the reference leaves numpy in
        self._check_model(model)
        self._require()
        self._ready_for(model)
        self._push()
        cap = max(int(max_iters), 1)
        hist = np.zeros(cap, dtype=np.float64)
        stamps = np.zeros(cap, dtype=np.float64)
        n_it = C.c_int(0)
        _lib.check(_lib.load().gbrs_em_run(self._h, int(model), float(tol), int(max_iters), C.byref(n_it),
                                           _lib.ptr(hist), cap, _lib.ptr(stamps)))
        self.num_iters = int(n_it.value)
        self.err_history = hist[:self.num_iters].tolist()
        self._theta = None
        if verbose:
            _print_progress(self.err_history, stamps[:self.num_iters])

    # ------------------------------------------------------------------ reports
    report_pool = None      # a ReportPool: report_* hand their files to it instead of writing them before returning

    def _level(self, grp_wise, which):
        """(row names, H x n values) of theta (which=0) or of the expected read counts (which=1) at
        isoform or gene level."""
        apm = self.probability
        if grp_wise:
            return apm.gname, self._group_sums(which)
        return apm.lname, (self.allelic_expression if which == 0 else self.expected_read_counts())

    def report_read_counts(self, filename, grp_wise=False, reorder='as-is', notes=None):
        """Expected read counts of the last E-step as a TSV table (file format of EMfactory.py:289-331)."""
        names, values = self._level(grp_wise, 1)
        write_locus_table(filename, self.probability.hname, names, values, reorder, notes, pool=self.report_pool)

    def report_depths(self, filename, tpm=True, grp_wise=False, reorder='as-is', notes=None) -> None:
        """Depths (theta) as a TSV table, scaled to TPM on request (file format of EMfactory.py:333-380).
        Reference behaviour kept: at isoform level the TPM scaling is applied to allelic_expression
        itself, so it carries over to whatever is reported next (:352-354)."""
        names, values = self._level(grp_wise, 0)
        if tpm:
            values *= 1000000.0 / values.sum()
            if not grp_wise:
                self._theta_dirty = True
        write_locus_table(filename, self.probability.hname, names, values, reorder, notes, pool=self.report_pool)

    def export_posterior_probability(self, filename: str, title: str = 'Posterior Probability',
                                     values: bool = False) -> None:
        """The reference saves with incidence_only=True (EMfactory.py:392 ->
        AlignmentPropertyMatrix.py:484), i.e. the structure without posterior values.
        values=True (extension, needs keep_posterior=True): the file carries /h*/data with the posteriors of the
        last E-step, fetched from the device one haplotype at a time (incidence_only=False, the reference's own
        layout for stored values)."""
        if not values:
            self.probability.save(filename, title=title)
            return
        self._require()
        self.probability.save(filename, title=title, incidence_only=False, values=self.posterior)


def _print_progress(err_history, stamps):
    """The reference's progress table (EMfactory.py:259-262, :284-287); the time column holds the
    moment the host learned of the iteration (one stamp per device batch of 8)."""
    print('')
    print('Iter No  Time (hh:mm:ss)    Total change (TPM)  ')
    print('-------  ---------------  ----------------------')
    for k, (err, t) in enumerate(zip(err_history, stamps), start=1):
        secs = int(t)
        print(' %5d      %4d:%02d:%02d     %9.1f / 1000000' % (k, secs // 3600, secs // 60 % 60, secs % 60, err))


def read_length_file(apm, lenfile, read_length=100):
    """Effective lengths (H x L) from a `<locus>_<haplotype>TAB<length>` table (plain `<locus>` ids when
    there is one haplotype): max(length - read_length + 1, 1), what EMfactory.prepare builds at
    EMfactory.py:60-94.  As there, an id is cut at its underscore into exactly two parts, so a locus id
    that itself contains '_' is an error."""
    L, H = apm.num_loci, apm.num_haplotypes
    if H < 1:
        raise RuntimeError('There is something wrong with your emase-format alignment file.')
    eff = np.zeros((H, L))
    # plain files (every line `<known locus>_<known haplotype> TAB <number>`) are parsed natively; anything
    # else goes through the line-by-line path below, which raises what the reference raises
    with open(lenfile, 'rb') as fh:
        text = fh.read()
    name_blob, name_off = _blob_cached(apm.lname)
    hap_blob, hap_off = _blob(apm.hname)
    st = _lib.load().gbrs_parse_length_table(text, len(text), name_blob, _lib.ptr(name_off), L, hap_blob,
                                             _lib.ptr(hap_off), H, float(read_length), _lib.ptr(eff))
    if st == 0:
        return eff
    if st < 0:
        _lib.check(st)
    del text
    eff[:] = 0.0
    hap_row = {name: k for k, name in enumerate(apm.hname)}
    with open(lenfile) as fh:
        for line in fh:
            key, value = line.rstrip().split('\t')[:2]
            if H > 1:
                locus, hap = key.split('_')           # ValueError on a second underscore, as in the reference
                row = hap_row[hap]
            else:
                locus, row = key, 0
            eff[row, apm.lid[locus]] = max(float(value) - read_length + 1.0, 1.0)
    return eff


def _blob(strings):
    """(utf-8 bytes of the strings laid end to end, int64 offsets [n + 1])."""
    enc = [x.encode() for x in strings]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=len(enc)), out=off[1:])
    return b''.join(enc), off


_blob_cache = {}


def _blob_cached(names):
    """_blob of a name list, remembered per list object: the isoform (and gene) names are written into
    two reports each.  A numpy string array (the gene names) is laid out without touching its elements."""
    key = id(names)
    hit = _blob_cache.get(key)
    if hit is None or hit[0] is not names:
        made = None
        if isinstance(names, np.ndarray) and names.dtype.kind == 'U' and names.ndim == 1:
            made = _blob_of_unicode_array(names)
        if made is None:
            made = _blob([str(x) for x in names])
        if len(_blob_cache) > 4:
            _blob_cache.clear()
        hit = _blob_cache[key] = (names, made)
    return hit[1]


def _blob_of_unicode_array(arr):
    """(bytes, offsets) of an ASCII 'U' array from its code points, None when a name is not plain ASCII (or holds
    an inner NUL, which the fixed-width storage cannot tell from padding)."""
    n, width = len(arr), arr.dtype.itemsize // 4
    if n == 0 or width == 0:
        return b'', np.zeros(n + 1, dtype=np.int64)
    code = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint32).reshape(n, width)
    if (code > 127).any():
        return None
    used = code != 0
    length = used.sum(axis=1)
    if (used != (np.arange(width)[None, :] < length[:, None])).any():
        return None
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(length, out=off[1:])
    return code[used].astype(np.uint8).tobytes(), off


def write_locus_table(filename, hap_names, row_names, values, reorder='as-is', notes=None, pool=None):
    """`locus <haplotypes...> total [notes]` table: one line per locus (or gene) with the per-haplotype
    values, their sum and, when `notes` maps names to text, that text.  Numbers are written in their
    shortest round-trip form, which is what str(numpy.float64) gives in the reference's writers; the
    text is produced by libgbrs_hip's gbrs_write_locus_table (1.5 M numbers per sample at DO size).
    `pool` (a ReportPool) takes the formatting and writing onto a thread: the caller goes on to the next report and
    collects errors with pool.finish(); `values` must not change until then."""
    values = np.asarray(values, dtype=np.float64)
    totals = values.sum(axis=0)
    order = None
    if reorder in ('increasing', 'decreasing'):
        order = np.argsort(totals.ravel())
        if reorder == 'decreasing':
            order = order[::-1]
        order = np.ascontiguousarray(order, dtype=np.int64)
    elif reorder != 'as-is':
        raise ValueError(f'unknown reorder option: {reorder}')
    if not (values.flags.c_contiguous or values.flags.f_contiguous):
        values = np.ascontiguousarray(values)
    totals = np.ascontiguousarray(totals.ravel(), dtype=np.float64)
    n_haps, n_rows = values.shape
    item = values.itemsize
    names = row_names if isinstance(row_names, (list, np.ndarray)) else [str(x) for x in row_names]
    if len(names) != n_rows:
        raise RuntimeError('The number of names does not match to the matrix shape.')
    name_blob, name_off = _blob_cached(names)
    note_blob = note_off = None
    if notes is not None:
        aligned = notes.aligned_blob(row_names) if hasattr(notes, 'aligned_blob') else None
        note_blob, note_off = aligned if aligned is not None else _blob([str(notes[n]) for n in names])
    head = '\t'.join(['locus', *hap_names, 'total'] + (['notes'] if notes is not None else [])) + '\n'

    def emit():       # every array the call reads is held by this closure
        _lib.check(_lib.load().gbrs_write_locus_table(
            os.fsencode(filename), head.encode(), _lib.ptr(values), n_rows, n_haps, values.strides[1] // item,
            values.strides[0] // item, _lib.ptr(totals), name_blob, _lib.ptr(name_off), note_blob,
            _lib.ptr(note_off) if note_off is not None else None, _lib.ptr(order) if order is not None else None))
    if pool is None:
        emit()
    else:
        pool.submit(emit)


class ReportPool:
    """Report files written behind the caller's back: `gbrs quantify` leaves four tables of 10^5 lines each, and the
    numbers of the next one can be fetched from the device while the previous one is formatted and written."""

    def __init__(self):
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=4)
        self._pending = []

    def submit(self, fn):
        self._pending.append(self._pool.submit(fn))

    def finish(self):
        """Wait for every table; the first failure is raised here."""
        pending, self._pending = self._pending, []
        try:
            for f in pending:
                f.result()
        finally:
            self._pool.shutdown(wait=True)
