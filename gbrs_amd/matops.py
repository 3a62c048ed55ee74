"""Commands that edit the structure of an alignment incidence tensor and write it back in the EMASE format:
`get-common-alignments`, `combine`, `pull-out-unique-reads` (emase/emase_utils.py:236-274, :73-111, :277-317), `stencil`
(gbrs/emase_utils.py:110-177), the `count-alignments` wrapper (emase/emase_utils.py:114-139) and
`count-shared-multireads-pairwise` (emase/emase_utils.py:142-176), which reads the tensor and writes count matrices.  Same argument names,
defaults and log lines as the reference plus `device`; the edits run in HIP (gbrs_matops_*, gbrs_amd/csrc/matops.hip) and
there is no CPU fallback.  Everything that needs no device - shapes, read names, stored values, group files - is checked
before the first device call.  `stage_times` (optional dict, as for bam2emase) receives the wall-clock seconds of the
stages load, upload (gbrs_matops_create), kernels (the edit calls; for intersect / append_rows they include the upload of
the second operand), download and write."""
from __future__ import annotations

import ctypes as C
import logging
import os
import time

import numpy as np

from . import _lib
from .alignment import AlignmentPropertyMatrix, load_alignment, read_rname

logger = logging.getLogger('gbrs')


class MatOps:
    """One sample's per-haplotype CSC arrays on the device (gbrs_matops_create) and the edits on them."""

    def __init__(self, apm, device=0):
        self._lib = _lib.load()
        L, H, R = apm.shape
        self.L, self.H = L, H
        self._h = C.c_void_p()
        _lib.check(self._lib.gbrs_matops_create(R, L, H, _lib.ptr_table(apm.indptr), _lib.ptr_table(apm.indices),
                                                device, C.byref(self._h)))

    def _same_columns(self, apm):
        if apm.shape[:2] != (self.L, self.H):
            raise RuntimeError('The matrices do not share loci / haplotypes.')

    def intersect(self, apm):
        self._same_columns(apm)
        _lib.check(self._lib.gbrs_matops_intersect(self._h, _lib.ptr_table(apm.indptr), _lib.ptr_table(apm.indices)))

    def append_rows(self, apm):
        self._same_columns(apm)
        _lib.check(self._lib.gbrs_matops_append_rows(self._h, apm.num_reads, _lib.ptr_table(apm.indptr),
                                                     _lib.ptr_table(apm.indices)))

    def keep_unique_rows(self, locus_group=None, num_groups=0, ignore_haplotype=False):
        """Returns the bool array [R] of the rows that stayed."""
        R = self.sizes()[0]
        keep = np.zeros(R, dtype=np.uint8)
        group = None if locus_group is None else np.ascontiguousarray(locus_group, dtype=np.int32)
        if group is not None and group.shape != (self.L,):
            raise RuntimeError('The locus-to-group map does not match to the matrix shape.')
        _lib.check(self._lib.gbrs_matops_keep_unique_rows(self._h, _lib.ptr(group), int(num_groups),
                                                          1 if ignore_haplotype else 0, _lib.ptr(keep)))
        return keep.astype(bool)

    def mask_columns(self, allowed):
        allowed = np.ascontiguousarray(allowed, dtype=np.uint32)
        if allowed.shape != (self.L,):
            raise RuntimeError('The haplotype mask does not match to the matrix shape.')
        _lib.check(self._lib.gbrs_matops_mask_columns(self._h, _lib.ptr(allowed)))

    def shared_counts(self, locus_group=None, num_groups=0):
        """(indptr int64[n + 1], indices int32[nnz], data float64[nnz], n) of C = P^T P in CSR form, both triangles,
        column ids ascending inside every row: C[i, j] = the reads with an entry at columns i and j in any haplotype.
        A column is a locus (n = L), or with locus_group (int[L], -1 = in no group) a group (n = num_groups).  The
        tensor is left as it is; shared_counts_info() tells how the call went."""
        group = _checked_group_map(locus_group, self.L)
        n = self.L if group is None else int(num_groups)
        nnz = C.c_uint64(0)
        _lib.check(self._lib.gbrs_matops_shared_counts(self._h, _lib.ptr(group), int(num_groups) if group is not None else 0,
                                                       C.byref(nnz)))
        indptr = np.zeros(n + 1, dtype=np.uint64)
        indices = np.zeros(nnz.value, dtype=np.uint32)
        data = np.zeros(nnz.value, dtype=np.float64)
        _lib.check(self._lib.gbrs_matops_shared_counts_get(self._h, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data)))
        return indptr.astype(np.int64), indices.astype(np.int32 if n <= 0x7FFFFFFF else np.int64), data, n

    def shared_counts_info(self):
        """The last shared_counts call: columns, distinct (read, column) entries, pairs emitted, batches, the pair
        budget of a batch, peak device bytes of the call (sampled) and its milliseconds on the device."""
        n, ent, pairs, budget, peak = (C.c_uint64(0) for _ in range(5))
        batches, ms = C.c_uint32(0), C.c_double(0.0)
        _lib.check(self._lib.gbrs_matops_shared_counts_info(self._h, C.byref(n), C.byref(ent), C.byref(pairs),
                                                            C.byref(batches), C.byref(budget), C.byref(peak), C.byref(ms)))
        return dict(num_columns=int(n.value), pattern_entries=int(ent.value), pairs_emitted=int(pairs.value),
                    batches=int(batches.value), pair_budget=int(budget.value), peak_device_bytes=int(peak.value),
                    device_ms=float(ms.value))

    def sizes(self):
        """(R, entries per haplotype uint64[H], haplotype arrays given so far that needed the radix sort)."""
        R, srt = C.c_uint64(0), C.c_uint32(0)
        nnz = np.zeros(self.H, dtype=np.uint64)
        _lib.check(self._lib.gbrs_matops_sizes(self._h, C.byref(R), _lib.ptr(nnz), C.byref(srt)))
        return int(R.value), nnz, int(srt.value)

    def get(self):
        """(R, indptr list, indices list) of the tensor as it stands; row ids ascend inside every column."""
        R, nnz, _ = self.sizes()
        ip = [np.zeros(self.L + 1, dtype=np.uint32) for _ in range(self.H)]
        ix = [np.zeros(int(n), dtype=np.uint32) for n in nnz]
        _lib.check(self._lib.gbrs_matops_get(self._h, _lib.ptr_table(ip), _lib.ptr_table(ix)))
        return R, ip, ix

    def close(self):
        if self._h is not None and self._h.value:
            self._lib.gbrs_matops_destroy(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _checked_group_map(locus_group, L):
    """The locus-to-group map as contiguous int32[L] (None stays None); another shape is refused here, on the host."""
    if locus_group is None:
        return None
    group = np.ascontiguousarray(locus_group, dtype=np.int32)
    if group.shape != (L,):
        raise RuntimeError('The locus-to-group map does not match to the matrix shape.')
    return group


class _Stages:
    def __init__(self, sink):
        self.sink = sink if sink is not None else {}
        self.t = time.perf_counter()

    def mark(self, name):
        now = time.perf_counter()
        self.sink[name] = self.sink.get(name, 0.0) + now - self.t
        self.t = now


def _load_all(emase_files):
    mats, names = [], []
    for f in emase_files:
        logger.info(f'Loading EMASE file: {f}')
        m = load_alignment(f)
        logger.debug(f'Number Loci: {m.num_loci}')
        logger.debug(f'Number Haplotypes: {m.num_haplotypes}')
        logger.debug(f'Number Reads: {m.num_reads}')
        mats.append(m)
        names.append(read_rname(f))
    return mats, names


def get_common_alignments(emase_files: list, output_file: str = None, comp_lib: str = 'zlib', device: int = 0,
                          stage_times: dict = None) -> None:
    """The alignments every file holds (two ends of a paired-end sample converted separately): the elementwise
    product of the incidence tensors.  All files must have the same (L, H, R) and the same read names; files that
    all lack read names pass, as `None == None` does in the reference.  The output has the first file's names, no
    `count` (the reference's `__mul__` drops it) and is saved incidence_only: a stored entry counts as present
    whatever its value, and no stored value reaches the output."""
    if output_file is None:
        output_file = f'alignments.common.{os.path.basename(emase_files[0])}'
    for x in emase_files:
        logger.info(f'EMASE file: {x}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Compression Library: {comp_lib}')
    st = _Stages(stage_times)
    _lib.warm_up_device_async(device)
    mats, names = _load_all(emase_files)
    first = mats[0]
    for m, rn in zip(mats[1:], names[1:]):
        if m.shape != first.shape:
            raise RuntimeError('The EMASE files do not share loci / haplotypes / reads.')
        same = (rn is None and names[0] is None) or \
            (rn is not None and names[0] is not None and np.array_equal(np.asarray(rn, dtype='S'),
                                                                        np.asarray(names[0], dtype='S')))
        if not same:
            logger.error('The read ID\'s are not compatible.')
            raise ValueError('The read ID\'s are not compatible.')
    st.mark('load')
    with MatOps(first, device=device) as dev:
        st.mark('upload')
        for m in mats[1:]:
            dev.intersect(m)
        st.mark('kernels')
        R, ip, ix = dev.get()
        st.mark('download')
    out = AlignmentPropertyMatrix(shape=first.shape, indptr=ip, indices=ix, haplotype_names=first.hname,
                                  locus_names=first.lname, read_names=names[0])
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    out.save(output_file, complib=comp_lib)
    st.mark('write')
    logger.info('Done')


def combine(emase_files: list, output_file: str, comp_lib: str = 'zlib', device: int = 0,
            stage_times: dict = None) -> None:
    """The reads of several files one after another (lanes of one sample).  Same (L, H) required; `count` is kept
    (concatenated) only when every file has one; the read names are concatenated, padded to the widest, when every
    file has them and left out otherwise (the reference raises inside `np.concatenate((None, None))` there)."""
    for x in emase_files:
        logger.info(f'EMASE file: {x}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Compression Library: {comp_lib}')
    st = _Stages(stage_times)
    _lib.warm_up_device_async(device)
    mats, names = _load_all(emase_files)
    first = mats[0]
    for m in mats[1:]:
        if m.shape[:2] != first.shape[:2]:
            raise RuntimeError('The EMASE files do not share loci / haplotypes.')
    if sum(m.num_reads for m in mats) >= 1 << 32:
        raise RuntimeError('2^32 or more reads in the combined file are not supported.')
    count = np.concatenate([m.count for m in mats]) if all(m.count is not None for m in mats) else None
    rname = np.concatenate([np.asarray(n, dtype='S') for n in names]) if all(n is not None for n in names) else None
    st.mark('load')
    with MatOps(first, device=device) as dev:
        st.mark('upload')
        for f, m in zip(emase_files[1:], mats[1:]):
            logger.info(f'Combining EMASE file: {f}')
            dev.append_rows(m)
        st.mark('kernels')
        R, ip, ix = dev.get()
        st.mark('download')
    logger.debug(f'Combined Number Reads: {R}')
    out = AlignmentPropertyMatrix(shape=(first.num_loci, first.num_haplotypes, R), indptr=ip, indices=ix, count=count,
                                  haplotype_names=first.hname, locus_names=first.lname, read_names=rname)
    logger.info(f'Saving EMASE file {output_file}')
    out.save(output_file, complib=comp_lib)
    st.mark('write')
    logger.info('Done')


def pull_out_unique_reads(alignment_file: str, output_file: str, group_file: str = None, shallow: bool = False,
                          ignore_alleles: bool = False, device: int = 0, stage_times: dict = None) -> None:
    """Keep only the alignments of uniquely aligning reads: reads with exactly one alignment, or - `ignore_alleles` -
    reads whose alignments all go to one locus.  With a group file the test is made at the gene level and applied to
    the isoform-level alignments, so a kept read may keep several isoforms of its one gene.  Shape and names are
    unchanged; `count` (when present) is 0 for the other reads; `shallow` saves without names.  The reference's test
    sums stored values; this one tests the structure, which is the same thing for incidence files, and refuses a
    file that carries stored values."""
    logger.info(f'Alignment File: {alignment_file}')
    logger.info(f'Group File: {group_file}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Shallow: {shallow}')
    logger.info(f'Ignore Alleles: {ignore_alleles}')
    st = _Stages(stage_times)
    _lib.warm_up_device_async(device)
    logger.info(f'Loading EMASE file: {alignment_file}')
    apm = load_alignment(alignment_file, grpfile=group_file)
    logger.debug(f'Number Loci: {apm.num_loci}')
    logger.debug(f'Number Haplotypes: {apm.num_haplotypes}')
    logger.debug(f'Number Reads: {apm.num_reads}')
    if apm.values is not None:
        raise RuntimeError('The alignment file carries stored values; pull-out-unique-reads on the MI355X path tests '
                           'the incidence structure only and refuses such a file.')
    group, G = None, 0
    if group_file:
        logger.debug('Using group file')
        from .counts import _group_map
        group, _ = _group_map(apm)                 # refuses a locus listed in two groups
        G = apm.num_groups
    else:
        logger.debug('Not using group file')
    rname = None if shallow else read_rname(alignment_file)
    st.mark('load')
    logger.info('Getting unique reads')
    with MatOps(apm, device=device) as dev:
        st.mark('upload')
        keep = dev.keep_unique_rows(group, G, ignore_haplotype=ignore_alleles)
        st.mark('kernels')
        R, ip, ix = dev.get()
        st.mark('download')
    count = None
    if apm.count is not None:
        count = apm.count.copy()
        count[~keep] = 0
    out = AlignmentPropertyMatrix(shape=apm.shape, indptr=ip, indices=ix, count=count,
                                  haplotype_names=None if shallow else apm.hname,
                                  locus_names=None if shallow else apm.lname, read_names=rname)
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    out.save(output_file, shallow=shallow)
    st.mark('write')
    logger.info('Done')


def stencil(alignment_file: str, genotype_file: str, group_file: str = None, output_file: str = None,
            device: int = 0, stage_times: dict = None) -> None:
    """Apply genotype calls to a multi-way alignment incidence file and save the result: the output is the input
    without exactly the entries `gbrs quantify -G <genotype_file>` removes before its EM.  (The reference's function
    cannot run as it stands: it assigns `out_file` where `output_file` is meant and indexes `gtmask` with a bare
    `np.meshgrid`.)  The group file is resolved like quantify's; without any, the first column of the genotype file
    names loci ("stenciled as is").  `count`, names and read names are carried over; a file with stored values is
    refused, as the device holds the structure alone."""
    from .quantify import (DEFAULT_GROUP_FILE, diplotype_mask, genotype_mask_from_file, read_genotype_table)
    if group_file is None:
        group_file = os.path.join(os.getenv('GBRS_DATA', '.'), DEFAULT_GROUP_FILE)
        if not os.path.exists(group_file):
            logger.info('A group file is *not* given. Genotype will be stenciled as is.')
            group_file = None
    if output_file is None:
        output_file = f'gbrs.stenciled.{os.path.basename(alignment_file)}'
    logger.info(f'Alignment File: {alignment_file}')
    logger.info(f'Genotype File: {genotype_file}')
    logger.info(f'Group File: {group_file}')
    logger.info(f'Output File: {output_file}')
    st = _Stages(stage_times)
    _lib.warm_up_device_async(device)
    logger.info(f'Loading EMASE file: {alignment_file}')
    apm = load_alignment(alignment_file, grpfile=group_file)
    logger.debug(f'Number Loci: {apm.num_loci}')
    logger.debug(f'Number Haplotypes: {apm.num_haplotypes}')
    logger.debug(f'Number Reads: {apm.num_reads}')
    if apm.values is not None:
        raise RuntimeError('The alignment file carries stored values; stencil on the MI355X path edits the incidence '
                           'structure only and refuses such a file.')
    if group_file is None:                           # every locus a gene of its own
        if apm.lname is None:
            raise RuntimeError('Locus IDs are not available.')
        apm.gname = np.array(apm.lname)
        apm.groups = [[l] for l in range(apm.num_loci)]
        apm.num_groups = apm.num_loci
    logger.info(f'Loading and processing genotype calls from: {genotype_file}')
    allowed = (genotype_mask_from_file(apm, genotype_file) or
               diplotype_mask(apm, read_genotype_table(genotype_file)))[0]
    rname = read_rname(alignment_file)
    st.mark('load')
    with MatOps(apm, device=device) as dev:
        st.mark('upload')
        dev.mask_columns(allowed)
        st.mark('kernels')
        R, ip, ix = dev.get()
        st.mark('download')
    out = AlignmentPropertyMatrix(shape=apm.shape, indptr=ip, indices=ix, count=apm.count, haplotype_names=apm.hname,
                                  locus_names=apm.lname, read_names=rname)
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    out.save(output_file)
    st.mark('write')
    logger.info('Done')


def count_alignments(alignment_file: str, group_file: str, outbase: str = 'emase', device: int = 0) -> None:
    """The two reports `gbrs quantify -a` writes (gbrs_amd/counts.py), under the names of emase/emase_utils.py:114-139."""
    from .counts import AlignmentCounter, report_alignment_counts
    logger.info(f'Alignment File: {alignment_file}')
    logger.info(f'Group File: {group_file}')
    logger.info(f'Outbase: {outbase}')
    if group_file is None:
        raise RuntimeError('count-alignments needs a group file.')
    _lib.warm_up_device_async(device)
    logger.info(f'Loading EMASE file: {alignment_file}')
    apm = load_alignment(alignment_file, grpfile=group_file)
    logger.debug(f'Number Loci: {apm.num_loci}')
    logger.debug(f'Number Haplotypes: {apm.num_haplotypes}')
    logger.debug(f'Number Reads: {apm.num_reads}')
    from .counts import _group_map
    _group_map(apm)                                   # a locus in two groups is refused before the device is opened
    with AlignmentCounter(apm, device=device) as counter:
        for level, grp_wise in (('isoform', False), ('gene', True)):
            path = f'{outbase}.{level}s.alignment_counts'
            logger.info(f'Generating {level} Alignment Counts: {path}')
            report_alignment_counts(apm, path, grp_wise=grp_wise, device=device, counter=counter)
    logger.info('Done')


def save_shared_counts(path: str, indptr, indices, data, n: int) -> str:
    """One shared-read-count matrix as `<path>` (`.npz` is appended when missing, as numpy does).  Always the plain
    members `indptr`, `indices`, `data` and `shape` of the n x n CSR matrix, readable with allow_pickle=False.  Where
    scipy can be imported also `counts`, what the reference's `np.savez_compressed(name, counts=cnt_mat)` leaves: a 0-d
    object array with the pickled float64 `scipy.sparse.csr_matrix`.  Without scipy `counts` is left out and one
    warning says so.  Needs no device.  Returns the path written."""
    if not path.endswith('.npz'):
        path += '.npz'
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32 if n <= 0x7FFFFFFF else np.int64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    if indptr.shape != (n + 1,) or indices.shape != data.shape or int(indptr[-1]) != len(data):
        raise RuntimeError('The count matrix arrays do not match to its shape.')
    members = dict(indptr=indptr, indices=indices, data=data, shape=np.array([n, n], dtype=np.int64))
    try:
        from scipy.sparse import csr_matrix
    except ImportError:
        logger.warning(f'scipy is not available: {path} holds indptr/indices/data/shape only, not the pickled '
                       '`counts` matrix.')
    else:
        members['counts'] = csr_matrix((data, indices, indptr), shape=(n, n))
    np.savez_compressed(path, **members)
    return path


def shared_counts_paths(outbase: str = 'emase', separate_outputs: bool = False):
    """(isoform-level path, gene-level path) without `.npz`.  The reference gives both levels one name
    (emase/emase_utils.py:164, :171), so its gene-level matrix overwrites the isoform-level one; that is the default."""
    iso = f'{outbase}.isoforms.shared_read_counts'
    return iso, (f'{outbase}.genes.shared_read_counts' if separate_outputs else iso)


def count_shared_multireads_pairwise(alignment_file: str, group_file: str, outbase: str = 'emase', device: int = 0,
                                     stage_times: dict = None, separate_outputs: bool = False) -> None:
    """For every pair of loci, then for every pair of genes, the number of reads that align to both, in any haplotype
    (emase/emase_utils.py:142-176); the diagonal holds the reads per locus / gene.  Stored values are ignored (an
    entry counts as present) and so is a `count` vector: every row counts once, as in the reference.  By default a run
    leaves what the reference leaves - `<outbase>.isoforms.shared_read_counts.npz` holding the GENE-level matrix, which
    has overwritten the isoform-level one; `separate_outputs` keeps both (`...isoforms...` and `...genes...`)."""
    logger.info(f'Alignment File: {alignment_file}')
    logger.info(f'Group File: {group_file}')
    logger.info(f'Outbase: {outbase}')
    if group_file is None:
        raise RuntimeError('count-shared-multireads-pairwise needs a group file.')
    st = _Stages(stage_times)
    _lib.warm_up_device_async(device)
    logger.info(f'Loading EMASE file: {alignment_file}')
    apm = load_alignment(alignment_file, grpfile=group_file)
    logger.debug(f'Number Loci: {apm.num_loci}')
    logger.debug(f'Number Haplotypes: {apm.num_haplotypes}')
    logger.debug(f'Number Reads: {apm.num_reads}')
    from .counts import _group_map
    group, _ = _group_map(apm)                       # a locus in two groups is refused before the device is opened
    if apm.count is not None:
        logger.info('The alignment file carries a count vector; as in the reference it is ignored and every row counts once.')
    outfile1, outfile2 = shared_counts_paths(outbase, separate_outputs)
    st.mark('load')
    with MatOps(apm, device=device) as dev:
        st.mark('upload')
        for level, path, grp in (('isoform', outfile1, None), ('genes', outfile2, group)):
            logger.info(f'Generating {level} Shared Read Counts: {path}')
            indptr, indices, data, n = dev.shared_counts(grp, apm.num_groups if grp is not None else 0)
            info = dev.shared_counts_info()
            logger.debug(f'{n} columns, {len(data)} stored counts, {info["pairs_emitted"]} pairs in {info["batches"]} '
                         f'batches, {info["device_ms"]:.1f} ms on the device')
            if stage_times is not None:
                stage_times[f'shared_counts_{level}'] = dict(info, nnz=int(len(data)))
            st.mark('kernels')
            save_shared_counts(path, indptr, indices, data, n)
            st.mark('write')
    logger.info('Done')
