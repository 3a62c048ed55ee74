"""Commands that edit the structure of an alignment incidence tensor and write it back in the EMASE format:
`get-common-alignments`, `combine`, `pull-out-unique-reads` (emase/emase_utils.py:236-274, :73-111, :277-317), `stencil`
(gbrs/emase_utils.py:110-177) and the `count-alignments` wrapper (emase/emase_utils.py:114-139).  Same argument names,
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
