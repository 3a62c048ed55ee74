"""`gbrs bam2emase` on the MI355X path: same arguments, log lines and output file as
emase/emase_utils.py:26-70 + emase/AlignmentMatrixFactory.py:26-142, without pysam, PyTables or temporary
files.  The BAM file is inflated and parsed by the library's host reader (gbrs_bam_open / bamio.hip); ranking
the read names and building the per-haplotype CSC matrices runs in HIP (gbrs_bam_convert / bam.hip).

`gbrs bam2ec` (extension) goes from one or more BAM files straight to the file `gbrs compress` writes: the
read-level matrices stay on the device and the read names are never gathered (gbrs_ecset_* / bam.hip).  With
`--mate-file` the two ends of a paired-end sample are intersected there as well (gbrs_ecset_add_bam_pair)."""
from __future__ import annotations

import ctypes as C
import logging
import time

import numpy as np

from . import _lib
from .alignment import AlignmentPropertyMatrix

logger = logging.getLogger('gbrs')

_UNUSABLE = 0xFFFFFFFF
_NOT_TWO_PARTS, _UNKNOWN_HAPLOTYPE, _UNKNOWN_LOCUS = 1, 2, 3
_INCOMPATIBLE = "The read ID's are not compatible."      # emase/emase_utils.py:262-264


def get_names(id_file):
    """First tab-separated field of every line, first occurrence order, duplicates dropped (utils.py:160-181)."""
    ids = {}
    with open(id_file) as fh:
        for line in fh:
            ids.setdefault(line.rstrip().split('\t')[0], len(ids))
    return list(ids)


class BamFile:
    """A gbrs_bam handle: the header on open, the host-only record scan, the conversion."""

    def __init__(self, path, threads=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        n_ref, names_len = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.gbrs_bam_open(str(path).encode(), threads, C.byref(self._h), C.byref(n_ref),
                                           C.byref(names_len)))
        try:
            buf = np.zeros(max(int(names_len.value), 1), dtype=np.uint8)
            off = np.zeros(int(n_ref.value) + 1, dtype=np.uint64)
            self.reference_lengths = np.zeros(int(n_ref.value), dtype=np.uint32)
            _lib.check(self._lib.gbrs_bam_references(self._h, _lib.ptr(buf), buf.size, _lib.ptr(off),
                                                     _lib.ptr(self.reference_lengths)))
            raw = buf.tobytes()
            self.references = [raw[int(off[k]):int(off[k + 1])].decode('latin-1') for k in range(int(n_ref.value))]
        except BaseException:
            self.close()
            raise

    def close(self):
        if self._h:
            self._lib.gbrs_bam_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def scan_records(self):
        """(refID int32[n], flag uint32[n], names list[bytes]) of every record in file order, on the host: for small
        files and tests."""
        n, nb = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.gbrs_bam_scan_records(self._h, 0, None, None, None, None, 0, C.byref(n), C.byref(nb)))
        cap = int(n.value)
        refid = np.zeros(cap, dtype=np.int32)
        flag = np.zeros(cap, dtype=np.uint32)
        off = np.zeros(cap + 1, dtype=np.uint64)
        buf = np.zeros(max(int(nb.value), 1), dtype=np.uint8)
        _lib.check(self._lib.gbrs_bam_scan_records(self._h, cap, _lib.ptr(refid), _lib.ptr(flag), _lib.ptr(off),
                                                   _lib.ptr(buf), buf.size, C.byref(n), C.byref(nb)))
        raw = buf.tobytes()
        return refid, flag, [raw[int(off[k]):int(off[k + 1])] for k in range(cap)]

    def reference_map(self, haplotypes, loci, delim='_'):
        """(hname, hap uint32[n_ref], locus uint32[n_ref]): where every reference sequence of the header goes
        (AlignmentMatrixFactory.py:57-71).  A sequence that cannot be placed is marked with the reason instead of
        raising: the reference only looks at the sequences that kept records use, and so does the device."""
        hname = list(haplotypes) if len(haplotypes) > 0 else ['h0']
        hid = {}
        for k, h in enumerate(hname):
            hid[h] = k                                   # a repeated name: the last one, as dict.fromkeys + the file table
        lid = dict(zip(loci, range(len(loci))))
        n = len(self.references)
        hap = np.full(n, _UNUSABLE, dtype=np.uint32)
        loc = np.zeros(n, dtype=np.uint32)
        for k, ref in enumerate(self.references):
            if len(haplotypes) > 0:
                parts = ref.split(delim)
                if len(parts) != 2:
                    loc[k] = _NOT_TWO_PARTS
                    continue
                locus, h = parts
                if h not in hid:
                    loc[k] = _UNKNOWN_HAPLOTYPE
                    continue
            else:
                locus, h = ref, hname[0]
            if locus not in lid:
                loc[k] = _UNKNOWN_LOCUS
                continue
            hap[k] = hid[h]
            loc[k] = lid[locus]
        return hname, hap, loc

    def convert(self, hap, loc, num_haps, num_loci, device=0, stage_times=None):
        """-> (indptr list, indices list, rname bytes array [R]) on device `device`."""
        lib = self._lib
        hap = np.ascontiguousarray(hap, dtype=np.uint32)
        loc = np.ascontiguousarray(loc, dtype=np.uint32)
        _lib.check(lib.gbrs_bam_set_reference_map(self._h, len(hap), _lib.ptr(hap), _lib.ptr(loc), num_haps, num_loci))
        R, width = C.c_uint64(0), C.c_uint32(1)
        nnz = np.zeros(num_haps, dtype=np.uint64)
        secs = np.zeros(3, dtype=np.float64)
        _lib.check(lib.gbrs_bam_convert(self._h, device, C.byref(R), C.byref(width), _lib.ptr(nnz), _lib.ptr(secs)))
        if stage_times is not None:
            stage_times['read'], stage_times['rank'], stage_times['build'] = (float(x) for x in secs)
        ip = [np.zeros(num_loci + 1, dtype=np.uint32) for _ in range(num_haps)]
        ix = [np.zeros(int(nnz[k]), dtype=np.uint32) for k in range(num_haps)]
        rname = np.zeros(int(R.value), dtype=f'S{int(width.value)}')
        _lib.check(lib.gbrs_bam_get(self._h, _lib.ptr_table(ip), _lib.ptr_table(ix), _lib.ptr(rname) if R.value else None))
        return ip, ix, rname


def bam_to_matrix(alignment_file, haplotypes, loci, delim='_', device=0, stage_times=None, threads=0):
    """BAM file -> AlignmentPropertyMatrix with read names (rules of the module docstring of bam2emase())."""
    if len(loci) >= 1 << 32:
        raise RuntimeError('2^32 or more loci do not fit uint32 index arrays.')
    with BamFile(alignment_file, threads=threads) as bam:
        hname, hap, loc = bam.reference_map(haplotypes, loci, delim)
        ip, ix, rname = bam.convert(hap, loc, len(hname), len(loci), device=device, stage_times=stage_times)
    if len(rname) == 0:
        raise RuntimeError(f'{alignment_file} holds no alignment records.')
    return AlignmentPropertyMatrix(shape=(len(loci), len(hname), len(rname)), indptr=ip, indices=ix,
                                   haplotype_names=hname, locus_names=loci, read_names=rname)


def _download_classes(lib, e, hname, loci):
    """The classes of a gbrs_ecset as an AlignmentPropertyMatrix with counts."""
    L, H = len(loci), len(hname)
    R, G = C.c_uint64(0), C.c_uint64(0)
    nnz = np.zeros(H, dtype=np.uint64)
    _lib.check(lib.gbrs_ecset_sizes(e, C.byref(R), C.byref(G), _lib.ptr(nnz)))
    ip = [np.zeros(L + 1, dtype=np.uint32) for _ in range(H)]
    ix = [np.zeros(int(nnz[k]), dtype=np.uint32) for k in range(H)]
    count = np.zeros(int(G.value), dtype=np.float64)
    _lib.check(lib.gbrs_ecset_get(e, _lib.ptr_table(ip), _lib.ptr_table(ix), _lib.ptr(count) if G.value else None))
    return AlignmentPropertyMatrix(shape=(L, H, max(int(G.value), 1)), indptr=ip, indices=ix,
                                   count=count if G.value else np.zeros(1), haplotype_names=hname, locus_names=loci)


def bam_to_classes(alignment_files, haplotypes, loci, delim='_', device=0, stage_times=None, threads=0):
    """BAM file(s) -> AlignmentPropertyMatrix of equivalence classes with counts: what bam_to_matrix on every file
    followed by compress over the files' reads, one file after the other, gives (the same name in two files is
    two reads).  Only the class matrix leaves the device.  stage_times gets read / rank / classes, summed over the
    files."""
    if len(loci) >= 1 << 32:
        raise RuntimeError('2^32 or more loci do not fit uint32 index arrays.')
    lib = _lib.load()
    hname = list(haplotypes) if len(haplotypes) > 0 else ['h0']
    L, H = len(loci), len(hname)
    total = np.zeros(3, dtype=np.float64)
    e = C.c_void_p()
    _lib.check(lib.gbrs_ecset_create(L, H, device, C.byref(e)))
    try:
        for path in alignment_files:
            with BamFile(path, threads=threads) as bam:
                _, hap, loc = bam.reference_map(haplotypes, loci, delim)
                _lib.check(lib.gbrs_bam_set_reference_map(bam._h, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L))
                n, secs = C.c_uint64(0), np.zeros(3, dtype=np.float64)
                _lib.check(lib.gbrs_ecset_add_bam(e, bam._h, C.byref(n), _lib.ptr(secs)))
                total += secs
            if n.value == 0:
                raise RuntimeError(f'{path} holds no alignment records.')
        ec = _download_classes(lib, e, hname, loci)
    finally:
        lib.gbrs_ecset_destroy(e)
        if stage_times is not None:
            stage_times['read'], stage_times['rank'], stage_times['classes'] = (float(x) for x in total)
    return ec


def paired_bam_to_classes(alignment_files, mate_files, haplotypes, loci, delim='_', device=0, stage_times=None, threads=0):
    """Paired-end BAM files, aligned one end at a time -> AlignmentPropertyMatrix of equivalence classes with counts:
    what bam_to_matrix on both ends of every pair, get_common_alignments on the two and compress over the pairs'
    results, one pair after the other, give.  mate_files[k] is the second end of alignment_files[k].  Both ends of
    a pair must name the same reads (no suffix is stripped), else ValueError with the reference's sentence; an
    alignment is kept iff both ends have it, and a read left without any is a read of the empty class.  Only the
    class matrix leaves the device.  stage_times gets read / rank / common / classes, summed over the pairs."""
    if len(loci) >= 1 << 32:
        raise RuntimeError('2^32 or more loci do not fit uint32 index arrays.')
    if len(alignment_files) != len(mate_files):
        raise RuntimeError(f'{len(alignment_files)} BAM file(s) but {len(mate_files)} mate file(s): every BAM file '
                           'needs its second end.')
    lib = _lib.load()
    hname = list(haplotypes) if len(haplotypes) > 0 else ['h0']
    L, H = len(loci), len(hname)
    total = np.zeros(4, dtype=np.float64)
    e = C.c_void_p()
    _lib.check(lib.gbrs_ecset_create(L, H, device, C.byref(e)))
    try:
        for path, mate in zip(alignment_files, mate_files):
            with BamFile(path, threads=threads) as first, BamFile(mate, threads=threads) as second:
                _, hap, loc = first.reference_map(haplotypes, loci, delim)
                _lib.check(lib.gbrs_bam_set_reference_map(first._h, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L))
                if second.references != first.references:      # (two ends aligned to one index share the header's list)
                    _, hap, loc = second.reference_map(haplotypes, loci, delim)
                _lib.check(lib.gbrs_bam_set_reference_map(second._h, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L))
                n, secs = C.c_uint64(0), np.zeros(4, dtype=np.float64)
                status = lib.gbrs_ecset_add_bam_pair(e, first._h, second._h, C.byref(n), _lib.ptr(secs))
                total += secs
                if status == _lib.GBRS_ERR_INVALID:
                    msg = lib.gbrs_last_error().decode(errors='replace')
                    if msg.startswith(_INCOMPATIBLE):
                        logger.error(msg)
                        raise ValueError(msg)
                _lib.check(status)
            if n.value == 0:
                raise RuntimeError(f'{path} and {mate} hold no alignment records.')
        ec = _download_classes(lib, e, hname, loci)
    finally:
        lib.gbrs_ecset_destroy(e)
        if stage_times is not None:
            for k, name in enumerate(('read', 'rank', 'common', 'classes')):
                stage_times[name] = float(total[k])
    return ec


def bam2ec(alignment_files, haplotypes, locusid_file, output_file, delim='_', comp_lib='zlib', index_dtype='uint32',
           device=0, stage_times=None):
    """BAM file(s) -> the equivalence-class file of `gbrs compress` in one pass (extension): member for member what
    bam2emase() on every file and compress() over the results write, with the rules of bam2emase() per file and
    the files' reads one after the other.  No intermediate file, no read names, no CPU fallback."""
    for x in alignment_files:
        logger.info(f'BAM File: {x}')
    logger.info(f'Locus ID File: {locusid_file}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Haplotypes: {haplotypes}')
    logger.info(f'Delimiter: {delim}')
    logger.info(f'Index dtype: {index_dtype}')
    logger.info(f'Compression Library: {comp_lib}')
    if np.dtype(index_dtype) != np.uint32:
        raise RuntimeError(f'--index-dtype {index_dtype}: the index arrays of this implementation are uint32.')
    if len(alignment_files) == 0:
        raise RuntimeError('No BAM file was given.')
    init = _lib.warm_up_device_async(device)          # the runtime starts while the first file is inflated
    logger.info(f'Parsing Locus ID File: {locusid_file}')
    loci = get_names(locusid_file)
    for x in alignment_files:
        logger.info(f'Parsing BAM File: {x}')
    ec = bam_to_classes(list(alignment_files), list(haplotypes), loci, delim=delim, device=device,
                        stage_times=stage_times)
    init.join()
    logger.debug(f'Number Loci: {ec.num_loci}')
    logger.debug(f'Number Haplotypes: {ec.num_haplotypes}')
    logger.debug(f'Number ECs: {ec.num_reads}')
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    t0 = time.time()
    ec.save(output_file, complib=comp_lib)
    if stage_times is not None:
        stage_times['write'] = time.time() - t0
    logger.info('Done')


def bam2ec_paired(alignment_files, mate_files, haplotypes, locusid_file, output_file, delim='_', comp_lib='zlib',
                  index_dtype='uint32', device=0, stage_times=None):
    """`gbrs bam2ec --mate-file`: paired-end BAM file(s), aligned one end at a time -> the equivalence-class file
    in one pass: member for member what bam2emase() on both ends, get_common_alignments() on the two and compress()
    over the pairs write (rules of paired_bam_to_classes).  No intermediate file, no CPU fallback."""
    for x in alignment_files:
        logger.info(f'BAM File: {x}')
    for x in mate_files:
        logger.info(f'Mate BAM File: {x}')
    logger.info(f'Locus ID File: {locusid_file}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Haplotypes: {haplotypes}')
    logger.info(f'Delimiter: {delim}')
    logger.info(f'Index dtype: {index_dtype}')
    logger.info(f'Compression Library: {comp_lib}')
    if np.dtype(index_dtype) != np.uint32:
        raise RuntimeError(f'--index-dtype {index_dtype}: the index arrays of this implementation are uint32.')
    if len(alignment_files) == 0:
        raise RuntimeError('No BAM file was given.')
    if len(alignment_files) != len(mate_files):
        raise RuntimeError(f'{len(alignment_files)} BAM file(s) but {len(mate_files)} mate file(s): every BAM file '
                           'needs its second end.')
    init = _lib.warm_up_device_async(device)          # the runtime starts while the first file is inflated
    logger.info(f'Parsing Locus ID File: {locusid_file}')
    loci = get_names(locusid_file)
    for x, y in zip(alignment_files, mate_files):
        logger.info(f'Parsing BAM Files: {x} + {y}')
    ec = paired_bam_to_classes(list(alignment_files), list(mate_files), list(haplotypes), loci, delim=delim,
                               device=device, stage_times=stage_times)
    init.join()
    logger.debug(f'Number Loci: {ec.num_loci}')
    logger.debug(f'Number Haplotypes: {ec.num_haplotypes}')
    logger.debug(f'Number ECs: {ec.num_reads}')
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    t0 = time.time()
    ec.save(output_file, complib=comp_lib)
    if stage_times is not None:
        stage_times['write'] = time.time() - t0
    logger.info('Done')


def bam2emase(alignment_file, haplotypes, locusid_file, output_file='alignments.transcriptome.h5', delim='_',
              index_dtype='uint32', data_dtype='uint8', device=0, stage_times=None):
    """Convert a BAM file to the EMASE format (emase/emase_utils.py:26-70).

    * loci: first field of every line of `locusid_file`, duplicates dropped; haplotypes as given, or the single
      haplotype `h0` (then a reference sequence's whole name is its locus);
    * read ids: rank of the read's name among the distinct names of ALL records, unmapped ones included, in the
      order of sorted(); a read without any kept record still has its (empty) row;
    * kept records: those whose flag word is neither exactly 4 nor exactly 8.  This is the reference's test
      (`aln.flag != 4 and aln.flag != 8`, AlignmentMatrixFactory.py:60): an equality on the whole word, not a
      test of the `unmapped` bit, so e.g. flag 20 (4 + 16) is kept and must name a reference sequence;
    * a kept record without a reference sequence, or with one that does not split at `delim` into exactly
      (locus, haplotype) with both known, raises RuntimeError naming it; sequences no kept record uses are
      never looked at;
    * per haplotype coo_matrix((ones, (read, locus))).tocsc(): duplicates stored once, read ids ascending in a
      column; written with incidence_only=True, /lname and /rname, no /count.  `data_dtype` is accepted and
      unused, as in the reference; `index_dtype` must be uint32.  No temporary files.
    """
    logger.info(f'BAM File: {alignment_file}')
    logger.info(f'Locus ID File: {locusid_file}')
    logger.info(f'Output File: {output_file}')
    logger.info(f'Haplotypes: {haplotypes}')
    logger.info(f'Delimiter: {delim}')
    logger.info(f'Index dtype: {index_dtype}')
    logger.info(f'Data dtype: {data_dtype}')
    if np.dtype(index_dtype) != np.uint32:
        raise RuntimeError(f'--index-dtype {index_dtype}: the index arrays of this implementation are uint32.')
    if output_file is None:
        output_file = 'alignments.transcriptome.h5'
    init = _lib.warm_up_device_async(device)          # the runtime starts while the file is inflated
    logger.info(f'Parsing Locus ID File: {locusid_file}')
    loci = get_names(locusid_file)
    logger.info(f'Parsing BAM File: {alignment_file}')
    apm = bam_to_matrix(alignment_file, list(haplotypes), loci, delim=delim, device=device, stage_times=stage_times)
    init.join()
    logger.debug(f'Number Loci: {apm.num_loci}')
    logger.debug(f'Number Haplotypes: {apm.num_haplotypes}')
    logger.debug(f'Number Reads: {apm.num_reads}')
    logger.info(f'Saving EMASE Formatted File: {output_file}')
    t0 = time.time()
    if str(output_file).endswith('.npz'):
        apm.save_npz(output_file)
    else:
        apm.save(output_file, title='Alignments')
    if stage_times is not None:
        stage_times['write'] = time.time() - t0
    logger.info('Done')
