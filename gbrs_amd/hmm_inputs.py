"""`gbrs get-transition-prob` and `gbrs get-alignment-spec` on MI355X: the transition tables, the gene order and the
alignment specificity blocks that `gbrs reconstruct` reads (gbrs/gbrs_utils.py:208-294, :297-379; flags of
gbrs/commands.py:282-339).  Same inputs, files and log lines as the reference; the arithmetic - nine logarithm
differences per marker interval, an S x S block per gene - runs in HIP kernels through include/gbrs_hip.h
(gbrs_ri_transition_tables, gbrs_alignment_spec).  No CPU fallback: without libgbrs_hip.so / a gfx950 device both
commands raise.

Deliberate deviations:
  * `RI` with a haplotype count other than 2 is a RuntimeError (the reference writes NaN into all but nine entries);
  * `F2`, `CC` and `DO` raise NotImplementedError naming the scheme (stubs in the reference, which fail with a
    TypeError); any other scheme raises the reference's ValueError;
  * all three are checked before any file is written (the reference writes the gene-position file first).
get_alignment_spec follows the reference with its two Python-2 idioms restored (`dtype=str` for the gene list, the
`map` result taken as a list): as written it does not run under Python 3.
"""
from __future__ import annotations

import io
import logging
import os
import time
from collections import defaultdict

import numpy as np

from . import _lib
from .npzfast import savez_compressed

logger = logging.getLogger('gbrs')

UNIMPLEMENTED_SCHEMES = ('F2', 'CC', 'DO')


def check_mating_scheme(mating_scheme, haplotypes):
    """The three refusals of get_transition_prob, made before any file is touched."""
    if mating_scheme == 'RI':
        if len(haplotypes) != 2:
            raise RuntimeError(f'Mating scheme RI is defined for two haplotypes, not {len(haplotypes)}: '
                               f'{",".join(haplotypes)}')
    elif mating_scheme in UNIMPLEMENTED_SCHEMES:
        raise NotImplementedError(f'Mating scheme {mating_scheme} is not implemented: only RI has a step function.')
    else:
        raise ValueError(f'Unknown mating scheme: {mating_scheme}')


def parse_marker_text(text):
    """{chromosome: [(id, cM)]}, {chromosome: [(id, position)]} of a marker file's text: tab-separated
    `id, chromosome, position, cM` lines without a header.  Chromosomes in order of first appearance, markers in file
    order (gbrs_utils.py:245-251); a malformed line raises what float() / int() / indexing raise."""
    locs, gpos = defaultdict(list), defaultdict(list)
    for line in io.StringIO(text):
        item = line.rstrip().split('\t')
        locs[item[1]].append((item[0], float(item[3])))
        gpos[item[1]].append((item[0], int(item[2])))
    return dict(locs), dict(gpos)


def ri_transition_tables(positions, is_x, gamma_scale, epsilon, device=0):
    """positions: one float64 array of cM positions per chromosome -> one (n_c - 1, 3, 3) table per chromosome, made
    by one call of gbrs_ri_transition_tables."""
    sizes = np.array([len(p) for p in positions], dtype=np.int64)
    chrom_ptr = np.zeros(len(positions) + 1, dtype=np.int64)
    np.cumsum(sizes, out=chrom_ptr[1:])
    cm = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64) for p in positions])
                              if len(positions) else np.zeros(0), dtype=np.float64)
    flags = np.ascontiguousarray(is_x, dtype=np.uint8)
    steps = np.maximum(sizes - 1, 0)
    out = np.empty((int(steps.sum()), 3, 3), dtype=np.float64)
    _lib.check(_lib.load().gbrs_ri_transition_tables(_lib.ptr(cm), _lib.ptr(chrom_ptr), _lib.ptr(flags), len(positions),
                                                     float(gamma_scale), float(epsilon), int(device), _lib.ptr(out)))
    ends = np.cumsum(steps)
    return [out[e - n:e] for e, n in zip(ends, steps)]


def get_transition_prob(marker_file: str, haplotypes: str = 'A,B', mating_scheme: str = 'RI', gamma_scale: float = 0.01,
                        epsilon: float = 0.000001, output_file: str = 'tranprob.npz', device: int = 0,
                        stage_times: dict = None) -> None:
    """`gbrs get-transition-prob`: the log transition tables between neighbouring markers, one (n - 1, 3, 3) member per
    chromosome, into $GBRS_DATA/<output_file>, and the markers' order into $GBRS_DATA/ref.gene_pos.ordered.npz."""
    clock = time.perf_counter
    marks = stage_times if stage_times is not None else {}
    data_dir = os.getenv('GBRS_DATA', '.')
    logger.info(f'Marker File: {marker_file}')
    logger.info(f'Haplotypes: {haplotypes}')
    logger.info(f'Mating Scheme: {mating_scheme}')
    logger.info(f'Gama Scale: {gamma_scale}')
    logger.info(f'Epsilon: {epsilon}')
    logger.info(f'Output File: {output_file}')
    check_mating_scheme(mating_scheme, haplotypes.split(','))

    _lib.warm_up_device_async(device)
    t0 = clock()
    logger.info(f'Loading marker file: {marker_file}')
    with open(marker_file) as fh:
        locs_by_chro, gpos_by_chro = parse_marker_text(fh.read())
    chroms = list(locs_by_chro)
    marks['load'] = clock() - t0

    t0 = clock()
    for c in chroms:
        logger.debug(f'Working on {c}')
    tables = ri_transition_tables([np.array([e[1] for e in locs_by_chro[c]], dtype=np.float64) for c in chroms],
                                  [c == 'X' for c in chroms], gamma_scale, epsilon, device)
    marks['device'] = clock() - t0

    t0 = clock()
    gpos_file = os.path.join(data_dir, 'ref.gene_pos.ordered.npz')
    logger.info(f'Saving {gpos_file}')
    np.savez_compressed(gpos_file, **gpos_by_chro)
    logger.info(f'Saving {os.path.join(data_dir, output_file)}')
    savez_compressed(os.path.join(data_dir, output_file), dict(zip(chroms, tables)))
    marks['save'] = clock() - t0
    logger.info('Done')


def read_sample_list(text):
    """{strain: [report paths in file order]} of a sample file's text (`strain TAB path` lines, gbrs_utils.py:328-333)."""
    flist = defaultdict(list)
    for line in io.StringIO(text):
        item = line.rstrip().split('\t')
        flist[item[0]].append(item[1])
    return dict(flist)


def read_report_table(tpmfile, gid, num_genes, num_strains):
    """The (genes x strains) table one report contributes (gbrs_utils.py:340-352): the header line is skipped, a line
    gives float() of its fields 1 .. S to its gene's row, a gene the list does not know is ignored, a gene missing
    from the file keeps zeros and a gene listed twice takes its last line.  A plain table's numbers go through one
    C-level parse (gbrs_parse_number_table), anything else line by line."""
    table = np.zeros((num_genes, num_strains))
    with open(tpmfile) as fh:
        fh.readline()
        body = fh.read()
    lines = body.splitlines()
    if not lines:
        return table
    width = lines[0].rstrip().count('\t')
    if width >= num_strains and len(lines) == body.count('\n') + (0 if body.endswith('\n') else 1):
        raw = body.encode()
        numbers = np.empty((len(lines), width), dtype=np.float64)
        try:
            status = _lib.load().gbrs_parse_number_table(raw, len(raw), len(lines), width, _lib.ptr(numbers))
        except (ImportError, OSError):
            status = 1
        if status == 0:
            rows = np.fromiter((gid.get(line.partition('\t')[0], -1) for line in lines), dtype=np.int64, count=len(lines))
            known = np.flatnonzero(rows >= 0)
            table[rows[known]] = numbers[known, :num_strains]  # a gene listed twice takes its last line
            return table
    for curline in io.StringIO(body):
        item = curline.rstrip().split('\t')
        if item[0] in gid:
            table[gid[item[0]], :] = list(map(float, item[1:(num_strains + 1)]))
    return table


def alignment_spec_arrays(tables, strain_ptr, strain_div, num_genes, num_strains, min_expr, device=0):
    """(axes [G, S, S], ases [G, S], avecs [G, S, S], has_avec [G]) through gbrs_alignment_spec.  tables: [F, G, S],
    the files that exist, strain by strain; strain_div: the files every strain lists."""
    G, S = int(num_genes), int(num_strains)
    tables = np.ascontiguousarray(tables, dtype=np.float64)
    strain_ptr = np.ascontiguousarray(strain_ptr, dtype=np.int64)
    strain_div = np.ascontiguousarray(strain_div, dtype=np.int64)
    axes, ases, avecs = np.empty((G, S, S)), np.empty((G, S)), np.empty((G, S, S))
    has_avec = np.zeros(G, dtype=np.uint8)
    _lib.check(_lib.load().gbrs_alignment_spec(_lib.ptr(tables) if tables.size else None, _lib.ptr(strain_ptr),
                                               _lib.ptr(strain_div), G, S, float(min_expr), int(device), _lib.ptr(axes),
                                               _lib.ptr(ases), _lib.ptr(avecs), _lib.ptr(has_avec)))
    return axes, ases, avecs, has_avec


def get_alignment_spec(sample_file: str, haplotypes: list, min_expr: float = 2.0, device: int = 0,
                       stage_times: dict = None) -> None:
    """`gbrs get-alignment-spec`: from the genes.tpm reports of the founder strains' own samples, per gene the mean
    TPM of every strain on every haplotype (axes.npz), its sum per strain (ases.npz) and, for genes some strain
    expresses above min_expr, the unit vectors `gbrs reconstruct` compares a sample with (avecs.npz); all three in
    $GBRS_DATA, keyed by gene id."""
    clock = time.perf_counter
    marks = stage_times if stage_times is not None else {}
    data_dir = os.getenv('GBRS_DATA', '.')
    logger.info(f'Sample File: {sample_file}')
    logger.info(f'Haplotypes: {haplotypes}')
    logger.info(f'Min Expression: {min_expr}')
    num_strains = len(haplotypes)

    _lib.warm_up_device_async(device)
    t0 = clock()
    gene_file = os.path.join(data_dir, 'ref.gene2transcripts.tsv')
    logger.info(f'Loading {gene_file}')
    gname = np.loadtxt(gene_file, usecols=(0,), dtype=str)
    num_genes = len(gname)
    gid = dict(zip(gname.tolist(), range(num_genes)))
    logger.info(f'Loading {sample_file}')
    with open(sample_file) as fh:
        flist = read_sample_list(fh.read())
    tables, strain_ptr, strain_div = [], [0], []
    for st in haplotypes:
        for tpmfile in flist[st]:                              # KeyError: a strain without a line
            logger.debug(f'Working on {tpmfile}')
            if not os.path.isfile(tpmfile):
                print(f'File {tpmfile} does not exist.')
                continue
            tables.append(read_report_table(tpmfile, gid, num_genes, num_strains))
        strain_ptr.append(len(tables))
        strain_div.append(len(flist[st]))
    stacked = np.stack(tables) if tables else np.zeros((0, num_genes, num_strains))
    marks['load'] = clock() - t0

    t0 = clock()
    axes, ases, avecs, has_avec = alignment_spec_arrays(stacked, strain_ptr, strain_div, num_genes, num_strains,
                                                        min_expr, device)
    marks['device'] = clock() - t0

    t0 = clock()
    genes = gname.tolist()
    for name, members in (('axes.npz', {g: axes[gid[g]] for g in genes}),
                          ('ases.npz', {g: ases[gid[g]][None, :] for g in genes}),
                          ('avecs.npz', {g: avecs[gid[g]] for g in genes if has_avec[gid[g]]})):
        path = os.path.join(data_dir, name)
        logger.info(f'Saving {path}')
        if len(members) > 0xFFFF:
            np.savez_compressed(path, **members)               # more members than the plain zip format holds
        else:
            savez_compressed(path, members)
    marks['save'] = clock() - t0
