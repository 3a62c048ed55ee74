"""Host side of `gbrs bam2ec` (no device needed): the argument parser, the function signatures, a hand-checked
answer of the restatement the GPU tests compare against, and the rule that there is no CPU fallback."""
import ctypes as C
import inspect
import logging
import os

import numpy as np
import pytest

from gbrs_amd import _lib
from test_bam2emase_cpu import KNOWN, _write


def _inputs(tmp_path):
    return (_write(tmp_path, 'a.bam', KNOWN), _write(tmp_path, 'b.bam', KNOWN), _write(tmp_path, 'ids.tsv', b'g1\ng2\n'))


def test_argument_parser(tmp_path, capsys):
    from gbrs_amd.cli import build_parser
    a_bam, b_bam, ids = _inputs(tmp_path)
    ap = build_parser()
    a = ap.parse_args(['bam2ec', '-i', a_bam, '-m', ids, '-o', 'o.h5'])
    assert a.command == 'bam2ec' and a.alignment_files == [os.path.realpath(a_bam)]
    assert a.haplotypes is None and a.output_file == 'o.h5' and a.locusid_file == os.path.realpath(ids)
    assert (a.delim, a.comp_lib, a.index_dtype, a.verbose, a.device) == ('_', 'zlib', 'uint32', 0, 0)
    # -i repeats; one option may hold a comma list, which is passed on as it is and split by the command
    a = ap.parse_args(['bam2ec', '-i', a_bam, '--alignment-file', b_bam, '-m', ids, '-o', 'o.npz', '-h', 'A,B', '-h', 'C'])
    assert a.alignment_files == [os.path.realpath(a_bam), os.path.realpath(b_bam)] and a.haplotypes == ['A,B', 'C']
    both = a_bam + ',' + b_bam
    a = ap.parse_args(['bam2ec', '-i', both, '-i', a_bam, '--locus-ids', ids, '--output', 'o.h5', '--haplotype-char', 'X',
                       '-d', '.', '-c', 'lzo', '--index-dtype', 'uint64', '-vv', '--device', '3'])
    assert a.alignment_files == [both, os.path.realpath(a_bam)]
    assert (a.haplotypes, a.delim, a.comp_lib, a.index_dtype, a.verbose, a.device) == (['X'], '.', 'lzo', 'uint64', 2, 3)
    # -o is required; a missing file given alone is the parser's error
    for argv in (['bam2ec', '-i', a_bam, '-m', ids],
                 ['bam2ec', '-i', str(tmp_path / 'nope.bam'), '-m', ids, '-o', 'o.h5'],
                 ['bam2ec', '-m', ids, '-o', 'o.h5']):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(argv)
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(['bam2ec', '--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--haplotype-char' in out and '--alignment-file' in out and '--comp-lib' in out
    with pytest.raises(SystemExit) as e:
        ap.parse_args(['--help'])
    assert e.value.code == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.strip().startswith('bam2ec')]
    assert line and '(extension)' in line[0]


def test_missing_file_in_a_comma_list_is_logged(tmp_path, caplog):
    from gbrs_amd import cli
    a_bam, _, ids = _inputs(tmp_path)
    out = str(tmp_path / 'o.npz')
    missing = str(tmp_path / 'nope.bam')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', a_bam + ',' + missing, '-m', ids, '-o', out, '-h', 'A,B']) == 0
    assert any(f"File '{missing}' does not exist." in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def test_function_signatures():
    from gbrs_amd.bam2emase import bam2ec, bam_to_classes
    p = inspect.signature(bam_to_classes).parameters
    assert list(p) == ['alignment_files', 'haplotypes', 'loci', 'delim', 'device', 'stage_times', 'threads']
    assert (p['delim'].default, p['device'].default, p['stage_times'].default, p['threads'].default) == ('_', 0, None, 0)
    p = inspect.signature(bam2ec).parameters
    assert list(p) == ['alignment_files', 'haplotypes', 'locusid_file', 'output_file', 'delim', 'comp_lib', 'index_dtype',
                       'device', 'stage_times']
    assert p['output_file'].default is inspect.Parameter.empty
    assert (p['delim'].default, p['comp_lib'].default, p['index_dtype'].default, p['device'].default,
            p['stage_times'].default) == ('_', 'zlib', 'uint32', 0, None)


def test_index_dtype_other_than_uint32_is_refused(tmp_path):
    from gbrs_amd.bam2emase import bam2ec
    a_bam, _, ids = _inputs(tmp_path)
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError, match='index-dtype'):
        bam2ec([a_bam], ['A', 'B'], ids, out, index_dtype='uint64')
    assert not os.path.exists(out)


def test_restatement_known_answer():
    """Two files, haplotypes A, B, loci g1, g2.
    File 1 (names sort r1 < r2 < r3): r2 on g1_A and g1_B, r1 on g2_A, r3 unmapped.
    File 2 (x < y): x on g2_A - the class of r1 -, y on g1_B twice - a class of its own.
    Reads in order r1 r2 r3 x y, so the classes in first-seen order are
        0 {A: g2} x 2,  1 {A: g1, B: g1} x 1,  2 {} x 1,  3 {B: g1} x 1."""
    from bam2ec_restate import restate_classes
    refs = ['g1_A', 'g1_B', 'g2_A']
    f1 = dict(ref_names=refs, names=['r2', 'r2', 'r1', 'r3'], refids=[0, 1, 2, -1], flags=[0, 256, 16, 4])
    f2 = dict(ref_names=refs, names=['y', 'x', 'y'], refids=[1, 2, 1], flags=[0, 0, 256])
    w = restate_classes([f1, f2], ['A', 'B'], ['g1', 'g2'])
    assert w['shape'] == (2, 2, 4) and w['num_reads'] == 5 and w['num_ecs'] == 4
    assert w['hname'] == ['A', 'B'] and w['lname'] == ['g1', 'g2']
    assert w['count'].dtype == np.float64 and w['count'].tolist() == [2.0, 1.0, 1.0, 1.0]
    assert w['indptr'][0].tolist() == [0, 1, 2] and w['indices'][0].tolist() == [1, 0]
    assert w['indptr'][1].tolist() == [0, 2, 2] and w['indices'][1].tolist() == [1, 3]
    assert all(a.dtype == np.uint32 for a in w['indptr'] + w['indices'])
    # the same name in both files is two reads: file 1 twice doubles every count and changes nothing else
    w2 = restate_classes([f1, f1], ['A', 'B'], ['g1', 'g2'])
    assert w2['num_reads'] == 6 and w2['count'].tolist() == [2.0, 2.0, 2.0]
    # no -h: the whole reference name is the locus, one haplotype h0
    w3 = restate_classes([f1], [], refs)
    assert w3['hname'] == ['h0'] and w3['shape'] == (3, 1, 3) and w3['count'].tolist() == [1.0, 1.0, 1.0]
    assert w3['indptr'][0].tolist() == [0, 1, 2, 3] and w3['indices'][0].tolist() == [1, 1, 0]


def test_no_cpu_fallback(tmp_path, hip_lib):
    from gbrs_amd.bam2emase import bam2ec, bam_to_classes
    if hip_lib.gbrs_device_count() > 0:
        pytest.skip("a HIP device is visible")
    a_bam, _, ids = _inputs(tmp_path)
    with pytest.raises(_lib.GbrsHipError) as e:
        bam_to_classes([a_bam], ['A', 'B'], ['g1', 'g2'])
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
    out = str(tmp_path / 'o.npz')
    with pytest.raises(_lib.GbrsHipError) as e:
        bam2ec([a_bam], ['A', 'B'], ids, out)
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
    assert not os.path.exists(out)
    h = C.c_void_p()
    assert hip_lib.gbrs_ecset_create(2, 2, 0, C.byref(h)) == _lib.GBRS_ERR_NO_DEVICE
    assert not h.value


def test_argument_checks_need_no_device(hip_lib):
    """NULL and out-of-range arguments are refused before a device is looked for."""
    h = C.c_void_p()
    assert hip_lib.gbrs_ecset_create(2, 2, 0, None) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_ecset_create(2, 17, 0, C.byref(h)) == _lib.GBRS_ERR_INVALID       # compress: H <= 16
    assert hip_lib.gbrs_ecset_create(1 << 27, 2, 0, C.byref(h)) == _lib.GBRS_ERR_INVALID  # compress: L < 2^27
    assert hip_lib.gbrs_ecset_create(0, 2, 0, C.byref(h)) == _lib.GBRS_ERR_INVALID
    n = C.c_uint64(0)
    nnz = np.zeros(2, dtype=np.uint64)
    assert hip_lib.gbrs_ecset_add_bam(None, None, C.byref(n), None) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_ecset_sizes(None, C.byref(n), C.byref(n), _lib.ptr(nnz)) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_ecset_get(None, None, None, None) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_ecset_destroy(None) == _lib.GBRS_OK
