"""Host side of `gbrs bam2ec --mate-file` (no device needed): the argument parser, the function signatures,
hand-checked answers of the restatement the GPU tests compare against - its intersection step also against what the
reference's own `A * B` left in tests/golden/matops_*.npz -, and the rule that there is no CPU fallback."""
import ctypes as C
import inspect
import logging
import os

import numpy as np
import pytest

import bam2ec_paired_restate as pr
from conftest import golden_files, load_golden
from gbrs_amd import _lib
from test_bam2emase_cpu import KNOWN, _write
from test_matops_cpu import golden_matrix


def _inputs(tmp_path):
    return (_write(tmp_path, 'a.bam', KNOWN), _write(tmp_path, 'b.bam', KNOWN), _write(tmp_path, 'ids.tsv', b'g1\ng2\n'))


def test_argument_parser(tmp_path, capsys):
    from gbrs_amd.cli import build_parser
    a_bam, b_bam, ids = _inputs(tmp_path)
    ap = build_parser()
    a = ap.parse_args(['bam2ec', '-i', a_bam, '-m', ids, '-o', 'o.h5'])
    assert a.mate_files is None                               # without the option the command is today's
    a = ap.parse_args(['bam2ec', '-i', a_bam, '-I', b_bam, '-m', ids, '-o', 'o.h5'])
    assert a.alignment_files == [os.path.realpath(a_bam)] and a.mate_files == [os.path.realpath(b_bam)]
    # the option repeats under both names; a comma list is passed on as it is and split by the command
    a = ap.parse_args(['bam2ec', '-i', a_bam, '-i', b_bam, '-I', b_bam, '--mate-file', a_bam, '-m', ids, '-o', 'o.npz'])
    assert a.mate_files == [os.path.realpath(b_bam), os.path.realpath(a_bam)]
    both = b_bam + ',' + a_bam
    a = ap.parse_args(['bam2ec', '-i', a_bam + ',' + b_bam, '-i', a_bam, '--mate-file', both, '-I', b_bam, '-m', ids, '-o', 'o'])
    assert a.mate_files == [both, os.path.realpath(b_bam)]
    # a missing file given alone is the parser's error, as for -i
    for opt in ('-I', '--mate-file'):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(['bam2ec', '-i', a_bam, opt, str(tmp_path / 'nope.bam'), '-m', ids, '-o', 'o.h5'])
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(['bam2ec', '--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert '--mate-file' in out and '-I' in out and 'second end' in out


@pytest.mark.parametrize('first,mates', [(['-i', 'A', '-i', 'B'], ['-I', 'B']), (['-i', 'A'], ['-I', 'B,A']),
                                         (['-i', 'A,B', '-i', 'A'], ['-I', 'A', '-I', 'B'])])
def test_count_mismatch_is_logged_and_writes_nothing(tmp_path, caplog, first, mates):
    from gbrs_amd import cli
    a_bam, b_bam, ids = _inputs(tmp_path)
    path = {'A': a_bam, 'B': b_bam}
    put = lambda argv: [x if x.startswith('-') else ','.join(path[k] for k in x.split(',')) for x in argv]
    out = str(tmp_path / 'o.npz')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', *put(first), *put(mates), '-m', ids, '-o', out, '-h', 'A,B']) == 0
    assert any('--mate-file' in r.getMessage() and 'second end' in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def test_missing_mate_in_a_comma_list_is_logged(tmp_path, caplog):
    from gbrs_amd import cli
    a_bam, b_bam, ids = _inputs(tmp_path)
    out = str(tmp_path / 'o.npz')
    missing = str(tmp_path / 'nope.bam')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', a_bam + ',' + b_bam, '-I', b_bam + ',' + missing, '-m', ids, '-o', out, '-h', 'A,B']) == 0
    assert any(f"File '{missing}' does not exist." in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def test_function_signatures():
    from gbrs_amd.bam2emase import bam2ec_paired, paired_bam_to_classes
    p = inspect.signature(paired_bam_to_classes).parameters
    assert list(p) == ['alignment_files', 'mate_files', 'haplotypes', 'loci', 'delim', 'device', 'stage_times', 'threads']
    assert (p['delim'].default, p['device'].default, p['stage_times'].default, p['threads'].default) == ('_', 0, None, 0)
    p = inspect.signature(bam2ec_paired).parameters
    assert list(p) == ['alignment_files', 'mate_files', 'haplotypes', 'locusid_file', 'output_file', 'delim', 'comp_lib',
                       'index_dtype', 'device', 'stage_times']
    assert p['output_file'].default is inspect.Parameter.empty and p['mate_files'].default is inspect.Parameter.empty
    assert (p['delim'].default, p['comp_lib'].default, p['index_dtype'].default, p['device'].default,
            p['stage_times'].default) == ('_', 'zlib', 'uint32', 0, None)


def test_checks_before_the_device(tmp_path):
    from gbrs_amd.bam2emase import bam2ec_paired, paired_bam_to_classes
    a_bam, b_bam, ids = _inputs(tmp_path)
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError, match='index-dtype'):
        bam2ec_paired([a_bam], [b_bam], ['A', 'B'], ids, out, index_dtype='uint64')
    with pytest.raises(RuntimeError, match='second end'):
        bam2ec_paired([a_bam, b_bam], [b_bam], ['A', 'B'], ids, out)
    with pytest.raises(RuntimeError, match='second end'):
        paired_bam_to_classes([a_bam], [], ['A', 'B'], ['g1', 'g2'])
    with pytest.raises(RuntimeError, match='No BAM file'):
        bam2ec_paired([], [], ['A', 'B'], ids, out)
    assert not os.path.exists(out)


REFS = ['g1_A', 'g1_B', 'g2_A', 'g2_B']


def _six_reads():
    """Haplotypes A, B, loci g1, g2, reads r1 < ... < r6.
        read  first end        second end              common
        r1    g1_A g1_B        g1_A g1_B g2_B          g1_A g1_B
        r2    g1_A g1_B        g1_A (twice)            g1_A
        r3    g2_A             g2_B                    -          (entries in both ends, none in common)
        r4    g2_A g2_B        g2_B g2_A               g2_A g2_B
        r5    unmapped         g1_A                    -
        r6    g1_B             unmapped                -
    The records of either end are not in read order."""
    first = dict(ref_names=REFS, names=['r4', 'r1', 'r6', 'r1', 'r2', 'r3', 'r2', 'r5', 'r4'],
                 refids=[2, 0, 1, 1, 1, 2, 0, -1, 3], flags=[0, 0, 16, 256, 0, 0, 256, 4, 256])
    second = dict(ref_names=REFS, names=['r5', 'r2', 'r1', 'r4', 'r3', 'r1', 'r6', 'r2', 'r4', 'r1'],
                  refids=[0, 0, 3, 3, 3, 0, -1, 0, 2, 1], flags=[0, 0, 0, 16, 0, 256, 4, 256, 256, 256])
    return first, second


def test_restatement_known_answer():
    """Classes of the pair in first-seen order over r1 ... r6:
        0 {A: g1, B: g1} x 1 (r1),  1 {A: g1} x 1 (r2),  2 {} x 3 (r3, r5, r6),  3 {A: g2, B: g2} x 1 (r4)."""
    first, second = _six_reads()
    assert pr.entry_counts(first, second, ['A', 'B'], ['g1', 'g2']) == (8, 8, 5, 1)
    c = pr.restate_pair(first, second, ['A', 'B'], ['g1', 'g2'])
    assert c['shape'] == (2, 2, 6) and c['rname'] == ['r1', 'r2', 'r3', 'r4', 'r5', 'r6']
    assert c['indptr'][0].tolist() == [0, 2, 3] and c['indices'][0].tolist() == [0, 1, 3]
    assert c['indptr'][1].tolist() == [0, 1, 2] and c['indices'][1].tolist() == [0, 3]
    w = pr.restate_classes([(first, second)], ['A', 'B'], ['g1', 'g2'])
    assert w['shape'] == (2, 2, 4) and w['num_reads'] == 6 and w['num_ecs'] == 4
    assert w['hname'] == ['A', 'B'] and w['lname'] == ['g1', 'g2']
    assert w['count'].dtype == np.float64 and w['count'].tolist() == [1.0, 1.0, 3.0, 1.0]
    assert w['indptr'][0].tolist() == [0, 2, 3] and w['indices'][0].tolist() == [0, 1, 3]
    assert w['indptr'][1].tolist() == [0, 1, 2] and w['indices'][1].tolist() == [0, 3]
    assert all(a.dtype == np.uint32 for a in w['indptr'] + w['indices'])
    # the ends the other way round have the same common entries
    v = pr.restate_classes([(second, first)], ['A', 'B'], ['g1', 'g2'])
    assert v['count'].tolist() == w['count'].tolist()
    assert all(v[k][h].tolist() == w[k][h].tolist() for k in ('indptr', 'indices') for h in range(2))
    # a single-end file after the pair: r1 r2 {A: g1, B: g1} -> class 0, r3 {A: g2} new (4), r4 -> 3, r5 {} -> 2,
    # r6 {B: g1} new (5)
    m = pr.restate_classes([(first, second), first], ['A', 'B'], ['g1', 'g2'])
    assert m['num_reads'] == 12 and m['count'].tolist() == [3.0, 1.0, 4.0, 2.0, 1.0, 1.0]
    assert m['indptr'][0].tolist() == [0, 2, 4] and m['indices'][0].tolist() == [0, 1, 3, 4]
    assert m['indptr'][1].tolist() == [0, 2, 3] and m['indices'][1].tolist() == [0, 5, 3]
    # the same pair twice doubles every count
    t = pr.restate_classes([(first, second), (first, second)], ['A', 'B'], ['g1', 'g2'])
    assert t['num_reads'] == 12 and t['count'].tolist() == [2.0, 2.0, 6.0, 2.0]


@pytest.mark.parametrize('path', golden_files('matops'), ids=os.path.basename)
def test_intersection_step_against_the_reference(path):
    """common_entries on the fixture's a and b gives what the reference's get-common-alignments (A * B) wrote."""
    g = load_golden(path)
    R, H, L = int(g['num_rows']), int(g['num_haps']), int(g['num_loci'])
    a, b, want = (golden_matrix(g, k) for k in ('a', 'b', 'common'))
    assert 0 < sum(len(x) for x in want[1]) < min(sum(len(x) for x in a[1]), sum(len(x) for x in b[1]))
    for h in range(H):
        ip, ix = pr.common_entries(L, R, (a[0][h], a[1][h]), (b[0][h], b[1][h]))
        assert ip.dtype == np.uint32 and ix.dtype == np.uint32
        np.testing.assert_array_equal(ip, want[0][h])
        np.testing.assert_array_equal(ix, want[1][h])


@pytest.mark.parametrize('which', ['missing', 'extra', 'last_byte'])
def test_restatement_refuses_incompatible_names(which):
    first, second = _six_reads()
    if which == 'missing':                                   # the second end lacks r5
        keep = [k for k, n in enumerate(second['names']) if n != 'r5']
        second = dict(second, **{f: [second[f][k] for k in keep] for f in ('names', 'refids', 'flags')})
    elif which == 'extra':
        second = dict(second, names=second['names'] + ['r7'], refids=second['refids'] + [-1], flags=second['flags'] + [4])
    else:                                                    # same count, one name differs in its last byte
        second = dict(second, names=[n if n != 'r3' else 'r0' for n in second['names']])
        assert len(set(second['names'])) == 6
    with pytest.raises(ValueError, match="The read ID's are not compatible."):
        pr.restate_classes([(first, second)], ['A', 'B'], ['g1', 'g2'])
    with pytest.raises(ValueError):
        pr.restate_classes([first, (second, first)], ['A', 'B'], ['g1', 'g2'])


def test_second_end_generator_is_seeded_and_keeps_the_names():
    from test_bam2ec_gpu import make_case
    case = make_case(43, 8)
    s1, s2, other = pr.second_end(case, 43), pr.second_end(case, 43), pr.second_end(case, 44)
    assert s1 == s2 and s1['names'] != other['names']
    assert sorted(set(s1['names'])) == sorted(set(case['names'])) and s1['names'] != case['names']
    assert 4 in s1['flags'] and 256 in s1['flags'] and s1['ref_names'] == case['ref_names']


def test_no_cpu_fallback(tmp_path, hip_lib):
    from gbrs_amd.bam2emase import bam2ec_paired, paired_bam_to_classes
    if hip_lib.gbrs_device_count() > 0:
        pytest.skip("a HIP device is visible")
    a_bam, b_bam, ids = _inputs(tmp_path)
    with pytest.raises(_lib.GbrsHipError) as e:
        paired_bam_to_classes([a_bam], [b_bam], ['A', 'B'], ['g1', 'g2'])
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
    out = str(tmp_path / 'o.npz')
    with pytest.raises(_lib.GbrsHipError) as e:
        bam2ec_paired([a_bam], [b_bam], ['A', 'B'], ids, out)
    assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
    assert not os.path.exists(out)


def test_argument_checks_need_no_device(tmp_path, hip_lib):
    """NULL arguments, one handle for both ends and a handle without a reference map are refused before a device is
    looked for (the set is never dereferenced before that)."""
    from gbrs_amd.bam2emase import BamFile
    a_bam, b_bam, _ = _inputs(tmp_path)
    n = C.c_uint64(7)
    lib = hip_lib
    assert 'gbrs_ecset_add_bam_pair' in _lib.EXPORTS
    assert lib.gbrs_ecset_add_bam_pair(None, None, None, C.byref(n), None) == _lib.GBRS_ERR_INVALID
    with BamFile(a_bam) as a, BamFile(b_bam) as b:
        assert lib.gbrs_ecset_add_bam_pair(None, a._h, b._h, C.byref(n), None) == _lib.GBRS_ERR_INVALID
    assert n.value == 7
