"""`gbrs bam2ec` on the device against tests/bam2ec_restate.py: the `bam2emase` restatement per file, the files'
reads one after the other, then the compress oracle.  Integers, and float64 sums of ones: every comparison is exact."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

import bam_synth
from bam2ec_restate import restate_classes
from test_bam2emase_gpu import ERRORS, KEPT_FLAGS, _error_case, _have_h5, write_case

pytestmark = pytest.mark.gpu


N_PATTERNS = 40


def make_case(seed, H, n_reads=300, L=6, n_patterns=N_PATTERNS, tag='HWI-ST1:77:C0', patterns_from=None):
    """Seeded records on L = 6 loci.  A read takes one of `n_patterns` sets of 1-4 reference sequences, so most rows
    repeat; about 10 % of the reads have only flag-4 / flag-8 records; some records are reported twice; the kept
    records carry every flag value of KEPT_FLAGS; the header has sequences outside `loci` that no kept record uses.
    Read k's name depends on (tag, k) alone; `patterns_from` takes the pattern pool of another seed."""
    rng = np.random.default_rng([seed if patterns_from is None else patterns_from, 0])
    haplotypes = [chr(65 + h) for h in range(H)] if H > 1 else []
    loci = [f'T{l:05d}' for l in range(L)]
    ref_names = [f'{l}_{h}' for l in loci for h in haplotypes] if haplotypes else list(loci)
    n_usable = len(ref_names)
    ref_names = ref_names + ['other_Z', 'no-delimiter', 'T00000_A_x']
    patterns = [rng.choice(n_usable, size=int(min(rng.integers(1, 5), n_usable)), replace=False).tolist()
                for _ in range(n_patterns)]
    rng = np.random.default_rng([seed, 1])
    names, refids, flags = [], [], []
    for k in range(n_reads):
        nm = f'{tag}:{1 + k % 3}:{1101 + k // 7}:{(k * 7919) % 10007}'
        kind = int(rng.integers(0, 10))
        if kind == 0:                                  # only dropped records: a flag-4 record, sometimes a flag-8 mate
            names += [nm]; refids += [-1]; flags += [4]
            if rng.integers(0, 2):
                names += [nm]; refids += [int(rng.integers(0, len(ref_names)))]; flags += [8]
            continue
        pat = patterns[int(rng.integers(0, n_patterns))]
        for ref in rng.permutation(pat).tolist():
            names.append(nm); refids.append(ref); flags.append(KEPT_FLAGS[(k + ref) % len(KEPT_FLAGS)])
        if kind == 1:                                  # the same alignment reported twice
            names.append(nm); refids.append(refids[-1]); flags.append(256)
        if kind == 2:                                  # a dropped record on an unusable sequence: never looked at
            names.append(nm); refids.append(len(ref_names) - 2); flags.append(8)
    return dict(ref_names=ref_names, names=names, refids=refids, flags=flags, haplotypes=haplotypes, loci=loci)


def check_ec_file(path, want):
    from gbrs_amd.alignment import load_alignment, read_rname
    m = load_alignment(path)
    assert m.shape == want['shape']
    assert m.hname == want['hname'] and m.lname == want['lname']
    assert m.values is None
    assert m.count is not None and m.count.dtype == np.float64
    np.testing.assert_array_equal(m.count, want['count'])
    assert read_rname(path) is None
    if path.endswith('.npz'):
        with np.load(path) as z:
            assert 'rname' not in z.files and not any(k.startswith('values') for k in z.files)
    for h in range(want['shape'][1]):
        assert m.indptr[h].dtype == np.uint32 and m.indices[h].dtype == np.uint32
        np.testing.assert_array_equal(m.indptr[h], want['indptr'][h])
        np.testing.assert_array_equal(m.indices[h], want['indices'][h])
        col = np.repeat(np.arange(want['shape'][0]), np.diff(m.indptr[h].astype(np.int64)))
        step = np.diff(m.indices[h].astype(np.int64))
        assert (step[col[1:] == col[:-1]] > 0).all()            # class ids ascending inside a column
    return m


def npz_members(path):
    with np.load(path) as z:
        return {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}


def classes_of(paths, case):
    from gbrs_amd.bam2emase import bam_to_classes
    return bam_to_classes(paths, case['haplotypes'], case['loci'])


def check_matrix(m, want):
    assert m.shape == want['shape'] and m.hname == want['hname'] and m.lname == want['lname']
    np.testing.assert_array_equal(m.count, want['count'])
    for h in range(want['shape'][1]):
        np.testing.assert_array_equal(m.indptr[h], want['indptr'][h])
        np.testing.assert_array_equal(m.indices[h], want['indices'][h])


@pytest.mark.parametrize('H,seed', [(1, 31), (2, 32), (8, 33), (16, 34)])
def test_seeded_cases_library_and_cli(tmp_path, H, seed):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec
    case = make_case(seed, H)
    assert set(KEPT_FLAGS) | {4, 8} <= set(case['flags'])
    want = restate_classes([case], case['haplotypes'], case['loci'])
    R = want['num_reads']
    assert R == 300 and want['num_ecs'] < R / 2            # most rows repeat: the class build has something to merge
    assert want['count'].sum() == R and (want['count'] > 1).any()
    bam, ids = write_case(tmp_path, case)
    for ext in ['npz'] + (['h5'] if _have_h5() else []):
        out = str(tmp_path / f'lib.{ext}')
        stages = {}
        bam2ec([bam], case['haplotypes'], ids, out, stage_times=stages)
        check_ec_file(out, want)
        assert set(stages) == {'read', 'rank', 'classes', 'write'}
        out = str(tmp_path / f'cli.{ext}')
        argv = ['bam2ec', '-i', bam, '-m', ids, '-o', out]
        if case['haplotypes']:
            argv += ['-h', ','.join(case['haplotypes'][:-1]), '-h', case['haplotypes'][-1]] if H > 2 else \
                    ['-h', ','.join(case['haplotypes'])]
        st = tmp_path / 'stages.json'
        os.environ['GBRS_STAGE_TIMES'] = str(st)
        try:
            assert cli.main(argv) == 0
        finally:
            del os.environ['GBRS_STAGE_TIMES']
        check_ec_file(out, want)
        got = json.loads(st.read_text())
        assert 'error' not in got and set(got) >= {'read', 'rank', 'classes', 'write'} and 'build' not in got


def test_shuffled_records_give_identical_members(tmp_path):
    """Neither the read ids nor the classes may depend on a read's records being adjacent."""
    from gbrs_amd.bam2emase import bam2ec
    case = make_case(41, 8, n_reads=500)
    bam, ids = write_case(tmp_path, case, name='sorted.bam')
    order = np.random.default_rng(1).permutation(len(case['names']))
    bam2, _ = write_case(tmp_path, case, name='shuffled.bam', order=order, payload=333)
    a, b = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    bam2ec([bam], case['haplotypes'], ids, a)
    bam2ec([bam2], case['haplotypes'], ids, b)
    check_ec_file(b, restate_classes([case], case['haplotypes'], case['loci']))
    assert npz_members(a) == npz_members(b)


def test_long_identical_rows(tmp_path):
    """A row of 40 loci x 8 haplotypes = 320 entries three times under different names, and a fourth read that differs
    from it in its last (locus, haplotype) only: the packed row key cannot tell them apart, the full comparison must."""
    H, L = 8, 44
    case = make_case(51, H, n_reads=200, L=L, tag='M')
    refs = [l * H + h for l in range(40) for h in range(H)]
    last = (L - 1) * H + (H - 1)
    assert last > refs[-1]
    for nm, mine in (('K:long:1', refs), ('A:long:2', refs), ('Z:long:3', list(reversed(refs))),
                     ('L:nearly', refs[:-1] + [last])):
        case['names'] += [nm] * len(mine); case['refids'] += mine; case['flags'] += [0] * len(mine)
    want = restate_classes([case], case['haplotypes'], case['loci'])
    assert want['num_reads'] == 204
    long_classes = [int(c) for c in np.unique(want['indices'][0][want['indptr'][0][0]:want['indptr'][0][1]])
                    if sum(int((want['indices'][h] == c).sum()) for h in range(H)) == 320]
    assert len(long_classes) == 2 and sorted(want['count'][long_classes].tolist()) == [1.0, 3.0]
    bam, _ = write_case(tmp_path, case)
    check_matrix(classes_of([bam], case), want)


def test_different_rows_under_one_row_key(tmp_path):
    """The class build sorts the rows by a 64-bit key (first locus, a hash of the loci, a 16-bit hash of the haplotype
    masks) and the sort keeps equal keys in read order.  The three rows below have the same two loci and masks
    (10, 56), (34, 202) and (41, 18), which that hash maps to one value, so their repeats interleave in the sorted
    order: A B C A B C B A.  Each must still be one class, in one file and in the merge of a file with itself."""
    H, L = 8, 6
    haplotypes = [chr(65 + h) for h in range(H)]
    loci = [f'T{l:05d}' for l in range(L)]
    ref_names = [f'{l}_{h}' for l in loci for h in haplotypes]
    rows = {'A': (10, 56), 'B': (34, 202), 'C': (41, 18)}
    names, refids, flags = [], [], []
    for k, which in enumerate('ABCABCBA'):
        for l, mask in enumerate(rows[which]):
            for h in range(H):
                if mask >> h & 1:
                    names.append(f'read{k}'); refids.append(l * H + h); flags.append(0)
    case = dict(ref_names=ref_names, names=names, refids=refids, flags=flags, haplotypes=haplotypes, loci=loci)
    want = restate_classes([case], haplotypes, loci)
    assert want['num_ecs'] == 3 and want['count'].tolist() == [3.0, 3.0, 2.0]
    bam, _ = write_case(tmp_path, case)
    check_matrix(classes_of([bam], case), want)
    twice = restate_classes([case, case], haplotypes, loci)
    assert twice['num_ecs'] == 3 and twice['count'].tolist() == [6.0, 6.0, 4.0]
    check_matrix(classes_of([bam, bam], case), twice)


def _lane_cases():
    a = make_case(61, 8, n_reads=300)
    b = make_case(63, 8, n_reads=260, patterns_from=61)  # other reads under the same names, from the same patterns
    assert set(b['names']) <= set(a['names']) and b['refids'] != a['refids'][:len(b['refids'])]
    c = make_case(62, 8, n_reads=120, tag='LANE3')
    return a, b, c


def test_lanes_two_files_share_names_and_classes(tmp_path):
    from gbrs_amd import cli
    a, b, _ = _lane_cases()
    want = restate_classes([a, b], a['haplotypes'], a['loci'])
    one = restate_classes([a], a['haplotypes'], a['loci'])
    assert want['num_reads'] == 560 and one['num_ecs'] <= want['num_ecs'] <= N_PATTERNS + 1     # + the empty class
    bam_a, ids = write_case(tmp_path, a, name='a.bam')
    bam_b, _ = write_case(tmp_path, b, name='b.bam', payload=501)
    check_matrix(classes_of([bam_a, bam_b], a), want)
    other = restate_classes([b, a], a['haplotypes'], a['loci'])       # the order of the files is the order of the reads
    check_matrix(classes_of([bam_b, bam_a], a), other)
    for k, argv in enumerate((['-i', bam_a, '-i', bam_b], ['-i', bam_a + ',' + bam_b])):
        out = str(tmp_path / f'cli{k}.npz')
        assert cli.main(['bam2ec', *argv, '-m', ids, '-o', out, '-h', ','.join(a['haplotypes'])]) == 0
        check_ec_file(out, want)


def test_lanes_middle_file_has_unmapped_reads_only(tmp_path):
    a, _, c = _lane_cases()
    mid = dict(ref_names=a['ref_names'], names=[f'U{k}' for k in range(7)] + ['U3'], refids=[-1] * 7 + [2],
               flags=[4] * 7 + [8], haplotypes=a['haplotypes'], loci=a['loci'])
    want = restate_classes([a, mid, c], a['haplotypes'], a['loci'])
    without = restate_classes([a, c], a['haplotypes'], a['loci'])
    assert want['num_ecs'] == without['num_ecs'] and want['count'].sum() == without['count'].sum() + 7
    assert (want['count'] != without['count']).sum() == 1            # the empty class alone grows
    paths = [write_case(tmp_path, x, name=f'{k}.bam')[0] for k, x in enumerate((a, mid, c))]
    check_matrix(classes_of(paths, a), want)
    # and first: the empty class is then class 0
    first = restate_classes([mid, a], a['haplotypes'], a['loci'])
    assert first['count'][0] >= 7 and all(len(first['indices'][h]) == 0 or first['indices'][h].min() > 0 for h in range(8))
    check_matrix(classes_of([paths[1], paths[0]], a), first)


def test_same_file_twice_doubles_every_count(tmp_path):
    a, _, _ = _lane_cases()
    once = restate_classes([a], a['haplotypes'], a['loci'])
    twice = restate_classes([a, a], a['haplotypes'], a['loci'])
    np.testing.assert_array_equal(twice['count'], 2 * once['count'])
    bam, _ = write_case(tmp_path, a)
    m1, m2 = classes_of([bam], a), classes_of([bam, bam], a)
    check_matrix(m1, once)
    check_matrix(m2, twice)
    for h in range(8):
        np.testing.assert_array_equal(m1.indptr[h], m2.indptr[h])
        np.testing.assert_array_equal(m1.indices[h], m2.indices[h])


def test_file_without_records_is_named(tmp_path, caplog):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec
    a, _, _ = _lane_cases()
    bam, ids = write_case(tmp_path, a, name='full.bam')
    empty = dict(a, names=[], refids=[], flags=[])
    nothing, _ = write_case(tmp_path, empty, name='nothing.bam')
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError) as e:
        bam2ec([bam, nothing], a['haplotypes'], ids, out)
    assert str(e.value) == f'{nothing} holds no alignment records.'
    assert not os.path.exists(out)
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', nothing, '-i', bam, '-m', ids, '-o', out, '-h', ','.join(a['haplotypes'])]) == 0
    assert any(r.getMessage() == f'{os.path.realpath(nothing)} holds no alignment records.' for r in caplog.records)
    assert not os.path.exists(out)


@pytest.mark.parametrize('pool', [5000, 400_000])
def test_past_one_grid_pass(tmp_path, pool):
    """400,000 reads x 3 adjacent records = 1.2M records > 4096 x 256: every capped-grid kernel of the conversion loops.
    With a pool of 5,000 record triples most rows repeat; with 400,000, one per read, nearly every read is a class of its own, so the
    class matrix has more than 4096 x 256 entries and the merge kernels loop too.  The expectation is computed
    vectorised: name rank, per-read sorted unique columns, first occurrence per distinct row."""
    rng = np.random.default_rng(77)
    n_reads, per, L, H = 400_000, 3, 50, 8
    loci = [f'T{l:04d}' for l in range(L)]
    haps = [chr(65 + h) for h in range(H)]
    ref_names = [f'{l}_{h}' for l in loci for h in haps]                 # refID = l * H + h
    ids = rng.permutation(n_reads).astype(np.int64)
    uniq = np.char.add(np.char.add('HWI-D00:8:C6:1:', np.char.zfill((ids // 1000).astype('U4'), 4)),
                       np.char.add(':', np.char.zfill((ids % 1000 * 37 % 1000).astype('U4'), 4)))
    uniq = np.char.encode(uniq, 'ascii').astype('S24')
    assert len(np.unique(uniq)) == n_reads
    triples = rng.integers(0, L * H, size=(pool, per))
    dup = 5 if pool < n_reads else 50                                    # a duplicate record in every fifth / fiftieth triple
    triples[::dup, 1] = triples[::dup, 0]
    pick = rng.integers(0, pool, size=n_reads) if pool < n_reads else rng.permutation(pool)   # or a triple per read
    refids = triples[pick].reshape(-1).astype(np.int32)
    read_of = np.repeat(np.arange(n_reads), per)
    flags = rng.choice(np.array([0, 16, 256, 272], dtype=np.uint16), size=len(read_of))
    bam = str(tmp_path / 'large.bam')
    bam_synth.write_bam_fixed_width(bam, ref_names, uniq[read_of], refids, flags)
    # expectation
    order = np.argsort(uniq, kind='stable')                              # file read -> position = read id
    cols = (refids.astype(np.int64) % H) * L + refids.astype(np.int64) // H      # column h * L + l
    rows = np.sort(cols.reshape(n_reads, per), axis=1)[order]            # row of read id r: its sorted columns
    rows[:, 1:][rows[:, 1:] == rows[:, :-1]] = -1                        # duplicates stored once
    rows = np.sort(rows, axis=1)                                         # -1 (absent) first: a canonical form of the set
    distinct, first, counts = np.unique(rows, axis=0, return_index=True, return_counts=True)
    by_first = np.argsort(first, kind='stable')                          # class id = order of first occurrence
    class_of_distinct = np.empty(len(distinct), dtype=np.int64)
    class_of_distinct[by_first] = np.arange(len(distinct))
    want_count = counts[by_first].astype(np.float64)
    ent_class = np.repeat(class_of_distinct, per)
    ent_col = distinct.reshape(-1)
    keep = ent_col >= 0
    ent_class, ent_col = ent_class[keep], ent_col[keep]
    o = np.lexsort((ent_class, ent_col))
    ent_class, ent_col = ent_class[o], ent_col[o]
    ptr = np.searchsorted(ent_col, np.arange(H * L + 1))
    assert len(distinct) <= pool and want_count.sum() == n_reads
    assert len(distinct) < n_reads / 2 if pool == 5000 else len(ent_col) > 4096 * 256
    from gbrs_amd.bam2emase import bam_to_classes
    for paths, factor in (([bam], 1), ([bam, bam], 2)):
        m = bam_to_classes(paths, haps, loci)
        assert m.shape == (L, H, len(distinct))
        assert m.count.sum() == factor * 400000
        np.testing.assert_array_equal(m.count, factor * want_count)
        for h in range(H):
            np.testing.assert_array_equal(m.indptr[h], (ptr[h * L:(h + 1) * L + 1] - ptr[h * L]).astype(np.uint32))
            np.testing.assert_array_equal(m.indices[h], ent_class[ptr[h * L]:ptr[(h + 1) * L]].astype(np.uint32))


@pytest.mark.parametrize('which', ['no_reference', 'not_two_parts', 'unknown_haplotype', 'unknown_locus'])
def test_record_errors_reach_the_log_with_the_text_of_bam2emase(tmp_path, which, caplog):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec, bam2emase
    ref_names, records, haplotypes, loci, needle = ERRORS[which]
    bam, ids = _error_case(tmp_path, ref_names, records, haplotypes, loci)
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError) as ref:
        bam2emase(bam, haplotypes, ids, output_file=out)
    with pytest.raises(RuntimeError) as e:
        bam2ec([bam], haplotypes, ids, out)
    assert needle in str(e.value) and str(e.value) == str(ref.value) and bam in str(e.value)
    good = dict(ref_names=ref_names, names=['a', 'b'], refids=[0, 0], flags=[0, 16], haplotypes=haplotypes, loci=loci)
    ok, _ = write_case(tmp_path, good, name='good.bam')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', ok, '-i', bam, '-m', ids, '-o', out, '-h', ','.join(haplotypes)]) == 0
    assert any(r.getMessage() == str(ref.value).replace(bam, os.path.realpath(bam)) for r in caplog.records)
    assert not os.path.exists(out)


def test_index_dtype_uint64_is_refused(tmp_path, caplog):
    from gbrs_amd import cli
    case = make_case(71, 2, n_reads=20)
    bam, ids = write_case(tmp_path, case)
    out = str(tmp_path / 'o.npz')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', bam, '-m', ids, '-o', out, '-h', 'A,B', '--index-dtype', 'uint64']) == 0
    assert any('index-dtype' in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def _open(lib, path):
    h, n, nb = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    assert lib.gbrs_bam_open(path.encode(), 0, C.byref(h), C.byref(n), C.byref(nb)) == 0
    return h


def _set_contents(lib, e, H, L):
    from gbrs_amd import _lib
    R, G = C.c_uint64(99), C.c_uint64(99)
    nnz = np.full(H, 99, dtype=np.uint64)
    assert lib.gbrs_ecset_sizes(e, C.byref(R), C.byref(G), _lib.ptr(nnz)) == 0
    ip = [np.full(L + 1, 99, dtype=np.uint32) for _ in range(H)]
    ix = [np.zeros(int(nnz[h]), dtype=np.uint32) for h in range(H)]
    count = np.zeros(int(G.value), dtype=np.float64)
    assert lib.gbrs_ecset_get(e, _lib.ptr_table(ip), _lib.ptr_table(ix), _lib.ptr(count) if G.value else None) == 0
    return int(R.value), int(G.value), ip, ix, count


def test_abi_call_order_arguments_and_failed_add(tmp_path, hip_lib):
    from gbrs_amd import _lib
    from gbrs_amd.bam2emase import BamFile
    lib = hip_lib
    case = make_case(81, 2, n_reads=60)
    H, L = 2, len(case['loci'])
    want = restate_classes([case], case['haplotypes'], case['loci'])
    bam, _ = write_case(tmp_path, case)
    bad_case = dict(ref_names=case['ref_names'][:H * L] + ['T99999_A'], names=['q', 'r'], refids=[0, H * L], flags=[0, 0],
                    haplotypes=case['haplotypes'], loci=case['loci'])
    bad, _ = write_case(tmp_path, bad_case, name='bad.bam')
    e = C.c_void_p()
    assert lib.gbrs_ecset_create(L, H, 0, C.byref(e)) == 0
    n, secs = C.c_uint64(5), np.zeros(3)
    try:
        # an empty set: zero reads, zero classes, all-zero column pointers - not an error
        R, G, ip, ix, count = _set_contents(lib, e, H, L)
        assert (R, G) == (0, 0) and all((p == 0).all() for p in ip) and all(len(x) == 0 for x in ix)
        # before the reference map is set
        h = _open(lib, bam)
        assert lib.gbrs_ecset_add_bam(e, h, C.byref(n), None) == _lib.GBRS_ERR_STATE
        # NULL arguments
        assert lib.gbrs_ecset_add_bam(e, None, C.byref(n), None) == _lib.GBRS_ERR_INVALID
        assert lib.gbrs_ecset_add_bam(None, h, C.byref(n), None) == _lib.GBRS_ERR_INVALID
        assert lib.gbrs_ecset_add_bam(e, h, None, None) == _lib.GBRS_ERR_INVALID
        assert lib.gbrs_ecset_sizes(e, None, None, None) == _lib.GBRS_ERR_INVALID
        assert lib.gbrs_ecset_get(e, None, None, None) == _lib.GBRS_ERR_INVALID
        # a reference map of another shape: one haplotype less, then one locus more
        with BamFile(bam) as bf:
            _, hap, loc = bf.reference_map(case['haplotypes'], case['loci'])
        for hh, ll in ((H - 1, L), (H, L + 1)):
            assert lib.gbrs_bam_set_reference_map(h, len(hap), _lib.ptr(np.minimum(hap, hh - 1)), _lib.ptr(loc), hh, ll) == 0
            assert lib.gbrs_ecset_add_bam(e, h, C.byref(n), None) == _lib.GBRS_ERR_INVALID
        assert _set_contents(lib, e, H, L)[:2] == (0, 0)
        # the real thing
        assert lib.gbrs_bam_set_reference_map(h, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L) == 0
        assert lib.gbrs_ecset_add_bam(e, h, C.byref(n), _lib.ptr(secs)) == 0
        assert n.value == want['num_reads'] and (secs >= 0).all() and secs[0] > 0
        assert lib.gbrs_bam_destroy(h) == 0
        before = _set_contents(lib, e, H, L)
        assert before[:2] == (want['num_reads'], want['num_ecs'])
        np.testing.assert_array_equal(before[4], want['count'])
        for k in range(H):
            np.testing.assert_array_equal(before[2][k], want['indptr'][k])
            np.testing.assert_array_equal(before[3][k], want['indices'][k])
        # a file whose second record names an unknown locus: the add fails, the set holds what it held
        h = _open(lib, bad)
        with BamFile(bad) as bf:
            _, hap2, loc2 = bf.reference_map(case['haplotypes'], case['loci'])
        assert lib.gbrs_bam_set_reference_map(h, len(hap2), _lib.ptr(hap2), _lib.ptr(loc2), H, L) == 0
        assert lib.gbrs_ecset_add_bam(e, h, C.byref(n), None) == _lib.GBRS_ERR_INVALID
        assert b'T99999_A' in lib.gbrs_last_error() and n.value == 0
        assert lib.gbrs_bam_destroy(h) == 0
        after = _set_contents(lib, e, H, L)
        assert after[:2] == before[:2]
        for x, y in zip(before[2] + before[3] + [before[4]], after[2] + after[3] + [after[4]]):
            np.testing.assert_array_equal(x, y)
    finally:
        assert lib.gbrs_ecset_destroy(e) == 0


def test_drop_in_for_bam2emase_then_compress(tmp_path, monkeypatch):
    """The case of test_bam2emase_gpu.test_chain_bam2emase_compress_quantify (4000 x 8 x 120): the file of `bam2ec`
    has the members of `bam2emase` -> `compress` byte for byte, `quantify` writes the same reports from either, and
    an EM handle gives the same numbers whichever file it was built from."""
    from gbrs_amd import synth
    from gbrs_amd.alignment import load_alignment
    from gbrs_amd.bam2emase import bam2ec, bam2emase
    from gbrs_amd.compress import compress
    from gbrs_amd.em import EMfactory
    from gbrs_amd.quantify import quantify
    R, H, L = 4000, 8, 120
    inc = synth.make_em_problem(R=R, H=H, L=L, seed=17)
    rng = np.random.default_rng(4)
    read_name = [f'M0:1:FC:{int(x):07d}' for x in rng.permutation(R)]
    ref_names = [f'{l}_{h}' for l in inc.locus_names for h in inc.hap_names]
    per_read = [[] for _ in range(R)]
    for h in range(H):
        cols = np.repeat(np.arange(L), np.diff(inc.indptr[h].astype(np.int64)))
        for r, l in zip(inc.indices[h].tolist(), cols.tolist()):
            per_read[r].append(l * H + h)
    names, refids, flags = [], [], []
    for r in range(R):
        if not per_read[r]:
            names.append(read_name[r]); refids.append(-1); flags.append(4)
        for k, ref in enumerate(per_read[r]):
            names.append(read_name[r]); refids.append(ref); flags.append(0 if k == 0 else 256)
    bam = str(tmp_path / 'chain.bam')
    bam_synth.write_bam(bam, ref_names, names, refids, flags)
    ids = str(tmp_path / 'ids.tsv')
    with open(ids, 'w') as fh:
        fh.write('\n'.join(inc.locus_names) + '\n')
    conv, two, one = str(tmp_path / 'conv.npz'), str(tmp_path / 'two.npz'), str(tmp_path / 'one.npz')
    bam2emase(bam, inc.hap_names, ids, output_file=conv)
    compress([conv], two)
    bam2ec([bam], inc.hap_names, ids, one)
    a, b = npz_members(two), npz_members(one)
    assert sorted(a) == sorted(b) and 'count' in a and 'rname' not in a
    for k in a:
        assert a[k] == b[k], k
    grp, lens = str(tmp_path / 'g2t.tsv'), str(tmp_path / 'len.tsv')
    with open(grp, 'w') as fh:
        for g, mem in zip(inc.group_names, inc.groups):
            fh.write(g + '\t' + '\t'.join(inc.locus_names[m] for m in mem) + '\n')
    with open(lens, 'w') as fh:
        for l in range(L):
            for h in inc.hap_names:
                fh.write(f'{inc.locus_names[l]}_{h}\t{int(inc.raw_length[l])}\n')
    monkeypatch.setenv('GBRS_EM_DETERMINISTIC', '1')
    for aln, base in ((two, 'a'), (one, 'b')):
        quantify(alignment_file=aln, group_file=grp, length_file=lens, outbase=str(tmp_path / base), max_iters=10,
                 tolerance=0.0)
    reports = sorted(f[2:] for f in os.listdir(tmp_path) if f.startswith('a.'))
    assert any(f.endswith('isoforms.tpm') for f in reports) and len(reports) >= 2
    assert reports == sorted(f[2:] for f in os.listdir(tmp_path) if f.startswith('b.'))
    for f in reports:
        assert (tmp_path / ('a.' + f)).read_bytes() == (tmp_path / ('b.' + f)).read_bytes(), f
    theta = []
    for aln in (two, one):
        em = EMfactory(load_alignment(aln), deterministic=True)
        em.prepare(0.0, lenfile=lens)
        em.run(model=4, tol=0.0, max_iters=5, verbose=False)
        theta.append(np.array(em.allelic_expression))
        em.close()
    assert theta[0].sum() > 0
    np.testing.assert_array_equal(theta[0], theta[1])
