"""`gbrs bam2ec --mate-file` on the device against tests/bam2ec_paired_restate.py: the `bam2emase` restatement of
both ends, the name test, the intersection, the items' reads one after the other, then the compress oracle.
Integers, and float64 sums of ones: every comparison is exact."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

import bam_synth
import bam2ec_paired_restate as pr
from test_bam2emase_gpu import ERRORS, _error_case, _have_h5, write_case
from test_bam2ec_gpu import _open, _set_contents, check_ec_file, check_matrix, make_case, npz_members

pytestmark = pytest.mark.gpu

SENTENCE = "The read ID's are not compatible."


def paired_classes(firsts, seconds, case, stage_times=None):
    from gbrs_amd.bam2emase import paired_bam_to_classes
    return paired_bam_to_classes(firsts, seconds, case['haplotypes'], case['loci'], stage_times=stage_times)


def write_pair(tmp_path, first, second, tag='p'):
    a, ids = write_case(tmp_path, first, name=f'{tag}_1.bam')
    b, _ = write_case(tmp_path, second, name=f'{tag}_2.bam', payload=419)
    return a, b, ids


@pytest.mark.parametrize('H,seed,n_reads', [(1, 41, 300), (2, 42, 300), (8, 43, 300), (16, 44, 300), (8, 45, 1537)])
def test_seeded_pairs_library_and_cli(tmp_path, H, seed, n_reads):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec_paired
    first = make_case(seed, H, n_reads=n_reads)
    second = pr.second_end(first, seed)
    # the inputs are not vacuous (the restatement alone)
    n1, n2, nc, lost = pr.entry_counts(first, second, first['haplotypes'], first['loci'])
    assert nc >= n1 / 2 and nc < n1 and nc < n2 and lost >= 3
    want = pr.restate_classes([(first, second)], first['haplotypes'], first['loci'])
    assert want['num_reads'] == n_reads and want['num_ecs'] < n_reads / 2
    assert want['count'].sum() == n_reads and (want['count'] > 1).any()
    a, b, ids = write_pair(tmp_path, first, second)
    for ext in ['npz'] + (['h5'] if _have_h5() else []):
        out = str(tmp_path / f'lib.{ext}')
        stages = {}
        bam2ec_paired([a], [b], first['haplotypes'], ids, out, stage_times=stages)
        check_ec_file(out, want)
        assert set(stages) == {'read', 'rank', 'common', 'classes', 'write'}
        out = str(tmp_path / f'cli.{ext}')
        argv = ['bam2ec', '-i', a, '--mate-file' if ext == 'npz' else '-I', b, '-m', ids, '-o', out]
        if first['haplotypes']:
            argv += ['-h', ','.join(first['haplotypes'])]
        st = tmp_path / 'stages.json'
        os.environ['GBRS_STAGE_TIMES'] = str(st)
        try:
            assert cli.main(argv) == 0
        finally:
            del os.environ['GBRS_STAGE_TIMES']
        check_ec_file(out, want)
        got = json.loads(st.read_text())
        assert 'error' not in got and set(got) >= {'read', 'rank', 'common', 'classes', 'write'}


# ---- hand-made structures: the intersection and the offset rebuild ------------------------------------------------
H8, L97, R_HAND = 8, 97, 2000


def _case_of_entries(entries, R=R_HAND, H=H8, L=L97, seed=0):
    """entries: set of (read, column) with column = h * L + l -> a case whose read k is named rd{k:05d}; a read without
    an entry has one flag-4 record.  Records in shuffled order."""
    haplotypes = [chr(65 + h) for h in range(H)]
    loci = [f'T{l:05d}' for l in range(L)]
    ref_names = [f'{l}_{h}' for l in loci for h in haplotypes]          # refID = l * H + h
    recs = [(r, (c % L) * H + c // L, 0) for r, c in sorted(entries)]
    have = {r for r, _ in entries}
    recs += [(r, -1, 4) for r in range(R) if r not in have]
    order = np.random.default_rng(seed).permutation(len(recs))
    recs = [recs[i] for i in order]
    return dict(ref_names=ref_names, names=[f'rd{r:05d}' for r, _, _ in recs], refids=[x for _, x, _ in recs],
                flags=[f for _, _, f in recs], haplotypes=haplotypes, loci=loci)


def _hand_entries():
    rng = np.random.default_rng(7)
    ncols = H8 * L97
    a, b = set(), set()
    big, low, high, mid = 300, 100, 200, 388
    special = {0, 1, low, high, big, mid, ncols - 2, ncols - 1}
    reads_a = rng.choice(R_HAND, size=791, replace=False)
    shared = reads_a[:395]
    rest = np.setdiff1d(np.arange(R_HAND), reads_a)
    reads_b = np.concatenate((shared, rng.choice(rest, size=791 - 395, replace=False)))
    a |= {(int(r), big) for r in reads_a}
    b |= {(int(r), big) for r in reads_b}
    for c in range(ncols):                                 # hundreds of columns with 0 - 2 entries in either end
        if c in special:
            continue
        mine = rng.choice(R_HAND, size=int(rng.integers(0, 3)), replace=False).tolist()
        a |= {(int(r), c) for r in mine}
        b |= {(int(r), c) for r in mine if rng.random() < 0.6}
        b |= {(int(r), c) for r in rng.choice(R_HAND, size=int(rng.integers(0, 2)), replace=False).tolist()}
    a |= {(5, 0), (1999, 0), (17, ncols - 1)}              # in the first end only: the first and the last column
    b |= {(5, 1), (6, 1), (17, ncols - 2)}                 # in the second end only: next to them
    a |= {(r, mid) for r in (3, 4, 900)}                   # in the middle: first end only
    a |= {(r, low) for r in range(1500, 1510)}             # the second end's ids are all smaller ...
    b |= {(r, low) for r in range(10, 20)}
    a |= {(r, high) for r in range(10, 20)}                # ... and all larger
    b |= {(r, high) for r in range(1500, 1510)}
    return a, b, big


def _per_column(entries, ncols):
    n = np.zeros(ncols, dtype=np.int64)
    for _, c in entries:
        n[c] += 1
    return n


def test_hand_made_columns(tmp_path):
    a, b, big = _hand_entries()
    ncols = H8 * L97
    na, nb, nc = (_per_column(x, ncols) for x in (a, b, a & b))
    assert na[big] == 791 and nb[big] == 791 and 300 < nc[big] < 500            # one column over several workgroups
    small = (na <= 2) & (nb <= 3)
    assert small.sum() > 700 and (na == 0).sum() > 100 and ((na > 0) & (nc == 0)).sum() > 100
    for c in (0, 388, ncols - 1):
        assert na[c] > 0 and nb[c] == 0                                         # emptied at the start, middle, end
    assert nb[1] > 0 and na[1] == 0 and nb[ncols - 2] > 0 and na[ncols - 2] == 0
    assert nc[100] == 0 and nc[200] == 0 and na[100] == nb[100] == 10
    first, second = _case_of_entries(a, seed=1), _case_of_entries(b, seed=2)
    want = pr.restate_classes([(first, second)], first['haplotypes'], first['loci'])
    assert want['num_reads'] == R_HAND
    p, q, _ = write_pair(tmp_path, first, second)
    check_matrix(paired_classes([p], [q], first), want)
    check_matrix(paired_classes([q], [p], first), pr.restate_classes([(second, first)], first['haplotypes'], first['loci']))


def test_second_end_contains_the_first_and_nothing_in_common(tmp_path):
    a, b, _ = _hand_entries()
    first, both = _case_of_entries(a, seed=1), _case_of_entries(a | b, seed=3)
    alone = pr.restate_classes([first], first['haplotypes'], first['loci'])
    want = pr.restate_classes([(first, both)], first['haplotypes'], first['loci'])
    check_matrix_equal = lambda x, y: all(np.array_equal(x[k][h], y[k][h]) for k in ('indptr', 'indices') for h in range(H8))
    assert check_matrix_equal(alone, want) and np.array_equal(alone['count'], want['count'])
    p, q, _ = write_pair(tmp_path, first, both, tag='in')
    check_matrix(paired_classes([p], [q], first), want)
    # every entry of the second end one column further: nothing in common, one empty class of all reads
    ncols = H8 * L97
    moved = _case_of_entries({(r, (c + 1) % ncols) for r, c in a} - a, seed=4)
    none = pr.restate_classes([(first, moved)], first['haplotypes'], first['loci'])
    assert none['num_ecs'] == 1 and none['count'].tolist() == [float(R_HAND)] and all(len(x) == 0 for x in none['indices'])
    q2, _ = write_case(tmp_path, moved, name='moved.bam')
    m = paired_classes([p], [q2], first)
    check_matrix(m, none)
    assert m.shape == (L97, H8, 1)


def test_order_independence(tmp_path):
    from gbrs_amd.bam2emase import bam2ec_paired
    first = make_case(46, 8, n_reads=500)
    second = pr.second_end(first, 46)
    a, ids = write_case(tmp_path, first, name='a.bam')
    b, _ = write_case(tmp_path, second, name='b.bam')
    order = np.random.default_rng(3).permutation(len(second['names']))
    b2, _ = write_case(tmp_path, second, name='b_shuffled.bam', order=order, payload=333)
    outs = [str(tmp_path / f'{k}.npz') for k in range(3)]
    bam2ec_paired([a], [b], first['haplotypes'], ids, outs[0])
    bam2ec_paired([a], [b2], first['haplotypes'], ids, outs[1])
    bam2ec_paired([a], [b], first['haplotypes'], ids, outs[2])
    check_ec_file(outs[0], pr.restate_classes([(first, second)], first['haplotypes'], first['loci']))
    assert npz_members(outs[0]) == npz_members(outs[1])
    assert open(outs[0], 'rb').read() == open(outs[2], 'rb').read()


# ---- incompatible names -------------------------------------------------------------------------------------------
def _named_case(names, base):
    """One record per name on a reference sequence that depends on the name's place."""
    return dict(base, names=list(names), refids=[k % 12 for k in range(len(names))], flags=[0] * len(names))


def _incompatible(which):
    base = make_case(47, 2, n_reads=1)
    w13 = [f'R{k:012d}' for k in range(40)]
    w38 = ['N' * 25 + f'{k:013d}' for k in range(40)]
    assert len(w13[0]) == 13 and len(w38[0]) == 38
    if which == 'lacks_one':
        a, b = w13, w13[:17] + w13[18:]
    elif which == 'one_more':
        a, b = w13, w13 + ['R999999999999']
    elif which == 'last_byte_13':
        a, b = w13, w13[:23] + [w13[23][:-1] + 'x'] + w13[24:]
    elif which == 'last_byte_38':
        a, b = w38, w38[:31] + [w38[31][:-1] + 'x'] + w38[32:]
    elif which == 'first_name':
        a, b = w13, ['Q' + w13[0][1:]] + w13[1:]
    else:                                                    # the longest name differs: the widths differ too
        a, b = w13 + ['Z' * 20], w13 + ['Z' * 21]
    sa, sb = sorted(set(a)), sorted(set(b))
    p = next((k for k in range(min(len(sa), len(sb))) if sa[k] != sb[k]), min(len(sa), len(sb)))
    if p >= len(sb) or (p < len(sa) and sa[p] < sb[p]):
        who = (sa[p], 0)
    else:
        who = (sb[p], 1)
    rng = np.random.default_rng(len(which))
    a = [a[k] for k in rng.permutation(len(a))]
    b = [b[k] for k in rng.permutation(len(b))]
    return _named_case(a, base), _named_case(b, base), p, who


WHICH = ['lacks_one', 'one_more', 'last_byte_13', 'last_byte_38', 'first_name', 'longest_differs']


@pytest.mark.parametrize('which', WHICH)
def test_incompatible_names(tmp_path, hip_lib, caplog, which):
    from gbrs_amd import _lib, cli
    from gbrs_amd.bam2emase import BamFile, bam2ec_paired
    lib = hip_lib
    first, second, p, (name, end) = _incompatible(which)
    with pytest.raises(ValueError):
        pr.restate_classes([(first, second)], first['haplotypes'], first['loci'])
    a, b, ids = write_pair(tmp_path, first, second)
    tail = f"position {p}: '{name}' is in {(a, b)[end]} only."
    out = str(tmp_path / 'o.npz')
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        with pytest.raises(ValueError) as e:
            bam2ec_paired([a], [b], first['haplotypes'], ids, out)
    assert str(e.value).startswith(SENTENCE) and str(e.value).endswith(tail)
    assert any(r.getMessage() == str(e.value) for r in caplog.records) and not os.path.exists(out)
    caplog.clear()
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', a, '-I', b, '-m', ids, '-o', out, '-h', ','.join(first['haplotypes'])]) == 0
    assert any(r.getMessage().startswith(SENTENCE) for r in caplog.records) and not os.path.exists(out)
    # at the ABI: a set that holds a pair keeps it through the failed add, and takes a compatible pair afterwards
    H, L = len(first['haplotypes']), len(first['loci'])
    good = (first, _named_case(first['names'][::-1], first))
    ga, gb, _ = write_pair(tmp_path, *good, tag='good')
    e_set = C.c_void_p()
    assert lib.gbrs_ecset_create(L, H, 0, C.byref(e_set)) == 0
    n = C.c_uint64(0)
    try:
        def add(x, y):
            with BamFile(x) as f1, BamFile(y) as f2:
                for f in (f1, f2):
                    _, hap, loc = f.reference_map(first['haplotypes'], first['loci'])
                    assert lib.gbrs_bam_set_reference_map(f._h, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L) == 0
                return lib.gbrs_ecset_add_bam_pair(e_set, f1._h, f2._h, C.byref(n), None)
        assert add(ga, gb) == 0 and n.value == len(set(first['names']))
        before = _set_contents(lib, e_set, H, L)
        assert add(a, b) == _lib.GBRS_ERR_INVALID and n.value == 0
        msg = lib.gbrs_last_error().decode()
        assert msg.startswith(SENTENCE) and msg.endswith(tail)
        after = _set_contents(lib, e_set, H, L)
        assert after[:2] == before[:2]
        for x, y in zip(before[2] + before[3] + [before[4]], after[2] + after[3] + [after[4]]):
            np.testing.assert_array_equal(x, y)
        assert add(ga, gb) == 0
        want = pr.restate_classes([good, good], first['haplotypes'], first['loci'])
        R, G, ip, ix, count = _set_contents(lib, e_set, H, L)
        assert (R, G) == (want['num_reads'], want['num_ecs'])
        np.testing.assert_array_equal(count, want['count'])
        for h in range(H):
            np.testing.assert_array_equal(ip[h], want['indptr'][h])
            np.testing.assert_array_equal(ix[h], want['indices'][h])
    finally:
        assert lib.gbrs_ecset_destroy(e_set) == 0


def test_files_without_records(tmp_path, caplog):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec_paired
    first = make_case(48, 8, n_reads=40)
    empty = dict(first, names=[], refids=[], flags=[])
    a, ids = write_case(tmp_path, first, name='full.bam')
    n1, _ = write_case(tmp_path, empty, name='nothing_1.bam')
    n2, _ = write_case(tmp_path, empty, name='nothing_2.bam')
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError) as e:                   # a pair without any record is reported as an empty file is
        bam2ec_paired([n1], [n2], first['haplotypes'], ids, out)
    assert str(e.value) == f'{n1} and {n2} hold no alignment records.'
    for x, y in ((a, n1), (n1, a)):                          # one empty end against one with records: incompatible
        with pytest.raises(ValueError) as e:
            bam2ec_paired([x], [y], first['haplotypes'], ids, out)
        assert str(e.value).startswith(SENTENCE) and n1 in str(e.value)
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', a, '-I', n1, '-m', ids, '-o', out, '-h', ','.join(first['haplotypes'])]) == 0
    assert any(r.getMessage().startswith(SENTENCE) for r in caplog.records)
    assert not os.path.exists(out)


# ---- lanes and mixing ---------------------------------------------------------------------------------------------
def _two_pairs():
    a = make_case(61, 8, n_reads=300)
    c = make_case(62, 8, n_reads=120, tag='LANE3')
    return (a, pr.second_end(a, 61)), (c, pr.second_end(c, 62))


def test_two_pairs_through_the_cli(tmp_path):
    from gbrs_amd import cli
    p1, p2 = _two_pairs()
    hap, loci = p1[0]['haplotypes'], p1[0]['loci']
    want = pr.restate_classes([p1, p2], hap, loci)
    assert want['num_reads'] == 420
    one, two = pr.restate_classes([p1], hap, loci), pr.restate_classes([p2], hap, loci)
    assert max(one['num_ecs'], two['num_ecs']) < want['num_ecs'] < one['num_ecs'] + two['num_ecs']   # some classes merge
    a1, b1, ids = write_pair(tmp_path, *p1, tag='x')
    a2, b2, _ = write_pair(tmp_path, *p2, tag='y')
    for k, argv in enumerate((['-i', a1, '-I', b1, '-i', a2, '-I', b2], ['-i', a1 + ',' + a2, '--mate-file', b1 + ',' + b2],
                              ['-I', b1, '-I', b2, '-i', a1 + ',' + a2])):
        out = str(tmp_path / f'cli{k}.npz')
        assert cli.main(['bam2ec', *argv, '-m', ids, '-o', out, '-h', ','.join(hap)]) == 0
        check_ec_file(out, want)
    check_matrix(paired_classes([a2, a1], [b2, b1], p1[0]), pr.restate_classes([p2, p1], hap, loci))


def test_same_pair_twice_doubles_every_count(tmp_path):
    p1, _ = _two_pairs()
    hap, loci = p1[0]['haplotypes'], p1[0]['loci']
    once, twice = pr.restate_classes([p1], hap, loci), pr.restate_classes([p1, p1], hap, loci)
    np.testing.assert_array_equal(twice['count'], 2 * once['count'])
    a, b, _ = write_pair(tmp_path, *p1)
    m1, m2 = paired_classes([a], [b], p1[0]), paired_classes([a, a], [b, b], p1[0])
    check_matrix(m1, once)
    check_matrix(m2, twice)
    for h in range(8):
        np.testing.assert_array_equal(m1.indptr[h], m2.indptr[h])
        np.testing.assert_array_equal(m1.indices[h], m2.indices[h])


def _set_map(lib, handle, path, case, H, L):
    from gbrs_amd import _lib
    from gbrs_amd.bam2emase import BamFile
    with BamFile(path) as bf:
        _, hap, loc = bf.reference_map(case['haplotypes'], case['loci'])
    assert lib.gbrs_bam_set_reference_map(handle, len(hap), _lib.ptr(hap), _lib.ptr(loc), H, L) == 0
    return hap, loc


def test_abi_mixing_single_and_paired(tmp_path, hip_lib):
    from gbrs_amd import _lib
    lib = hip_lib
    p1, p2 = _two_pairs()
    single = p2[0]
    hap, loci = single['haplotypes'], single['loci']
    H, L = 8, len(loci)
    want = pr.restate_classes([single, p1, single], hap, loci)
    assert want['num_reads'] == 120 + 300 + 120
    s, ids = write_case(tmp_path, single, name='single.bam')
    a, b, _ = write_pair(tmp_path, *p1)
    e = C.c_void_p()
    assert lib.gbrs_ecset_create(L, H, 0, C.byref(e)) == 0
    n, secs = C.c_uint64(0), np.full(4, -1.0)
    try:
        hs, ha, hb = _open(lib, s), _open(lib, a), _open(lib, b)
        for h, path, case in ((hs, s, single), (ha, a, p1[0]), (hb, b, p1[1])):
            _set_map(lib, h, path, case, H, L)
        assert lib.gbrs_ecset_add_bam(e, hs, C.byref(n), None) == 0 and n.value == 120
        assert lib.gbrs_ecset_add_bam_pair(e, ha, hb, C.byref(n), _lib.ptr(secs)) == 0 and n.value == 300
        assert (secs >= 0).all() and secs[0] > 0
        assert lib.gbrs_ecset_add_bam(e, hs, C.byref(n), None) == 0 and n.value == 120
        for h in (hs, ha, hb):
            assert lib.gbrs_bam_destroy(h) == 0
        R, G, ip, ix, count = _set_contents(lib, e, H, L)
        assert (R, G) == (want['num_reads'], want['num_ecs'])
        np.testing.assert_array_equal(count, want['count'])
        for h in range(H):
            np.testing.assert_array_equal(ip[h], want['indptr'][h])
            np.testing.assert_array_equal(ix[h], want['indices'][h])
    finally:
        assert lib.gbrs_ecset_destroy(e) == 0


# ---- past one grid pass -------------------------------------------------------------------------------------------
def _classes_of_rows(rows, H, L):
    """rows: (R, per) columns per read id, -1 = absent -> (count per class, class-matrix column pointers and class ids)
    with the classes in first-occurrence order (the vectorised expectation of test_bam2ec_gpu.test_past_one_grid_pass)."""
    per = rows.shape[1]
    rows = np.sort(rows, axis=1)
    rows[:, 1:][rows[:, 1:] == rows[:, :-1]] = -1
    rows = np.sort(rows, axis=1)
    distinct, first, counts = np.unique(rows, axis=0, return_index=True, return_counts=True)
    by_first = np.argsort(first, kind='stable')
    class_of_distinct = np.empty(len(distinct), dtype=np.int64)
    class_of_distinct[by_first] = np.arange(len(distinct))
    ent_class = np.repeat(class_of_distinct, per)
    ent_col = distinct.reshape(-1)
    keep = ent_col >= 0
    ent_class, ent_col = ent_class[keep], ent_col[keep]
    o = np.lexsort((ent_class, ent_col))
    ent_class, ent_col = ent_class[o], ent_col[o]
    return counts[by_first].astype(np.float64), np.searchsorted(ent_col, np.arange(H * L + 1)), ent_class


def test_past_one_grid_pass(tmp_path):
    """400,000 reads x 3 records in either end: more than 4096 x 256 kept entries each and 400,000 x 3 name words, so
    the grid-stride loops of the name check, the intersection flags and the compaction all wrap."""
    rng = np.random.default_rng(78)
    n_reads, per, L, H = 400_000, 3, 50, 8
    loci = [f'T{l:04d}' for l in range(L)]
    haps = [chr(65 + h) for h in range(H)]
    ref_names = [f'{l}_{h}' for l in loci for h in haps]                 # refID = l * H + h
    ids = rng.permutation(n_reads).astype(np.int64)
    uniq = np.char.add(np.char.add('HWI-D00:8:C6:1:', np.char.zfill((ids // 1000).astype('U4'), 4)),
                       np.char.add(':', np.char.zfill((ids % 1000 * 37 % 1000).astype('U4'), 4)))
    uniq = np.char.encode(uniq, 'ascii').astype('S24')
    assert len(np.unique(uniq)) == n_reads
    ref_a = rng.integers(0, L * H, size=(n_reads, per))
    ref_b = ref_a.copy()
    change = rng.random(n_reads) < 0.4                                    # the second end differs in one record of 40 %
    ref_b[change, 2] = rng.integers(0, L * H, size=int(change.sum()))
    other = rng.permutation(n_reads)                                     # the second end's reads in another order
    read_of = np.repeat(np.arange(n_reads), per)
    flags = rng.choice(np.array([0, 16, 256, 272], dtype=np.uint16), size=len(read_of))
    a, b = str(tmp_path / 'large_1.bam'), str(tmp_path / 'large_2.bam')
    bam_synth.write_bam_fixed_width(a, ref_names, uniq[read_of], ref_a.reshape(-1).astype(np.int32), flags)
    bam_synth.write_bam_fixed_width(b, ref_names, uniq[np.repeat(other, per)], ref_b[other].reshape(-1).astype(np.int32), flags)
    # expectation: read id = rank of the name; a column is common iff the other end's row has it
    order = np.argsort(uniq, kind='stable')
    col = lambda ref: ((ref % H) * L + ref // H)[order]
    ca, cb = col(ref_a), col(ref_b)
    distinct_entries = lambda c: len(np.unique((np.arange(n_reads)[:, None] * (H * L) + c).reshape(-1)))
    assert distinct_entries(ca) > 4096 * 256 and distinct_entries(cb) > 4096 * 256 and n_reads * 3 > 4096 * 256
    common = np.where((ca[:, :, None] == cb[:, None, :]).any(axis=2), ca, -1)
    assert 4096 * 128 < (common >= 0).sum() < min(distinct_entries(ca), distinct_entries(cb))
    want_count, ptr, ent_class = _classes_of_rows(common, H, L)
    assert want_count.sum() == n_reads
    from gbrs_amd.bam2emase import paired_bam_to_classes
    m = paired_bam_to_classes([a], [b], haps, loci)
    assert m.shape == (L, H, len(want_count))
    np.testing.assert_array_equal(m.count, want_count)
    for h in range(H):
        np.testing.assert_array_equal(m.indptr[h], (ptr[h * L:(h + 1) * L + 1] - ptr[h * L]).astype(np.uint32))
        np.testing.assert_array_equal(m.indices[h], ent_class[ptr[h * L]:ptr[(h + 1) * L]].astype(np.uint32))


# ---- drop-in ------------------------------------------------------------------------------------------------------
def test_drop_in_for_the_four_command_chain(tmp_path):
    """bam2emase on each end -> get-common-alignments -> compress writes the members of `bam2ec --mate-file`."""
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2emase
    from gbrs_amd.compress import compress
    from gbrs_amd.matops import get_common_alignments
    first = make_case(49, 8, n_reads=1200)
    second = pr.second_end(first, 49)
    a, b, ids = write_pair(tmp_path, first, second)
    e1, e2, common, four, one = (str(tmp_path / f'{k}.npz') for k in ('end1', 'end2', 'common', 'four', 'one'))
    bam2emase(a, first['haplotypes'], ids, output_file=e1)
    bam2emase(b, first['haplotypes'], ids, output_file=e2)
    get_common_alignments([e1, e2], common)
    compress([common], four)
    assert cli.main(['bam2ec', '-i', a, '--mate-file', b, '-m', ids, '-o', one, '-h', ','.join(first['haplotypes'])]) == 0
    x, y = npz_members(four), npz_members(one)
    assert sorted(x) == sorted(y) and 'count' in x and 'rname' not in x
    for k in x:
        assert x[k] == y[k], k
    check_ec_file(one, pr.restate_classes([(first, second)], first['haplotypes'], first['loci']))


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_abi_arguments_and_record_error_in_the_second_file(tmp_path, hip_lib):
    from gbrs_amd import _lib
    lib = hip_lib
    first = make_case(81, 2, n_reads=60)
    second = pr.second_end(first, 81)
    H, L = 2, len(first['loci'])
    want = pr.restate_classes([(first, second)], first['haplotypes'], first['loci'])
    a, b, _ = write_pair(tmp_path, first, second)
    names = sorted(set(first['names']))
    bad_case = dict(ref_names=first['ref_names'][:H * L] + ['T99999_A'], names=names + [names[3]],
                    refids=[0] * len(names) + [H * L], flags=[0] * (len(names) + 1), haplotypes=first['haplotypes'],
                    loci=first['loci'])
    bad, _ = write_case(tmp_path, bad_case, name='bad.bam')
    e = C.c_void_p()
    assert lib.gbrs_ecset_create(L, H, 0, C.byref(e)) == 0
    n = C.c_uint64(5)
    try:
        ha, hb = _open(lib, a), _open(lib, b)
        # before the reference maps are set: neither, then only the first
        assert lib.gbrs_ecset_add_bam_pair(e, ha, hb, C.byref(n), None) == _lib.GBRS_ERR_STATE
        hap, loc = _set_map(lib, ha, a, first, H, L)
        assert lib.gbrs_ecset_add_bam_pair(e, ha, hb, C.byref(n), None) == _lib.GBRS_ERR_STATE
        assert b'gbrs_bam_set_reference_map' in lib.gbrs_last_error()
        # NULL arguments, one handle for both ends
        for args in ((None, ha, hb, C.byref(n)), (e, None, hb, C.byref(n)), (e, ha, None, C.byref(n)), (e, ha, hb, None),
                     (e, ha, ha, C.byref(n))):
            assert lib.gbrs_ecset_add_bam_pair(*args, None) == _lib.GBRS_ERR_INVALID
        # the second end's map has another shape: one haplotype less, then one locus more
        for hh, ll in ((H - 1, L), (H, L + 1)):
            assert lib.gbrs_bam_set_reference_map(hb, len(hap), _lib.ptr(np.minimum(hap, hh - 1)), _lib.ptr(loc), hh, ll) == 0
            assert lib.gbrs_ecset_add_bam_pair(e, ha, hb, C.byref(n), None) == _lib.GBRS_ERR_INVALID
            assert b.encode() in lib.gbrs_last_error() and b'the set' in lib.gbrs_last_error()
        assert _set_contents(lib, e, H, L)[:2] == (0, 0)
        # the real thing, stage_seconds NULL
        _set_map(lib, hb, b, second, H, L)
        assert lib.gbrs_ecset_add_bam_pair(e, ha, hb, C.byref(n), None) == 0 and n.value == want['num_reads']
        before = _set_contents(lib, e, H, L)
        assert before[:2] == (want['num_reads'], want['num_ecs'])
        np.testing.assert_array_equal(before[4], want['count'])
        for k in range(H):
            np.testing.assert_array_equal(before[2][k], want['indptr'][k])
            np.testing.assert_array_equal(before[3][k], want['indices'][k])
        # a second end whose last record names an unknown locus: the message names that file, the set holds what it held
        hbad = _open(lib, bad)
        _set_map(lib, hbad, bad, bad_case, H, L)
        assert lib.gbrs_ecset_add_bam_pair(e, ha, hbad, C.byref(n), None) == _lib.GBRS_ERR_INVALID
        msg = lib.gbrs_last_error()
        assert b'T99999_A' in msg and bad.encode() in msg and a.encode() not in msg and n.value == 0
        for h in (ha, hb, hbad):
            assert lib.gbrs_bam_destroy(h) == 0
        after = _set_contents(lib, e, H, L)
        assert after[:2] == before[:2]
        for x, y in zip(before[2] + before[3] + [before[4]], after[2] + after[3] + [after[4]]):
            np.testing.assert_array_equal(x, y)
    finally:
        assert lib.gbrs_ecset_destroy(e) == 0


@pytest.mark.parametrize('which', ['no_reference', 'unknown_locus'])
def test_record_errors_reach_the_log(tmp_path, which, caplog):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2ec_paired, bam2emase
    ref_names, records, haplotypes, loci, needle = ERRORS[which]
    bam, ids = _error_case(tmp_path, ref_names, records, haplotypes, loci)
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError) as ref:
        bam2emase(bam, haplotypes, ids, output_file=out)
    good = dict(ref_names=ref_names, names=['a', 'b'], refids=[0, 0], flags=[0, 16], haplotypes=haplotypes, loci=loci)
    ok, _ = write_case(tmp_path, good, name='good.bam')
    for x, y in ((ok, bam), (bam, ok)):
        with pytest.raises(RuntimeError) as e:
            bam2ec_paired([x], [y], haplotypes, ids, out)
        assert needle in str(e.value) and str(e.value) == str(ref.value)
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(['bam2ec', '-i', ok, '-I', bam, '-m', ids, '-o', out, '-h', ','.join(haplotypes)]) == 0
    assert any(r.getMessage() == str(ref.value).replace(bam, os.path.realpath(bam)) for r in caplog.records)
    assert not os.path.exists(out)
