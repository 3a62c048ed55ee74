"""`gbrs bam2emase` on the device against the restatement of the reference's rules (tests/bam2emase_restate.py).
Everything on this path is integers and bytes, so every comparison is exact."""
import json
import logging
import os

import numpy as np
import pytest

import bam_synth
from bam2emase_restate import restate

pytestmark = pytest.mark.gpu

KEPT_FLAGS = [0, 16, 99, 256, 272, 20]          # 20 = 4 + 16: not exactly 4, so kept (and needs a reference sequence)


def _have_h5():
    try:
        from gbrs_amd import emase_h5
        emase_h5._load()
        return True
    except ImportError:
        return False


def make_case(seed, H, n_reads=300, L=40):
    """Seeded records: duplicates of (read, locus, haplotype), reads with only flag-4 / flag-8 records, every kept
    flag value, and header sequences outside `loci` that no kept record uses."""
    rng = np.random.default_rng(seed)
    haplotypes = [chr(65 + h) for h in range(H)] if H > 1 else []
    loci = [f'T{l:05d}' for l in range(L)]
    ref_names = [f'{l}_{h}' for l in loci for h in haplotypes] if haplotypes else list(loci)
    ref_names += ['other_Z', 'no-delimiter', 'T00000_A_x']       # never used by a kept record
    n_usable = len(ref_names) - 3
    names, refids, flags = [], [], []
    for k in range(n_reads):
        nm = f'HWI-ST1:77:C0:{1 + k % 3}:{1101 + k // 7}:{(k * 7919) % 10007}'
        kind = rng.integers(0, 10)
        if kind == 0:                                  # an unmapped read: one flag-4 record, sometimes its flag-8 mate
            names += [nm]; refids += [-1]; flags += [4]
            if rng.integers(0, 2):
                names += [nm]; refids += [int(rng.integers(0, len(ref_names)))]; flags += [8]
            continue
        for _ in range(int(rng.integers(1, 9))):
            names.append(nm); refids.append(int(rng.integers(0, n_usable))); flags.append(int(rng.choice(KEPT_FLAGS)))
        if kind == 1:                                  # the same alignment reported twice
            names.append(nm); refids.append(refids[-1]); flags.append(256)
        if kind == 2:                                  # a dropped record on an unusable sequence: never looked at
            names.append(nm); refids.append(len(ref_names) - 2); flags.append(8)
    return dict(ref_names=ref_names, names=names, refids=refids, flags=flags, haplotypes=haplotypes, loci=loci)


def write_case(tmp_path, case, payload=777, name='case.bam', order=None):
    idx = range(len(case['names'])) if order is None else order
    bam = str(tmp_path / name)
    bam_synth.write_bam(bam, case['ref_names'], [case['names'][i] for i in idx], [case['refids'][i] for i in idx],
                        [case['flags'][i] for i in idx], payload=payload)
    ids = str(tmp_path / 'ids.tsv')
    with open(ids, 'w') as fh:
        for l in case['loci']:
            fh.write(f'{l}\t1000\n')
        fh.write(f"{case['loci'][0]}\tagain\n")              # a repeated id is dropped (get_names)
    return bam, ids


def expected(case):
    return restate(case['ref_names'], case['names'], case['refids'], case['flags'], case['haplotypes'], case['loci'])


def check_file(path, want):
    from gbrs_amd.alignment import load_alignment, read_rname
    m = load_alignment(path)
    assert m.shape == want['shape']
    assert m.hname == want['hname'] and m.lname == want['lname']
    assert m.count is None and m.values is None
    rn = read_rname(path)
    assert rn.dtype.kind == 'S' and rn.dtype.itemsize == max(max(len(n) for n in want['rname']), 1)
    assert [x.decode() for x in rn.tolist()] == want['rname']
    for h in range(want['shape'][1]):
        assert m.indptr[h].dtype == np.uint32 and m.indices[h].dtype == np.uint32
        np.testing.assert_array_equal(m.indptr[h], want['indptr'][h])
        np.testing.assert_array_equal(m.indices[h], want['indices'][h])
    return m


def file_members(path):
    if path.endswith('.npz'):
        with np.load(path) as z:
            return {k: z[k].tobytes() for k in z.files}
    from gbrs_amd.alignment import load_alignment, read_rname
    m = load_alignment(path)
    out = {'shape': repr(m.shape), 'hname': repr(m.hname), 'lname': repr(m.lname), 'rname': read_rname(path).tobytes()}
    for h in range(m.shape[1]):
        out[f'indptr{h}'] = m.indptr[h].tobytes()
        out[f'indices{h}'] = m.indices[h].tobytes()
    return out


@pytest.mark.parametrize('H,seed', [(1, 11), (2, 12), (8, 13), (16, 14)])
def test_seeded_cases_library_and_cli(tmp_path, H, seed):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2emase
    case = make_case(seed, H)
    assert any(f == 20 for f in case['flags']) and any(f == 4 for f in case['flags']) and any(f == 8 for f in case['flags'])
    want = expected(case)
    assert any(len(want['indices'][h]) for h in range(max(H, 1)))
    bam, ids = write_case(tmp_path, case)
    exts = ['npz'] + (['h5'] if _have_h5() else [])
    for ext in exts:
        out = str(tmp_path / f'lib.{ext}')
        stages = {}
        bam2emase(bam, case['haplotypes'], ids, output_file=out, stage_times=stages)
        check_file(out, want)
        assert set(stages) >= {'read', 'rank', 'build', 'write'}
        out = str(tmp_path / f'cli.{ext}')
        argv = ['bam2emase', '-i', bam, '-m', ids, '-o', out]
        if case['haplotypes']:                        # -h A,B -h C ... : the comma list and the repeated flag together
            argv += ['-h', ','.join(case['haplotypes'][:-1]), '-h', case['haplotypes'][-1]] if H > 2 else \
                    ['-h', ','.join(case['haplotypes'])]
        st = tmp_path / 'stages.json'
        os.environ['GBRS_STAGE_TIMES'] = str(st)
        try:
            assert cli.main(argv) == 0
        finally:
            del os.environ['GBRS_STAGE_TIMES']
        check_file(out, want)
        got = json.loads(st.read_text())
        assert 'error' not in got and set(got) >= {'read', 'rank', 'build', 'write'}


def test_default_output_name(tmp_path, monkeypatch):
    if not _have_h5():
        pytest.skip('libhdf5 is not loadable')
    from gbrs_amd import cli
    case = make_case(3, 2, n_reads=40, L=6)
    bam, ids = write_case(tmp_path, case)
    monkeypatch.chdir(tmp_path)
    assert cli.main(['bam2emase', '-i', bam, '-m', ids, '-h', 'A,B']) == 0
    check_file(str(tmp_path / 'alignments.transcriptome.h5'), expected(case))


def test_shuffled_records_give_identical_contents(tmp_path):
    """Correctness must not depend on a read's records being adjacent (the candidate shortcut of the reader)."""
    from gbrs_amd.bam2emase import bam2emase
    case = make_case(21, 8, n_reads=500)
    bam, ids = write_case(tmp_path, case, name='sorted.bam')
    order = np.random.default_rng(1).permutation(len(case['names']))
    bam2, _ = write_case(tmp_path, case, name='shuffled.bam', order=order, payload=333)
    for ext in ['npz'] + (['h5'] if _have_h5() else []):
        a, b = str(tmp_path / f'a.{ext}'), str(tmp_path / f'b.{ext}')
        bam2emase(bam, case['haplotypes'], ids, output_file=a)
        bam2emase(bam2, case['haplotypes'], ids, output_file=b)
        check_file(b, expected(case))
        assert file_members(a) == file_members(b)


def _name_case(names, seed=0):
    """Every name gets 1-3 records on a small two-haplotype reference, in a scrambled order."""
    rng = np.random.default_rng(seed)
    loci = ['x', 'y', 'z']
    ref_names = [f'{l}_{h}' for l in loci for h in 'AB']
    recs = [(n, int(rng.integers(0, 6)), 0) for n in names for _ in range(int(rng.integers(1, 4)))]
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    return dict(ref_names=ref_names, names=[r[0] for r in recs], refids=[r[1] for r in recs], flags=[r[2] for r in recs],
                haplotypes=['A', 'B'], loci=loci)


NAME_SETS = {
    'every_length': [('q' * k) for k in range(1, 255)] + [''.join(chr(33 + (7 * k + j) % 94) for j in range(k)) for k in range(1, 255)],
    'prefixes': ['r', 'r1', 'r1/1', 'r10', 'r1:', 'r1/', 'r1/10', 'r 1', 'r~', 'r!', 'R', 'r1/1/1/1/1/1/1/1/1', 'r1/1/1/1/1/1/1/1/'],
    'last_byte_of_long_prefix': ['P' * 200 + c for c in 'abcxyz!~0'] + ['P' * 253 + c for c in 'ba'] + ['P' * 199, 'P' * 200],
    # words 0, 2 and 4 are the same in every name, words 1 and 3 vary
    'constant_planes_between': [f'AAAAAAAA{a:08d}CCCCCCCC{b:08d}EEEEEEEE' for a in (5, 50, 500, 7) for b in (1, 10, 2, 99999999)],
    'one_name': ['only'],
    'single_bytes': [chr(c) for c in range(33, 127)],
}


@pytest.mark.parametrize('which', sorted(NAME_SETS))
def test_name_order(tmp_path, which):
    from gbrs_amd.bam2emase import bam2emase
    names = NAME_SETS[which]
    assert len(set(names)) == len(names)
    case = _name_case(names, seed=len(names))
    want = expected(case)
    assert want['rname'] == sorted(names)
    bam, ids = write_case(tmp_path, case, payload=4001)
    out = str(tmp_path / 'o.npz')
    bam2emase(bam, case['haplotypes'], ids, output_file=out)
    check_file(out, want)


def test_large_case_leaves_the_single_workgroup_paths(tmp_path):
    """>= 1M distinct names, >= 4M records, written vectorised (every name 24 bytes, so the chain is one array)."""
    from gbrs_amd.bam2emase import bam2emase
    from gbrs_amd.alignment import load_alignment, read_rname
    from scipy.sparse import coo_matrix
    rng = np.random.default_rng(99)
    n_reads, per, L, H = 1_100_000, 4, 3000, 8
    loci = [f'T{l:06d}' for l in range(L)]
    haps = [chr(65 + h) for h in range(H)]
    ref_names = [f'{l}_{h}' for l in loci for h in haps]
    ids = rng.permutation(n_reads).astype(np.int64)
    # Illumina-like: a shared prefix, then tile / x / y fields that vary
    uniq = np.char.add(np.char.add('HWI-D00:8:C6:1:', np.char.zfill((ids // 1000).astype('U4'), 4)),
                       np.char.add(':', np.char.zfill((ids % 1000 * 37 % 1000).astype('U4'), 4)))
    uniq = np.char.encode(uniq, 'ascii').astype('S24')
    assert len(np.unique(uniq)) == n_reads
    read_of = np.repeat(np.arange(n_reads), per)                         # a read's records are adjacent, as aligners write them
    refids = rng.integers(0, len(ref_names), size=len(read_of)).astype(np.int32)
    refids[1::per] = refids[0::per]                                      # a duplicate (read, locus, haplotype) per read
    flags = rng.choice(np.array([0, 16, 256, 272], dtype=np.uint16), size=len(read_of))
    bam = str(tmp_path / 'large.bam')
    bam_synth.write_bam_fixed_width(bam, ref_names, uniq[read_of], refids, flags)
    idf = str(tmp_path / 'ids.tsv')
    with open(idf, 'w') as fh:
        fh.write('\n'.join(loci) + '\n')
    out = str(tmp_path / 'large.npz')
    bam2emase(bam, haps, idf, output_file=out)
    order = np.argsort(uniq, kind='stable')
    rank = np.empty(n_reads, dtype=np.int64)
    rank[order] = np.arange(n_reads)
    m = load_alignment(out)
    assert m.shape == (L, H, n_reads)
    np.testing.assert_array_equal(read_rname(out), uniq[order])
    rows, col = rank[read_of], refids.astype(np.int64)
    for h in range(H):
        sel = col % H == h
        c = coo_matrix((np.ones(int(sel.sum())), (rows[sel], col[sel] // H)), shape=(n_reads, L)).tocsc()
        np.testing.assert_array_equal(m.indptr[h], c.indptr.astype(np.uint32))
        np.testing.assert_array_equal(m.indices[h], c.indices.astype(np.uint32))


def _error_case(tmp_path, ref_names, records, haplotypes, loci):
    case = dict(ref_names=ref_names, names=[r[0] for r in records], refids=[r[1] for r in records],
                flags=[r[2] for r in records], haplotypes=haplotypes, loci=loci)
    return write_case(tmp_path, case, payload=64)


ERRORS = {
    # the usual unmapped pair: flags 77 / 141, no reference sequence, and neither flag is exactly 4 or 8
    'no_reference': (['t1_A'], [('a', 0, 0), ('b', -1, 77), ('b', -1, 141)], ['A'], ['t1'], 'reference sequence'),
    'not_two_parts': (['t1_A', 't1_A_x'], [('a', 0, 0), ('a', 1, 16)], ['A'], ['t1'], 't1_A_x'),
    'no_delimiter': (['t1_A', 't1A'], [('a', 0, 0), ('a', 1, 16)], ['A'], ['t1'], 't1A'),
    'unknown_haplotype': (['t1_A', 't1_C'], [('a', 0, 0), ('b', 1, 0)], ['A', 'B'], ['t1'], 't1_C'),
    'unknown_locus': (['t1_A', 't9_A'], [('a', 0, 0), ('b', 1, 256)], ['A'], ['t1'], 't9_A'),
    'unknown_locus_no_h': (['t1', 't9'], [('a', 0, 0), ('b', 1, 0)], [], ['t1'], 't9'),
    # flag 20 = 4 + 16 is not exactly 4: the record is kept, and its sequence is unusable
    'flag_20_is_kept': (['t1_A', 'bad'], [('a', 0, 0), ('b', 1, 20)], ['A'], ['t1'], 'bad'),
}


@pytest.mark.parametrize('which', sorted(ERRORS))
def test_errors_name_the_reference_sequence(tmp_path, which, caplog):
    from gbrs_amd import cli
    from gbrs_amd.bam2emase import bam2emase
    ref_names, records, haplotypes, loci, needle = ERRORS[which]
    bam, ids = _error_case(tmp_path, ref_names, records, haplotypes, loci)
    out = str(tmp_path / 'o.npz')
    with pytest.raises(RuntimeError) as e:
        bam2emase(bam, haplotypes, ids, output_file=out)
    assert needle in str(e.value)
    assert not os.path.exists(out)
    # the first offending record in file order is the one reported
    if which == 'not_two_parts':
        bam2, _ = _error_case(tmp_path, ref_names + ['zz'], records + [('c', 2, 0)], haplotypes, loci)
        with pytest.raises(RuntimeError) as e:
            bam2emase(bam2, haplotypes, ids, output_file=out)
        assert needle in str(e.value) and "'zz'" not in str(e.value)
    argv = ['bam2emase', '-i', bam, '-m', ids, '-o', out] + (['-h', ','.join(haplotypes)] if haplotypes else [])
    with caplog.at_level(logging.ERROR, logger='gbrs'):
        assert cli.main(argv) == 0
    assert any(needle in r.getMessage() for r in caplog.records)
    assert not os.path.exists(out)


def test_unused_unusable_sequences_are_never_looked_at(tmp_path):
    from gbrs_amd.bam2emase import bam2emase
    case = dict(ref_names=['t1_A', 'junk', 't7_Q'], names=['a', 'a', 'b', 'c'], refids=[0, 1, 2, 0], flags=[0, 8, 4, 16],
                haplotypes=['A'], loci=['t1'])
    bam, ids = write_case(tmp_path, case, payload=50)
    out = str(tmp_path / 'o.npz')
    bam2emase(bam, ['A'], ids, output_file=out)
    m = check_file(out, expected(case))
    assert m.shape == (1, 1, 3) and list(m.indices[0]) == [0, 2]


def _read_tpm(path):
    with open(path) as fh:
        rows = [l.rstrip('\n').split('\t') for l in fh][1:]
    return {r[0]: np.array([float(x) for x in r[1:]]) for r in rows}


def test_chain_bam2emase_compress_quantify(tmp_path):
    """The converted file feeds the rest of the workflow: its TPMs equal those of the matrix the BAM was generated
    from (same structure, rows in the order of the name sort => the project's EM tolerance, rtol 1e-9)."""
    from gbrs_amd import synth
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.bam2emase import bam2emase
    from gbrs_amd.compress import compress
    from gbrs_amd.quantify import quantify
    R, H, L = 4000, 8, 120
    inc = synth.make_em_problem(R=R, H=H, L=L, seed=17)
    rng = np.random.default_rng(4)
    read_name = [f'M0:1:FC:{int(x):07d}' for x in rng.permutation(R)]           # the name sort scrambles the rows
    ref_names = [f'{l}_{h}' for l in inc.locus_names for h in inc.hap_names]
    names, refids, flags = [], [], []
    seen = np.zeros(R, dtype=bool)
    per_read = [[] for _ in range(R)]
    for h in range(H):
        cols = np.repeat(np.arange(L), np.diff(inc.indptr[h].astype(np.int64)))
        for r, l in zip(inc.indices[h].tolist(), cols.tolist()):
            per_read[r].append(l * H + h)
            seen[r] = True
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
    conv, ec = str(tmp_path / 'conv.npz'), str(tmp_path / 'ec.npz')
    bam2emase(bam, inc.hap_names, ids, output_file=conv)
    compress([conv], ec)
    orig = str(tmp_path / 'orig.npz')
    AlignmentPropertyMatrix(shape=(L, H, R), indptr=inc.indptr, indices=inc.indices, haplotype_names=inc.hap_names,
                            locus_names=inc.locus_names).save_npz(orig)
    grp, lens = str(tmp_path / 'g2t.tsv'), str(tmp_path / 'len.tsv')
    with open(grp, 'w') as fh:
        for g, mem in zip(inc.group_names, inc.groups):
            fh.write(g + '\t' + '\t'.join(inc.locus_names[m] for m in mem) + '\n')
    with open(lens, 'w') as fh:
        for l in range(L):
            for h in inc.hap_names:
                fh.write(f'{inc.locus_names[l]}_{h}\t{int(inc.raw_length[l])}\n')
    for aln, base in ((ec, 'a'), (orig, 'b')):
        quantify(alignment_file=aln, group_file=grp, length_file=lens, outbase=str(tmp_path / base), max_iters=10,
                 tolerance=0.0)
    a, b = _read_tpm(str(tmp_path / 'a.multiway.isoforms.tpm')), _read_tpm(str(tmp_path / 'b.multiway.isoforms.tpm'))
    assert list(a) == list(b) and len(a) == L
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-300)
    assert sum(v.sum() for v in b.values()) > 0
