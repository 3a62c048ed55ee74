"""Host side of `gbrs bam2emase` (no device needed): the BGZF/BAM reader through the library's host-only entry
points, the locus-name rule, the argument parser, and the rule that the conversion itself has no CPU fallback."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_synth
from gbrs_amd import _lib
from gbrs_amd.bam2emase import BamFile, get_names

# A whole BAM file, byte by byte: two BGZF blocks whose deflate streams are single *stored* blocks (so the plain
# bytes are readable below), cut in the middle of the second record's 4-byte length field, then the end-of-file block.
#   header: text "@HD\tVN:1.6\n", references g1_A, g1_B, g2_A (length 1000 each)
#   records (name, refID, flag): (r2, 0, 0) (r2, 1, 256) (r1, 2, 16) (r3, -1, 4)  - three reads, two haplotypes
KNOWN = bytes.fromhex(
    # block 1: gzip header with the BC subfield (BSIZE 0x0088), stored block of 0x6a bytes
    '1f8b08040000000000ff0600424302008800' '016a0095ff'
    '42414d01' '0b000000' '40484409564e3a312e360a' '03000000'                      # BAM\1, l_text, text, n_ref
    '05000000' '67315f4100' 'e8030000'                                             # g1_A
    '05000000' '67315f4200' 'e8030000'                                             # g1_B
    '05000000' '67325f4100' 'e8030000'                                             # g2_A
    '26000000' '00000000' '00000000' '03' '00' '4812' '0000' '0000' '02000000'     # record 0: r2 on g1_A, flag 0
    'ffffffff' 'ffffffff' '00000000' '723200' '11' 'ffff'
    '2600'                                                                         # half of record 1's block_size
    'd984caf3' '6a000000'                                                          # CRC-32, ISIZE
    # block 2
    '1f8b08040000000000ff0600424302009a00' '017c0083ff'
    '0000' '01000000' '00000000' '03' '00' '4812' '0000' '0001' '02000000'         # record 1: r2 on g1_B, flag 256
    'ffffffff' 'ffffffff' '00000000' '723200' '11' 'ffff'
    '26000000' '02000000' '00000000' '03' '00' '4812' '0000' '1000' '02000000'     # record 2: r1 on g2_A, flag 16
    'ffffffff' 'ffffffff' '00000000' '723100' '11' 'ffff'
    '26000000' 'ffffffff' 'ffffffff' '03' '00' '4812' '0000' '0400' '02000000'     # record 3: r3 unmapped, flag 4
    'ffffffff' 'ffffffff' '00000000' '723300' '11' 'ffff'
    '62924ba0' '7c000000'
    # end-of-file block
    '1f8b08040000000000ff0600424302001b0003000000000000000000')


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _scan(path):
    with BamFile(path) as bam:
        refid, flag, names = bam.scan_records()
        return bam.references, list(bam.reference_lengths), list(refid), list(flag), names


def test_known_answer_file(tmp_path):
    refs, lens, refid, flag, names = _scan(_write(tmp_path, 'known.bam', KNOWN))
    assert refs == ['g1_A', 'g1_B', 'g2_A']
    assert lens == [1000, 1000, 1000]
    assert refid == [0, 1, 2, -1]
    assert flag == [0, 256, 16, 4]
    assert names == [b'r2', b'r2', b'r1', b'r3']


def test_known_answer_reference_map(tmp_path):
    with BamFile(_write(tmp_path, 'known.bam', KNOWN)) as bam:
        hname, hap, loc = bam.reference_map(['A', 'B'], ['g2', 'g1'])
        assert hname == ['A', 'B'] and list(hap) == [0, 1, 0] and list(loc) == [1, 1, 0]
        hname, hap, loc = bam.reference_map([], ['g1_A', 'g2_A'])              # no -h: the whole name is the locus
        assert hname == ['h0'] and list(hap) == [0, 0xFFFFFFFF, 0] and list(loc) == [0, 3, 1]
        _, hap, loc = bam.reference_map(['A'], ['g1'], delim='_')
        assert list(hap) == [0, 0xFFFFFFFF, 0xFFFFFFFF] and list(loc) == [0, 2, 3]   # unknown haplotype, unknown locus
        _, hap, loc = bam.reference_map(['A', 'B'], ['g1'], delim='1')
        assert list(hap) == [0xFFFFFFFF] * 3 and list(loc) == [2, 2, 1]        # ('g', '_A'): no such haplotype; 'g2_A' has no '1'


CASE_REFS = ['t1_A', 't1_B', 't2_A', 't2_B']
CASE_NAMES = ['read/1', 'read/1', 'r', 'a-much-longer-read-name:1:2:3', 'r', 'z']
CASE_REFID = [0, 1, 3, 2, -1, 0]
CASE_FLAGS = [0, 256, 16, 99, 4, 272]


def test_records_straddle_blocks(tmp_path):
    """Every payload size from 1 byte up to past the second record's end: block borders fall on every byte of the
    header, of a record's length field and of its body."""
    stream = bam_synth.bam_stream(CASE_REFS, CASE_NAMES, CASE_REFID, CASE_FLAGS)
    first = len(bam_synth.bam_header(CASE_REFS)) + len(bam_synth.bam_record(b'read/1', 0, 0))
    for payload in list(range(1, first + 50)) + [len(stream) - 1, len(stream), len(stream) + 1]:
        for eof in (True, False):
            path = _write(tmp_path, 'c.bam', bam_synth.bgzf(stream, payload=payload, eof=eof))
            refs, _, refid, flag, names = _scan(path)
            assert refs == CASE_REFS, payload
            assert refid == CASE_REFID and flag == CASE_FLAGS, payload
            assert names == [n.encode() for n in CASE_NAMES], payload


def test_many_blocks_and_long_names(tmp_path):
    """More blocks than one inflate batch holds (1024), names of every length 1..254."""
    rng = np.random.default_rng(5)
    names = [''.join(chr(c) for c in rng.integers(33, 127, size=k)) for k in range(1, 255)] * 12
    refids = rng.integers(-1, 4, size=len(names))
    flags = rng.choice([0, 4, 8, 16, 20, 99, 256], size=len(names))
    path = str(tmp_path / 'many.bam')
    bam_synth.write_bam(path, CASE_REFS, names, refids, flags, payload=150)
    assert os.path.getsize(path) > 1024 * 150
    _, _, refid, flag, got = _scan(path)
    assert refid == list(refids) and flag == list(flags)
    assert got == [n.encode() for n in names]


def _open_error(path):
    with pytest.raises(_lib.GbrsHipError) as e:
        with BamFile(path) as bam:
            bam.scan_records()
    assert e.value.status == _lib.GBRS_ERR_INVALID
    return str(e.value)


def test_malformed_files_are_refused(tmp_path):
    stream = bam_synth.bam_stream(CASE_REFS, CASE_NAMES, CASE_REFID, CASE_FLAGS)
    good = bam_synth.bgzf(stream, payload=100, eof=True)
    assert 'truncated' in _open_error(_write(tmp_path, 't1.bam', good[:len(good) - 40]))       # inside a block
    assert 'truncated' in _open_error(_write(tmp_path, 't2.bam', bam_synth.bgzf(stream[:-7], payload=100)))   # inside a record
    assert 'truncated' in _open_error(_write(tmp_path, 't3.bam', bam_synth.bgzf(stream[:30], payload=100)))   # inside the header
    assert 'not a BGZF' in _open_error(_write(tmp_path, 'm1.bam', b'@HD\tVN:1.6\n' * 10))      # SAM text
    assert 'empty' in _open_error(_write(tmp_path, 'm0.bam', b''))
    assert 'not a BAM' in _open_error(_write(tmp_path, 'm2.bam', bam_synth.bgzf(b'BAM\x02' + stream[4:], payload=100)))
    bad = bytearray(good)
    first_len = bad[16] + (bad[17] << 8) + 1
    bad[first_len - 8] ^= 0x40                                                                  # the first block's CRC-32
    assert 'CRC' in _open_error(_write(tmp_path, 'c1.bam', bytes(bad)))
    bad = bytearray(good)
    bad[30] ^= 0xFF                                                                             # a byte of deflate data
    msg = _open_error(_write(tmp_path, 'c2.bam', bytes(bad)))
    assert 'CRC' in msg or 'inflate' in msg
    bad = bytearray(good)
    bad[16], bad[17] = 10, 0                                                                    # BSIZE below the header size
    assert 'BSIZE' in _open_error(_write(tmp_path, 'b1.bam', bytes(bad)))
    rec = bytearray(bam_synth.bam_record(b'x', 0, 0))
    rec[12] = 0                                                                                 # l_read_name
    assert 'l_read_name' in _open_error(_write(tmp_path, 'r1.bam', bam_synth.bgzf(bam_synth.bam_header(CASE_REFS) + bytes(rec))))
    rec = bytearray(bam_synth.bam_record(b'x', 0, 0))
    rec[0:4] = (1 << 20).to_bytes(4, 'little')                                                  # block_size past the end
    assert 'truncated' in _open_error(_write(tmp_path, 'r2.bam', bam_synth.bgzf(bam_synth.bam_header(CASE_REFS) + bytes(rec))))
    rec = bytearray(bam_synth.bam_record(b'x', 0, 0))
    rec[4:8] = (9).to_bytes(4, 'little')                                                        # refID beyond the header's list
    assert 'reference sequence 9' in _open_error(_write(tmp_path, 'r3.bam', bam_synth.bgzf(bam_synth.bam_header(CASE_REFS) + bytes(rec))))


def test_error_in_a_later_batch_keeps_its_message(tmp_path):
    """Batches after the first are inflated on a read-ahead thread: a bad block there is reported all the same."""
    names = [f'n{k}' for k in range(40000)]
    path = str(tmp_path / 'late.bam')
    bam_synth.write_bam(path, CASE_REFS, names, [0] * len(names), [0] * len(names), payload=300)
    data = bytearray(open(path, 'rb').read())
    assert len(data) > 3000 * 100
    data[-28 - 8] ^= 0x01                                  # CRC-32 of the last data block (the end-of-file block has 28 bytes)
    msg = _open_error(_write(tmp_path, 'late_crc.bam', bytes(data)))
    assert 'CRC' in msg and 'late_crc.bam' in msg
    msg = _open_error(_write(tmp_path, 'late_cut.bam', bytes(data[:-28 - 5])))
    assert 'truncated' in msg and 'late_cut.bam' in msg


def test_get_names_rule(tmp_path):
    p = tmp_path / 'ids.tsv'
    p.write_text('t2\t100\tx\nt1\nt2\t7\n t3 \t1\n\nt1\textra\n')
    assert get_names(str(p)) == ['t2', 't1', ' t3 ', '']


def test_argument_parser(tmp_path, capsys):
    from gbrs_amd.cli import build_parser
    bam = _write(tmp_path, 'a.bam', KNOWN)
    ids = _write(tmp_path, 'ids.tsv', b'g1\ng2\n')
    ap = build_parser()
    a = ap.parse_args(['bam2emase', '-i', bam, '-m', ids, '-h', 'A,B', '-h', 'C'])
    assert a.command == 'bam2emase' and a.haplotypes == ['A,B', 'C']
    assert a.output_file is None and a.delim == '_' and a.index_dtype == 'uint32' and a.data_dtype == 'uint8'
    assert a.verbose == 0 and a.device == 0
    assert a.alignment_file == os.path.realpath(bam) and a.locusid_file == os.path.realpath(ids)
    a = ap.parse_args(['bam2emase', '--alignment-file', bam, '--locus-ids', ids, '--haplotype-char', 'X', '-o', 'o.h5',
                       '-d', '.', '-vv', '--device', '3', '--index-dtype', 'uint64', '--data-dtype', 'float'])
    assert (a.haplotypes, a.output_file, a.delim, a.verbose, a.device) == (['X'], 'o.h5', '.', 2, 3)
    assert ap.parse_args(['bam2emase', '-i', bam, '-m', ids]).haplotypes is None
    with pytest.raises(SystemExit) as e:
        ap.parse_args(['bam2emase', '--help'])
    assert e.value.code == 0
    assert '--haplotype-char' in capsys.readouterr().out


def test_function_defaults():
    import inspect
    from gbrs_amd.bam2emase import bam2emase
    p = inspect.signature(bam2emase).parameters
    assert list(p) == ['alignment_file', 'haplotypes', 'locusid_file', 'output_file', 'delim', 'index_dtype', 'data_dtype',
                       'device', 'stage_times']
    assert (p['output_file'].default, p['delim'].default, p['index_dtype'].default, p['data_dtype'].default) == \
        ('alignments.transcriptome.h5', '_', 'uint32', 'uint8')


def test_index_dtype_other_than_uint32_is_refused(tmp_path):
    from gbrs_amd.bam2emase import bam2emase
    with pytest.raises(RuntimeError, match='index-dtype'):
        bam2emase(_write(tmp_path, 'a.bam', KNOWN), ['A', 'B'], _write(tmp_path, 'ids.tsv', b'g1\ng2\n'),
                  output_file=str(tmp_path / 'o.npz'), index_dtype='uint64')


def test_rname_is_written_only_when_set(tmp_path):
    """save / save_npz write rname when the matrix has one; load_alignment does not read it back."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix, load_alignment, read_rname
    ip = [np.array([0, 1, 2], dtype=np.uint32)]
    ix = [np.array([1, 0], dtype=np.uint32)]
    plain = AlignmentPropertyMatrix(shape=(2, 1, 2), indptr=ip, indices=ix, haplotype_names=['h0'], locus_names=['a', 'b'])
    named = AlignmentPropertyMatrix(shape=(2, 1, 2), indptr=ip, indices=ix, haplotype_names=['h0'], locus_names=['a', 'b'],
                                    read_names=np.array([b'r1', b'r10'], dtype='S3'))
    exts = ['.npz']
    try:
        from gbrs_amd import emase_h5
        emase_h5._load()
        exts.append('.h5')
    except ImportError:
        pass
    for ext in exts:
        a, b = str(tmp_path / ('plain' + ext)), str(tmp_path / ('named' + ext))
        plain.save(a)
        named.save(b)
        assert read_rname(a) is None
        assert read_rname(b).tolist() == [b'r1', b'r10']
        m = load_alignment(b)
        assert m.rname is None and m.shape == (2, 1, 2) and m.lname == ['a', 'b']
    with pytest.raises(RuntimeError):
        AlignmentPropertyMatrix(shape=(2, 1, 2), indptr=ip, indices=ix, read_names=[b'x'])


def test_convert_has_no_cpu_fallback(tmp_path, hip_lib):
    if hip_lib.gbrs_device_count() > 0:
        pytest.skip("a HIP device is visible")
    with BamFile(_write(tmp_path, 'known.bam', KNOWN)) as bam:
        _, hap, loc = bam.reference_map(['A', 'B'], ['g1', 'g2'])
        with pytest.raises(_lib.GbrsHipError) as e:
            bam.convert(hap, loc, 2, 2)
        assert e.value.status == _lib.GBRS_ERR_NO_DEVICE
        # and the call sequence is enforced: convert before the map is set is a state error, not a crash
    h = C.c_void_p()
    n, nb = C.c_uint64(0), C.c_uint64(0)
    assert hip_lib.gbrs_bam_open(_write(tmp_path, 'k2.bam', KNOWN).encode(), 0, C.byref(h), C.byref(n), C.byref(nb)) == 0
    R, w = C.c_uint64(0), C.c_uint32(0)
    nnz = np.zeros(2, dtype=np.uint64)
    assert hip_lib.gbrs_bam_convert(h, 0, C.byref(R), C.byref(w), _lib.ptr(nnz), None) == _lib.GBRS_ERR_STATE
    assert hip_lib.gbrs_bam_destroy(h) == 0
