"""A BAM *writer* for the bam2emase tests: Python standard library and numpy only, and no code in common with
the reader under test (gbrs_amd/csrc/bamio.hip).

    write_bam(path, ref_names, names, refids, flags, payload=..., eof=True)

writes one record per entry of (names, refids, flags) - unmapped records get refID -1 from the caller - with a
short dummy sequence, into BGZF blocks of `payload` plain bytes each (the last one shorter), so that with a
small payload records and even their 4-byte length fields straddle blocks.  `eof` appends the 28-byte empty
end-of-file block."""
import struct
import zlib

import numpy as np

EOF_BLOCK = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def bgzf_block(plain: bytes, level=1) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = co.compress(plain) + co.flush()
    bsize = 12 + 6 + len(cdata) + 8 - 1
    assert bsize < 65536
    return (struct.pack('<BBBBIBBH', 31, 139, 8, 4, 0, 0, 255, 6) + struct.pack('<BBHH', 66, 67, 2, bsize) + cdata +
            struct.pack('<II', zlib.crc32(plain) & 0xFFFFFFFF, len(plain)))


def bgzf(stream: bytes, payload=0xFF00, eof=True, level=1) -> bytes:
    out = [bgzf_block(stream[k:k + payload], level) for k in range(0, len(stream), payload)]
    if eof:
        out.append(EOF_BLOCK)
    return b''.join(out)


def bam_header(ref_names, ref_lengths=None, text=b'@HD\tVN:1.6\tSO:unsorted\n') -> bytes:
    out = [b'BAM\x01', struct.pack('<i', len(text)), text, struct.pack('<i', len(ref_names))]
    for k, n in enumerate(ref_names):
        n = n.encode() if isinstance(n, str) else n
        out += [struct.pack('<i', len(n) + 1), n, b'\x00', struct.pack('<i', 1000 if ref_lengths is None else ref_lengths[k])]
    return b''.join(out)


def bam_record(name: bytes, refid: int, flag: int, seq_len=4) -> bytes:
    body = struct.pack('<iiBBHHHiiii', refid, 0 if refid >= 0 else -1, len(name) + 1, 0, 4680, 0, flag, seq_len, -1, -1, 0)
    body += name + b'\x00' + b'\x11' * ((seq_len + 1) // 2) + b'\xff' * seq_len
    return struct.pack('<i', len(body)) + body


def bam_stream(ref_names, names, refids, flags) -> bytes:
    return bam_header(ref_names) + b''.join(bam_record(n.encode() if isinstance(n, str) else n, int(r), int(f))
                                            for n, r, f in zip(names, refids, flags))


def write_bam(path, ref_names, names, refids, flags, payload=0xFF00, eof=True):
    with open(path, 'wb') as fh:
        fh.write(bgzf(bam_stream(ref_names, names, refids, flags), payload=payload, eof=eof))


def records_fixed_width(names_s, refids, flags) -> bytes:
    """Vectorised record chain for the large case: `names_s` is a numpy 'S<w>' array whose names all have exactly w
    bytes, so every record has the same size and the chain is one 2-D uint8 array."""
    w = names_s.dtype.itemsize
    n = len(names_s)
    assert (np.char.str_len(names_s) == w).all()
    rec = np.zeros(n, dtype=np.dtype([('block_size', '<i4'), ('refid', '<i4'), ('pos', '<i4'), ('l_read_name', 'u1'),
                                      ('mapq', 'u1'), ('bin', '<u2'), ('n_cigar', '<u2'), ('flag', '<u2'), ('l_seq', '<i4'),
                                      ('next_refid', '<i4'), ('next_pos', '<i4'), ('tlen', '<i4'), ('name', f'S{w}'),
                                      ('nul', 'u1')]))
    rec['block_size'] = rec.dtype.itemsize - 4
    rec['refid'] = refids
    rec['pos'] = np.where(np.asarray(refids) >= 0, 0, -1)
    rec['l_read_name'] = w + 1
    rec['bin'] = 4680
    rec['flag'] = flags
    rec['next_refid'] = -1
    rec['next_pos'] = -1
    rec['name'] = names_s
    return rec.tobytes()


def write_bam_fixed_width(path, ref_names, names_s, refids, flags, payload=0xFF00, eof=True):
    stream = bam_header(ref_names) + records_fixed_width(names_s, refids, flags)
    with open(path, 'wb') as fh:
        for k in range(0, len(stream), payload << 8):          # block by block, a few MiB of plain bytes at a time
            fh.write(bgzf(stream[k:k + (payload << 8)], payload=payload, eof=False))
        if eof:
            fh.write(EOF_BLOCK)
