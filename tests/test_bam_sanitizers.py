"""AddressSanitizer + UndefinedBehaviorSanitizer build of the BAM reader (CPU build only: sanitizers do not run on
the device here).  gbrs_amd/csrc/bamio.hip is compiled with g++ -fsanitize=address,undefined -DGBRS_HOST_ONLY
together with tests/native/bam_driver.cpp, which reads the valid and the malformed files written below, and
truncates / corrupts a small file at every byte offset.  Any sanitizer report or failed check fails the test."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_synth
from conftest import ROOT

REFS = ['t1_A', 't1_B', 't2_A', 't2_B', 'unplaced']


def _valid(tmp_path, tag, names, refids, flags, **kw):
    bam_synth.write_bam(str(tmp_path / f'valid_{tag}.bam'), REFS, names, refids, flags, **kw)
    with open(tmp_path / f'valid_{tag}.expect', 'w') as fh:
        fh.write(f'{len(REFS)} {len(names)}\n')
        for n, r, f in zip(names, refids, flags):
            fh.write(f'{r} {f} {n}\n')


def _files(tmp_path):
    rng = np.random.default_rng(8)
    names = [f'read{k // 3}:{k % 5}' for k in range(60)] + ['x', 'y' * 254, 'x']
    refids = [int(x) for x in rng.integers(-1, len(REFS), size=len(names))]
    flags = [int(x) for x in rng.choice([0, 4, 8, 16, 20, 77, 141, 256, 65535], size=len(names))]
    for payload in (1, 2, 3, 5, 37, 64, 65, 4096):
        _valid(tmp_path, f'p{payload}', names, refids, flags, payload=payload, eof=payload % 2 == 1)
    many = [f'm{k}' for k in range(30000)]                      # several inflate batches of 1024 blocks
    _valid(tmp_path, 'many', many, [k % 5 - 1 for k in range(30000)], [k % 300 for k in range(30000)], payload=400)
    _valid(tmp_path, 'norecords', [], [], [])
    stream = bam_synth.bam_stream(REFS, names[:8], refids[:8], flags[:8])
    (tmp_path / 'small.bam').write_bytes(bam_synth.bgzf(stream, payload=211))
    head = bam_synth.bam_header(REFS)

    def bad(tag, data):
        (tmp_path / f'bad_{tag}.bam').write_bytes(data)

    def rec(patch):
        r = bytearray(bam_synth.bam_record(b'name', 0, 0))
        for off, (fmt, v) in patch.items():
            struct.pack_into(fmt, r, off, v)
        return bytes(r)

    good = bam_synth.bgzf(stream, payload=100)
    bad('empty', b'')
    bad('text', b'@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:t1_A\tLN:1000\n')
    bad('gzip_not_bgzf', bytes.fromhex('1f8b0800000000000003') + b'\x03\x00' + b'\x00' * 8 + b'\x00' * 20)
    bad('magic', bam_synth.bgzf(b'BAM\x02' + stream[4:]))
    bad('cut_block', good[:-40])
    bad('cut_header', bam_synth.bgzf(stream[:len(head) - 3]))
    bad('cut_text', bam_synth.bgzf(stream[:9]))
    bad('cut_record', bam_synth.bgzf(stream[:-5], payload=50))
    bad('block_size_past_end', bam_synth.bgzf(head + rec({0: ('<i', 1 << 24)})))
    bad('block_size_negative', bam_synth.bgzf(head + rec({0: ('<i', -5)})))
    bad('block_size_tiny', bam_synth.bgzf(head + rec({0: ('<i', 8)})))
    bad('l_read_name_0', bam_synth.bgzf(head + rec({12: ('<B', 0)})))
    bad('l_read_name_past_record', bam_synth.bgzf(head + struct.pack('<i', 34) + rec({12: ('<B', 200)})[4:38]))
    bad('refid_past_header', bam_synth.bgzf(head + rec({4: ('<i', len(REFS))})))
    bad('negative_l_text', bam_synth.bgzf(b'BAM\x01' + struct.pack('<i', -1) + stream[8:]))
    bad('negative_n_ref', bam_synth.bgzf(b'BAM\x01' + struct.pack('<i', 0) + struct.pack('<i', -2)))
    bad('ref_name_0', bam_synth.bgzf(b'BAM\x01' + struct.pack('<ii', 0, 1) + struct.pack('<i', 0) + struct.pack('<i', 5)))
    b = bytearray(good)
    b[16:18] = struct.pack('<H', 9)                                 # BSIZE smaller than the header
    bad('bsize_small', bytes(b))
    b = bytearray(good)
    b[16:18] = struct.pack('<H', 65535)                             # BSIZE past the end of the file
    bad('bsize_large', bytes(b))
    b = bytearray(good)
    b[10:12] = struct.pack('<H', 400)                               # XLEN past the block
    bad('xlen_large', bytes(b))
    b = bytearray(good)
    n0 = struct.unpack_from('<H', b, 16)[0] + 1
    b[n0 - 4:n0] = struct.pack('<I', 70000)                         # ISIZE above the format's limit
    bad('isize_large', bytes(b))
    b = bytearray(good)
    b[n0 - 4:n0] = struct.pack('<I', 3)                             # ISIZE that the data does not inflate to
    bad('isize_wrong', bytes(b))
    b = bytearray(good)
    b[n0 - 8] ^= 1                                                  # CRC-32
    bad('crc', bytes(b))


def test_bamio_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not installed")
    exe = tmp_path / "bam_asan"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DGBRS_HOST_ONLY", "-Wall", "-Wextra", "-x", "c++",
           os.path.join(ROOT, "gbrs_amd", "csrc", "bamio.hip"), os.path.join(ROOT, "tests", "native", "bam_driver.cpp"),
           "-o", str(exe), "-pthread", "-ldl"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan is not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    data = tmp_path / "files"
    data.mkdir()
    _files(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "bam sanitizer driver: ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
