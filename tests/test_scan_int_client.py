"""The scan with interactive covariates from C: tests/native/scan_int_client.c is compiled as C99 against
include/gbrs_hip.h, linked with the built libgbrs_hip.so and run on a case of tests/scan_int_cases.py (no Python between the
client and the library)."""
import struct
import subprocess

import numpy as np
import pytest

import scan_cases as base
import scan_int_cases as cases
from test_c_client import _build_client

CASE = cases.CASES[6]                      # H8-n32-c3-k2-P64: 32 rows per point, two interactive covariates


def test_the_client_compiles_as_c99_and_links(tmp_path):
    _build_client(tmp_path, "scan_int_client")


@pytest.mark.gpu
def test_the_client_against_the_restatements(tmp_path):
    """The three matrices within the device tolerance of both host routes, the ranks and the peaks of the client's own
    matrices exactly, and the refused calls left their buffer untouched."""
    H, n, c, k, P, points = CASE
    D, Z, Y, zint, _ = cases.build(CASE)
    M, nc = sum(points), len(points)
    exe = _build_client(tmp_path, "scan_int_client")
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<iiiiiiq", H, nc, n, c, k, 0, P))
        fh.write(pad(np.asarray(points, dtype=np.int32).tobytes()))
        for a in (D, np.linalg.qr(Z)[0], zint, Y):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(shape, dtype=np.float64):
        nonlocal at
        count = int(np.prod(shape))
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).reshape(shape)
        at += count * np.dtype(dtype).itemsize
        return a

    got = {key: take((P, M)) for key in cases.KEYS}
    peak_full, index_full, peak_add = take((P, nc)), take((P, nc), np.int64), take((P, nc))
    peak_int, index_int = take((P, nc)), take((P, nc), np.int64)
    rank = take((2, M), np.int32)
    at += -at % 8
    refused = take((P, nc))
    assert at == len(raw) and (refused == -1.0).all()
    (rule, rank_full, rank_add, _), (lstsq, _, _) = cases.expected(CASE)
    for key in cases.KEYS:
        for route in (rule, lstsq):
            assert cases.deviation(got[key], route[key]) <= cases.device_tol(CASE, key), key
    np.testing.assert_array_equal(rank[0], rank_full)
    np.testing.assert_array_equal(rank[1], rank_add)
    peak, index = base.peaks(got["lod_full"], points)
    np.testing.assert_array_equal(peak_full, peak)
    np.testing.assert_array_equal(index_full, index)
    np.testing.assert_array_equal(peak_add, got["lod_add"][np.arange(P)[:, None], index])
    peak, index = base.peaks(got["lod_int"], points)
    np.testing.assert_array_equal(peak_int, peak)
    np.testing.assert_array_equal(index_int, index)
