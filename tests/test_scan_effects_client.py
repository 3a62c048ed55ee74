"""gbrs_scan_effects and gbrs_scan_run_support from C: tests/native/scan_effects_client.c is compiled as C99 against
include/gbrs_hip.h, linked with the built libgbrs_hip.so and run on a case of tests/scan_effects_cases.py (no Python between
the client and the library)."""
import struct
import subprocess

import numpy as np
import pytest

import scan_cases as base
import scan_effects_cases as cases
from test_c_client import _build_client

CASE = (9, 33, 1, 9)
DROP = 1.5


def test_the_client_compiles_as_c99_and_links(tmp_path):
    _build_client(tmp_path, "scan_effects_client")


@pytest.mark.gpu
def test_the_client_against_the_restatements(tmp_path):
    """The effects within the device tolerance of both host routes, the ranks equal, the intervals those of the rule on the
    client's own LODs, and the four refused calls (before prepare, a column outside the table, a negative drop) left their
    buffers untouched."""
    from gbrs_amd.scan import covariate_basis
    H, n, c, T = CASE
    D, Z, pheno, columns, points, _ = cases.build(CASE)
    y = cases.zeroed(pheno)                                                         # the caller's step: a constant column goes in as zeros
    P, M, nc = y.shape[1], sum(base.POINTS), len(base.POINTS)
    exe = _build_client(tmp_path, "scan_effects_client")
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<iiiiqqd", H, nc, n, c, P, T, DROP))
        fh.write(pad(np.asarray(base.POINTS, dtype=np.int32).tobytes()))
        fh.write(np.ascontiguousarray(columns, dtype=np.int64).tobytes())
        fh.write(np.ascontiguousarray(points, dtype=np.int64).tobytes())
        for a in (D, covariate_basis(Z), y):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(shape, dtype=np.float64, padded=False):
        nonlocal at
        count = int(np.prod(shape))
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).reshape(shape)
        at += count * np.dtype(dtype).itemsize
        if padded:
            at += -at % 8
        return a

    got = {"effect": take((T, H)), "se": take((T, H)), "lod": take(T), "sigma2": take(T), "rank": take(T, np.int32, padded=True)}
    lods, peak_lod = take((P, M)), take((P, nc))
    peak_index, lo, hi = take((P, nc), np.int64), take((P, nc), np.int64), take((P, nc), np.int64)
    refused, refused_lo = take((T, H)), take((P, nc), np.int64)
    assert at == len(raw) and (refused == -1.0).all() and (refused_lo == -7).all()
    rule, svd, _ = cases.expected(CASE)
    np.testing.assert_array_equal(got["rank"], rule["rank"])
    for key in cases.KEYS:
        on = cases.judged(CASE, key)
        for route in (rule, svd):
            assert cases.deviation(got[key][on], route[key][on]) <= cases.device_tol(CASE, key), key
    peak, want_lo, want_hi = cases.support_rule(lods, base.POINTS, DROP)
    np.testing.assert_array_equal(peak_index, peak)
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(hi, want_hi)
    np.testing.assert_array_equal(peak_lod, np.take_along_axis(lods, peak, axis=1))
