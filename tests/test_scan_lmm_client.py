"""The mixed-model scan from C: tests/native/scan_lmm_client.c is compiled as C99 against include/gbrs_hip.h, linked with
the built libgbrs_hip.so and run on a case of tests/scan_lmm_cases.py with the decompositions the test writes for it (no
Python between the client and the library)."""
import struct
import subprocess

import numpy as np
import pytest

import scan_cases as base
import scan_lmm_cases as cases
from test_c_client import _build_client

CASE = cases.CASES[4]                      # H9-n65-c4-P7: Hx = Hp = 8, four covariates, three decompositions
LEAVE_OUT, SCALE = 1, 2.0


def test_the_client_compiles_as_c99_and_links(tmp_path):
    _build_client(tmp_path, "scan_lmm_client")


@pytest.mark.gpu
def test_the_client_against_the_restatements(tmp_path):
    """The kinship against numpy's, the LODs within the device tolerance of both host routes at the client's own
    heritabilities, those within MEASURED_HSQ of the restatement's, and the refused calls left their buffer untouched."""
    H, n, cz, P, points, _ = CASE
    D, Z, Y, kinships, kin_of_chrom, _ = cases.build(CASE)
    M, nc, eigs = sum(points), len(points), cases.decompositions(CASE)
    exe = _build_client(tmp_path, "scan_lmm_client")
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<iiiiiiqd", H, nc, n, cz, len(eigs), LEAVE_OUT, P, SCALE))
        fh.write(pad(np.asarray(points, dtype=np.int32).tobytes()))
        fh.write(pad(np.asarray(kin_of_chrom, dtype=np.int32).tobytes()))
        for a in [D, Z] + [a for pair in eigs for a in pair] + [cases.centred(Y)]:         # the caller's step: centred columns
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

    K, lod, peak_lod, peak_index = take((n, n)), take((P, M)), take((P, nc)), take((P, nc), np.int64)
    hsq, sigma2, rank = take((P, len(eigs))), take((P, len(eigs))), take((2, P), np.int32)
    at += -at % 8
    refused = take((P, len(eigs)))
    assert at == len(raw) and (refused == -1.0).all()
    want, exact = cases.kinship(D, points, LEAVE_OUT, SCALE), cases.kinship_longdouble(D, points, LEAVE_OUT, SCALE)
    assert (K == K.T).all()
    assert np.abs(K - want).max() <= base.DEVICE_FACTOR * max(np.abs(want - exact).max(), np.spacing(np.abs(exact).max()))
    rule = cases.lmm_rule(D, Z, Y, points, eigs, kin_of_chrom, hsq=hsq)
    for route in (rule["lod"], cases.lmm_gls(D, Z, Y, points, kinships, kin_of_chrom, hsq)):
        assert cases.deviation(lod, route) <= cases.device_tol(CASE)
    assert np.abs(hsq - cases.expected(CASE)[0]["hsq"]).max() <= cases.MEASURED_HSQ
    np.testing.assert_allclose(sigma2, rule["sigma2"], rtol=8 * n * np.finfo(float).eps, atol=0)
    np.testing.assert_array_equal(rank[0], rule["rank_min"])
    np.testing.assert_array_equal(rank[1], rule["rank_max"])
    peak, index = base.peaks(lod, points)
    np.testing.assert_array_equal(peak_index, index)
    np.testing.assert_array_equal(peak_lod, peak)
