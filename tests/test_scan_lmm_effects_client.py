"""The founder effects and support intervals under the mixed model from C: tests/native/scan_lmm_effects_client.c is
compiled as C99 against include/gbrs_hip.h, linked with the built libgbrs_hip.so and run on a case of
tests/scan_lmm_effects_cases.py with the decompositions the test writes for it (no Python between the client and the
library)."""
import struct
import subprocess

import numpy as np
import pytest

import scan_effects_cases as plain
import scan_lmm_cases as lmm
import scan_lmm_effects_cases as cases
from test_c_client import _build_client

CASE = lmm.CASES[4]                        # H9-n65-c4-P7: Hx = Hp = 8, four covariates, three decompositions
DROP = 1.5


def test_the_client_compiles_as_c99_and_links(tmp_path):
    _build_client(tmp_path, "scan_lmm_effects_client")


@pytest.mark.gpu
def test_the_client_against_the_restatements(tmp_path):
    """The intervals are the rule on the client's own LODs; the effects lie within the device tolerance of both host routes at
    the client's own heritabilities, their LODs and heritabilities are the scan's bits, and the refused calls left their
    buffer untouched."""
    H, n, cz, P, points, _ = CASE
    D, Z, _, _, kin_of_chrom, _ = lmm.build(CASE)
    pheno, columns, at, _ = cases.build(CASE)
    M, nc, eigs, T, P1 = sum(points), len(points), lmm.decompositions(CASE), len(columns), pheno.shape[1]
    exe = _build_client(tmp_path, "scan_lmm_effects_client")
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<iiiiiiqqd", H, nc, n, cz, len(eigs), 0, P1, T, DROP))
        fh.write(pad(np.asarray(points, dtype=np.int32).tobytes()))
        fh.write(pad(np.asarray(kin_of_chrom, dtype=np.int32).tobytes()))
        for a in [D, Z] + [a for pair in eigs for a in pair] + [lmm.centred(pheno)]:       # the caller's step: centred columns
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(columns.tobytes())
        fh.write(at.tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    where = 0

    def take(shape, dtype=np.float64):
        nonlocal where
        count = int(np.prod(shape))
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=where).reshape(shape)
        where += count * np.dtype(dtype).itemsize
        return a

    lod, peak_lod, peak_index, hsq = take((P1, M)), take((P1, nc)), take((P1, nc), np.int64), take((P1, len(eigs)))
    lo, hi = take((P1, nc), np.int64), take((P1, nc), np.int64)
    got = {"effect": take((T, H)), "se": take((T, H)), "lod": take(T), "sigma2": take(T), "hsq": take(T), "rank": take(T, np.int32)}
    where += -where % 8
    refused = take(T)
    assert where == len(raw) and (refused == -1.0).all()
    peak, want_lo, want_hi = plain.support_rule(lod, points, DROP)
    np.testing.assert_array_equal(peak_index, peak)
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(hi, want_hi)
    np.testing.assert_array_equal(peak_lod, lod[np.arange(P1)[:, None], peak])
    chrom = np.array([cases.chrom_of(points, m) for m in at])
    np.testing.assert_array_equal(got["lod"], lod[columns, at])
    np.testing.assert_array_equal(got["hsq"], hsq[columns, np.asarray(kin_of_chrom)[chrom]])
    rule, gls, _ = cases.both_routes(CASE, hsq)
    np.testing.assert_array_equal(got["rank"], rule["rank"])
    for route in (rule, gls):
        for key in cases.KEYS:
            on = cases.judged(CASE, key)
            assert cases.deviation(got[key][on], route[key][on]) <= cases.device_tol(CASE, key), key
