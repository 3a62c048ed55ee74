"""gbrs_scan_permute from C: tests/native/scan_perm_client.c is compiled as C99 against include/gbrs_hip.h, linked with
the built libgbrs_hip.so and run on a cohort of tests/scan_cases.py (no Python between the client and the library)."""
import struct
import subprocess

import numpy as np
import pytest

import scan_cases as cases
import scan_perm_restate as restate
from test_c_client import _build_client

CASE = (8, 70, 4, 130, (1, 65, 9))
MASK = (False, True, True)


def test_the_client_compiles_as_c99_and_links(tmp_path):
    _build_client(tmp_path, "scan_perm_client")


@pytest.mark.gpu
def test_the_client_against_the_restatement(tmp_path):
    """The permutations equal the restatement's, perm_max on chromosomes 2 and 3 is within the device tolerance of both
    host routes, and the two refused calls (before prepare, B = 0) left their buffer untouched."""
    from gbrs_amd.scan import covariate_basis
    H, n, c, P, points = CASE
    D, Z, Y, _ = cases.build(CASE)
    B = restate.N_PERM
    exe = _build_client(tmp_path, "scan_perm_client")
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<iiiiqqQ", H, len(points), n, c, P, B, restate.SEED))
        fh.write(pad(np.asarray(points, dtype=np.int32).tobytes()))
        fh.write(pad(np.asarray(MASK, dtype=np.uint8).tobytes()))
        for a in (D, covariate_basis(Z), Y):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    perm_max = np.frombuffer(raw, dtype=np.float64, count=P * B).reshape(P, B)
    index = np.frombuffer(raw, dtype=np.int32, count=B * n, offset=8 * P * B).reshape(B, n)
    refused = np.frombuffer(raw, dtype=np.float64, count=P * B, offset=8 * P * B + 4 * B * n)
    assert len(raw) == 16 * P * B + 4 * B * n and (refused == -1.0).all()
    np.testing.assert_array_equal(index, restate.permutations(restate.SEED, B, n))
    for route in restate.expected_max(CASE, B, restate.SEED, MASK):
        assert cases.deviation(perm_max, route) <= cases.DEVICE_FACTOR * restate.MEASURED_FLOOR_PERM
