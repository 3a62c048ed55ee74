"""The launch sizes of tests/cohort_cases.py, held to what they are aimed at without a GPU: every row resolves to the route
it names (gbrs_amd/csrc/hmm_route.h compiled with tests/native/hmm_route_driver.cpp, as tests/test_hmm_route_cpu.py does),
65 is one past a multiple of every partition of a launch's samples that a kernel makes, the samples of a launch are 65
different ones, and the seed of the path draws leaves no decision close on the CPU.  A threshold or a constant that moves
fails here, by row or by name: tests/test_cohort_sizes_gpu.py then no longer reaches what it was aimed at."""
import os
import re

import numpy as np
import pytest

import cohort_cases as cases
import grid_cases
from conftest import ROOT
from test_hmm_route_cpu import driver, route  # noqa: F401  (driver is a fixture)

CSRC = os.path.join(ROOT, "gbrs_amd", "csrc")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_case_table_routes(driver, case):  # noqa: F811
    """No GBRS_TUNING_HMM_* variable: route() drops them from the environment and is given none."""
    got = route(driver, case.founders, case.n_samples)
    assert {k: got[k] for k in ("sweep", "delta", "bp", "batched")} == \
        dict(sweep=case.sweep, delta=case.delta, bp=case.bp, batched=str(case.batched))


def test_case_table_is_the_four_rows():
    assert [(c.founders, c.n_samples) for c in cases.CASES] == [(8, 5), (8, 64), (8, 65), (3, 65)]
    assert cases.edge_samples(5) == (0,) and cases.edge_samples(64) == cases.EDGE_SAMPLES[:-1]
    assert cases.edge_samples(65) == cases.EDGE_SAMPLES


def constant(filename, pattern):
    with open(os.path.join(CSRC, filename)) as fh:
        found = re.findall(pattern, fh.read(), flags=re.M)
    assert len(found) == 1, (filename, pattern, found)
    return int(found[0])


def test_65_is_one_past_every_partition():
    """IMPUTE_SAMPLES (hmm_impute.inc), the pair pass's slab of 4 * DIAG_WAVES samples (hmm_passes.hip, hmm_diag.inc) - the size
    of an MFMA group too - and MT_ROWS (hmm_match.inc, sixteen rows per wavefront), read from the sources."""
    impute = constant("hmm_impute.inc", r"^constexpr\s+int\s+IMPUTE_SAMPLES\s*=\s*(\d+)\s*;")
    block = constant("hmm_diag.inc", r"^constexpr\s+int\s+DIAG_BLOCK\s*=\s*(\d+)\s*;")
    assert constant("hmm_diag.inc", r"^constexpr\s+int\s+DIAG_WAVES\s*=\s*DIAG_BLOCK\s*/\s*(\d+)\s*;") == 64
    slab = constant("hmm_passes.hip", r"^\s*int\s+slab\s*=\s*(\d+)\s*\*\s*DIAG_WAVES\s*;") * (block // 64)
    rows = constant("hmm_match.inc", r"^constexpr\s+int\s+MT_ROWS\s*=\s*(\d+)\s*,")
    assert dict(IMPUTE_SAMPLES=impute, DIAG_SLAB=slab, MT_ROWS=rows) == cases.PARTITIONS
    sizes = (impute, slab, rows)
    for size in sizes:
        assert 65 % size == 1, size
        # the first group's ends, the second group's first, the last full group's last and the lone sample behind it
        assert {0, size - 1, size, 63, 64} <= set(cases.EDGE_SAMPLES), size
    assert {s for s in range(65) if s % slab in (0, slab - 1)} <= set(cases.EDGE_SAMPLES)     # every group of 16, both ends
    assert all(any(s % size in (0, size - 1) for size in sizes) for s in cases.EDGE_SAMPLES)


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("founders", (8, 3))
def test_the_samples_of_a_launch_are_different_samples(founders, style):
    """The 65 samples' expression rows are pairwise different: "no two samples' rows are equal" on the device can only
    fail for the device's reasons."""
    rows = [np.concatenate(grid_cases.expression_rows(grid_cases.sample_problem(founders, style, s))).ravel() for s in range(65)]
    assert len({r.tobytes() for r in rows}) == 65


@pytest.mark.parametrize("style", cases.STYLES)
@pytest.mark.parametrize("founders,n_samples", cases.PATH_ROWS)
def test_the_path_seed_leaves_no_decision_close(founders, n_samples, style):
    """cohort_cases.PATH_SEED on the oracle's alpha: the smallest decision margin over the row's EDGE_SAMPLES."""
    smallest = cases.path_margin(cases.PATH_SEED, founders, n_samples, style)
    print(f"DEVIATION smallest decision margin on the oracle's alpha H={founders} n={n_samples} {style}: {smallest:.3g} "
          f"(bound {cases.PATH_MARGIN:g})")
    assert smallest >= cases.PATH_MARGIN
    ids = cases.streams(n_samples)
    assert len(set(ids)) == n_samples and not any(ids[s] == s for s in range(n_samples))
