"""Which passes over an EM handle take the gather-side M-step (gbrs_amd/csrc/em_step.h, em_gather_mstep): a Model-4 step on
the tile layout, kernel Tiles or TilesOneWord, unweighted, not deterministic, not persistent, 1, 2, 4 or 8 haplotypes, the
whole-locus view, no long rows, no heavy loci, acc not handed out, no posteriors, no resampling, no pair mode, block sums
that hold 8 slots per tile, and GBRS_TUNING_NO_GATHER_MSTEP not set.  One row per condition.  The header is host C++ only:
compiled here with tests/native/em_gather_driver.cpp by the host compiler, run once per row with the row's environment."""
import subprocess

import pytest

from em_plan_tool import FLAG, build_driver, tuned_env


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_gather"), "em_gather_driver")


def taken(driver, kind="step", H=8, L=400, N=100000, flags=(), counts=0, n_tiles=5, n_long=0, all_one_word=0, acc_out=0,
          n_heavy=0, msum_cap=4096, pair=0, **tuning):
    args = [driver, H, L, N, sum(FLAG[f] for f in flags), counts, kind, n_tiles, n_long, all_one_word, acc_out, n_heavy,
            msum_cap, pair]
    run = subprocess.run([str(a) for a in args], capture_output=True, text=True, env=tuned_env(tuning), timeout=60)
    assert run.returncode == 0, run.stderr
    got = {k: int(v) for k, v in (kv.split("=") for kv in run.stdout.split())}
    assert got["route_unchanged"] == 1
    assert got["no_gather_mstep"] == got["plan_no_gather_mstep"]
    return got["gather_mstep"]


def test_the_plain_step_takes_it(driver):
    assert taken(driver) == 1
    assert taken(driver, all_one_word=1) == 1                              # TilesOneWord
    assert taken(driver, NO_FUSED_MSTEP=1) == 1                            # whichever M-step launch it replaces


ROWS = [
    ("a prepare pass", dict(kind="prepare")),
    ("a partial pass", dict(kind="partial")),
    ("a model 1-3 pass", dict(kind="model")),
    ("the CSC layout", dict(flags=["LAYOUT_CSC"])),
    ("no tile to launch", dict(n_tiles=0)),
    ("row counts given: weighted", dict(counts=1)),
    ("merged rows: weighted", dict(flags=["MERGE_IDENTICAL_ROWS"])),
    ("deterministic", dict(flags=["DETERMINISTIC"])),
    ("persistent workgroups", dict(PERSISTENT=1)),
    ("16 haplotypes", dict(H=16)),
    ("3 haplotypes", dict(H=3)),
    ("32 haplotypes: CSC kernels", dict(H=32)),
    ("half-locus view", dict(H=16, HALF_LOCI=1)),
    ("long rows", dict(n_long=2)),
    ("heavy loci", dict(n_heavy=1)),
    ("acc handed out", dict(acc_out=1)),
    ("posteriors", dict(flags=["POSTERIOR"])),
    ("resampling", dict(flags=["RESAMPLE"])),
    ("pair mode", dict(pair=1)),
    ("block sums too small for 8 slots per tile", dict(n_tiles=513, msum_cap=4096)),
    ("GBRS_TUNING_NO_GATHER_MSTEP=1", dict(NO_GATHER_MSTEP=1)),
]


@pytest.mark.parametrize("why,row", ROWS, ids=[r[0] for r in ROWS])
def test_not_taken(driver, why, row):
    assert taken(driver, **row) == 0, why


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_haplotype_counts_taken(driver, H):
    assert taken(driver, H=H) == 1


def test_edges(driver):
    assert taken(driver, n_tiles=512, msum_cap=4096) == 1                  # exactly 8 slots per tile
    assert taken(driver, NO_GATHER_MSTEP=0) == 1                           # counts when set and non-zero
    assert taken(driver, PERSISTENT=0, PERSISTENT_GROUPS=4) == 1
