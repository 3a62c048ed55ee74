"""The route of an HMM pass (gbrs_amd/csrc/hmm_route.h): which kernels run the alpha / backward sweeps, the delta chain
and the backpointers for a handle's shape under the GBRS_TUNING_HMM_* variables.  The header is host C++ only, so it is
compiled here with tests/native/hmm_route_driver.cpp by the host compiler and run once per row with the row's
environment.  The expected routes were derived by reading hmm_launch as it stood before the route existed (one
difference, on purpose: the samples-on-lanes delta chain excludes the blocked scan, as the MFMA sweeps always did -
before, that combination ran the lanes chain and then skipped the backpointer kernel, whose rows nobody had written)."""
import os
import shutil
import subprocess

import pytest

import hmm_batched_cases
from conftest import ROOT

PREFIX = "GBRS_TUNING_HMM_"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("hmm_route") / "hmm_route_driver"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "native", "hmm_route_driver.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return str(exe)


def route(driver, founders, n_samples, n_chrom=2, total_trans=103, **tuning):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GBRS_TUNING_HMM_", "GBRS_DIAG_HMM_"))}
    env.update({PREFIX + k: str(v) for k, v in tuning.items()})
    run = subprocess.run([driver, str(founders), str(n_samples), str(n_chrom), str(total_trans)], capture_output=True,
                         text=True, env=env, timeout=60)
    assert run.returncode == 0, run.stderr
    return dict(kv.split("=") for kv in run.stdout.split())


def expect(got, sweep, delta, bp, **more):
    want = dict(sweep=sweep, delta=delta, bp=bp, batched=0, mfma_groups=0, deferred=0, grouped=0, delta_interleaved=0,
                tie_check=0, serial=0, back_after=0, bp_after=0, delta_after_ops=0,
                free_backward=int(sweep != "generic"))
    want.update(more)
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}


BLOCKED = dict(sweep="blocked", delta="blocked_rank", bp="chains", tie_check=1, tol_abs="1e-09", tol_rel="1e-13")


@pytest.mark.parametrize("n_samples", [1, 2, 4])
def test_36_states_blocked_scan_up_to_4_samples(driver, n_samples):
    expect(route(driver, 8, n_samples), **BLOCKED)


@pytest.mark.parametrize("n_samples,batched,bp", [(5, 0, "generic"), (23, 0, "generic"), (24, 1, "generic"),
                                                  (31, 1, "generic"), (32, 1, "lanes"), (63, 1, "lanes")])
def test_36_states_wave_chains(driver, n_samples, batched, bp):
    expect(route(driver, 8, n_samples), "wave", "wave", bp, batched=batched)


def batched_case_route(driver, c):
    got = route(driver, c.founders, c.n_samples, **{k[len(PREFIX):]: v for k, v in c.env.items()})
    return {k: got[k] for k in ("sweep", "delta", "bp", "batched")}


@pytest.mark.parametrize("case", hmm_batched_cases.CASES, ids=hmm_batched_cases.case_id)
def test_batched_case_table_routes(driver, case):
    """Every row of tests/hmm_batched_cases.py resolves to the route it names: tests/test_hmm_batched_wave_gpu.py runs
    these rows to cover the kernels behind that route.  A row that fails here no longer reaches them - re-aim it."""
    assert all(k.startswith(PREFIX) for k in case.env)
    assert batched_case_route(driver, case) == dict(sweep=case.sweep, delta=case.delta, bp=case.bp, batched=str(case.batched))


def test_batched_case_table_covers_both_backpointer_kernels(driver):
    """Behind the two-samples-per-wave delta chain with the library's defaults: viterbi_bp_kernel and
    viterbi_bp_lanes_kernel each read its rows in some row of the table."""
    got = [batched_case_route(driver, c) for c in hmm_batched_cases.CASES if c.founders == 8 and not c.env]
    assert {r["bp"] for r in got if r["batched"] == "1" and r["delta"] == "wave"} >= {"generic", "lanes"}


@pytest.mark.parametrize("n_samples", [64, 65, 256])
def test_36_states_mfma_from_64_samples(driver, n_samples):
    # [sample][gene] delta rows; never the grouped pass
    expect(route(driver, 8, n_samples), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, xcd_mask=0, xcd_span=2)


@pytest.mark.parametrize("founders", [7, 4, 3])       # 28, 10 and 6 states
def test_other_wave_state_counts(driver, founders):
    expect(route(driver, founders, 1), "wave", "wave", "wave")
    expect(route(driver, founders, 4), "wave", "wave", "wave")
    expect(route(driver, founders, 5), "wave", "wave", "generic")
    expect(route(driver, founders, 64), "wave", "wave", "generic", batched=1)
    expect(route(driver, founders, 2, BLOCKED=2, MFMA=1, DLANES=1, BPLANES=1), "wave", "wave", "wave")


def test_136_states_quad_chains(driver):
    for n_samples in (1, 64):
        expect(route(driver, 16, n_samples), "quad", "with_sweep", "quad")


@pytest.mark.parametrize("founders", [1, 2, 5, 6, 9, 10, 11, 15])
def test_other_state_counts_generic_fused(driver, founders):
    for n_samples in (1, 64):
        expect(route(driver, founders, n_samples), "generic", "with_sweep", "with_sweep")


def test_no_transition_blocks_switch_mfma_blocked_and_lanes_off(driver):
    expect(route(driver, 8, 2, total_trans=0), "wave", "wave", "wave")
    expect(route(driver, 8, 64, total_trans=0), "wave", "wave", "generic", batched=1)
    expect(route(driver, 8, 64, total_trans=0, PIPELINE=16, DELTA_ROWS=1), "wave", "wave", "generic", batched=1)


def test_thresholds(driver):
    expect(route(driver, 8, 16, MFMA=16, DLANES=16), "mfma", "lanes", "generic", mfma_groups=1)
    expect(route(driver, 8, 15, MFMA=16, DLANES=16), "wave", "wave", "generic")
    expect(route(driver, 8, 64, MFMA=0), "wave", "lanes", "lanes", batched=1)
    expect(route(driver, 8, 64, DLANES=0), "mfma", "wave", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 8, 64, DLANES=-1), "mfma", "wave", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 8, 64, BPLANES=0), "mfma", "lanes", "generic", batched=1, mfma_groups=1)
    expect(route(driver, 8, 8, BPLANES=8), "wave", "wave", "lanes")
    expect(route(driver, 8, 2, MFMA=0), **BLOCKED)
    # without the blocked scan the backpointers of 4 or fewer samples come from the wave kernel
    expect(route(driver, 8, 2, BLOCKED=0), "wave", "wave", "wave")
    expect(route(driver, 8, 6, BLOCKED=6), **BLOCKED)
    expect(route(driver, 8, 2, MFMA=2), "mfma", "wave", "wave", mfma_groups=1)


def test_blocked_delta_schemes(driver):
    expect(route(driver, 8, 2, BLOCKED=2, DELTA_SPEC=0), **dict(BLOCKED, delta="blocked_ops"))
    expect(route(driver, 8, 3, BLOCKED=2, DELTA_SPEC=0), "wave", "wave", "wave")
    expect(route(driver, 8, 2, BLOCKED=2, DELTA_TOL=-1), **dict(BLOCKED, tol_abs="-1", tol_rel="0"))
    expect(route(driver, 8, 2, DELTA_TOL="1e-6"), **dict(BLOCKED, tol_abs="1e-06"))
    expect(route(driver, 8, 1, DELTA_AFTER_OPS=1), **dict(BLOCKED, delta_after_ops=1))


def test_blocked_scan_gives_way_to_the_lanes_delta_chain(driver):
    # not blocked, and a backpointer kernel runs
    expect(route(driver, 8, 2, BLOCKED=2, DLANES=1, MFMA=0), "wave", "lanes", "wave")
    expect(route(driver, 8, 6, BLOCKED=6, DLANES=1, MFMA=0), "wave", "lanes", "generic")
    expect(route(driver, 8, 6, BLOCKED=6, DLANES=1, MFMA=0, BPLANES=1), "wave", "lanes", "lanes")


def test_mfma_groups(driver):
    expect(route(driver, 8, 64, MFMA_NG=2), "mfma", "lanes", "lanes", batched=1, mfma_groups=2)
    expect(route(driver, 8, 64, MFMA_NG=1), "mfma", "lanes", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 8, 64, MFMA_NG=3), "mfma", "lanes", "lanes", batched=1, mfma_groups=1)
    # two groups per wavefront: never the grouped pass, even with PIPELINE - the deferred emission is flushed
    expect(route(driver, 8, 64, MFMA_NG=2, PIPELINE=16), "mfma", "lanes", "lanes", batched=1, mfma_groups=2, deferred=1)


def test_pipeline(driver):
    expect(route(driver, 8, 16, PIPELINE=16, MFMA=16, DLANES=16), "mfma", "lanes", "generic", mfma_groups=1, deferred=1, grouped=1)
    expect(route(driver, 8, 64, PIPELINE=16), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, deferred=1, grouped=1)
    expect(route(driver, 8, 64, PIPELINE=16, DELTA_ROWS=1), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, deferred=1, grouped=1)
    # deferred when the expression is set, flushed by the run: its route is not made of the grouped pass's kernels
    expect(route(driver, 8, 16, PIPELINE=16), "wave", "wave", "generic", deferred=1)
    expect(route(driver, 8, 16, PIPELINE=16, MFMA=16), "mfma", "wave", "generic", mfma_groups=1, deferred=1)
    expect(route(driver, 8, 15, PIPELINE=16, MFMA=1, DLANES=1), "mfma", "lanes", "generic", mfma_groups=1)
    expect(route(driver, 8, 64, PIPELINE=0), "mfma", "lanes", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 8, 64, n_chrom=1, PIPELINE=16), "mfma", "lanes", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 7, 64, PIPELINE=16), "wave", "wave", "generic", batched=1)


def test_xcd_grids(driver):
    expect(route(driver, 8, 64, XCD=3), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, xcd_mask=3, xcd_span=2)
    expect(route(driver, 8, 64, XCD=3, XCD_SPAN=3), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, xcd_mask=3, xcd_span=2)
    for span in (1, 2, 4):
        expect(route(driver, 8, 64, XCD=1, XCD_SPAN=span), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, xcd_mask=1, xcd_span=span)


def test_delta_rows_interleaved_only_where_both_lanes_kernels_run(driver):
    expect(route(driver, 8, 64, DELTA_ROWS=1), "mfma", "lanes", "lanes", batched=1, mfma_groups=1, delta_interleaved=1)
    expect(route(driver, 8, 64, DELTA_ROWS=0), "mfma", "lanes", "lanes", batched=1, mfma_groups=1)
    expect(route(driver, 8, 32, DELTA_ROWS=1), "wave", "wave", "lanes", batched=1)
    expect(route(driver, 8, 16, DELTA_ROWS=1, DLANES=16), "wave", "lanes", "generic")
    expect(route(driver, 8, 16, DELTA_ROWS=1, DLANES=16, BPLANES=16), "wave", "lanes", "lanes", delta_interleaved=1)
    expect(route(driver, 8, 64, DELTA_ROWS=1, BPLANES=0), "mfma", "lanes", "generic", batched=1, mfma_groups=1)


def test_stream_ordering_switches(driver):
    expect(route(driver, 8, 8, SERIAL=1), "wave", "wave", "generic", serial=1)
    expect(route(driver, 8, 8, BACK_AFTER=1), "wave", "wave", "generic", back_after=1)
    expect(route(driver, 8, 8, BP_AFTER=1), "wave", "wave", "generic", bp_after=1)
    expect(route(driver, 8, 8, SERIAL=0, BACK_AFTER=0, BP_AFTER=0), "wave", "wave", "generic")


def test_block_and_group_cuts(driver):
    defaults = dict(block_genes=40, blocks_max=64, head=0, pipe_first=30)
    expect(route(driver, 8, 1), **BLOCKED, **defaults)
    expect(route(driver, 8, 1, BLOCK_GENES=5, BLOCKS_MAX=7, HEAD=40, PIPE_FIRST=50), **BLOCKED, block_genes=5, blocks_max=7,
           head=40, pipe_first=50)
    expect(route(driver, 8, 1, BLOCK_GENES=1, BLOCKS_MAX=0, HEAD=-3, PIPE_FIRST=100), **BLOCKED, **defaults)
    expect(route(driver, 8, 1, BLOCK_GENES=2, BLOCKS_MAX=1, HEAD=95, PIPE_FIRST=99), **BLOCKED, block_genes=2, blocks_max=1,
           head=90, pipe_first=99)
    expect(route(driver, 8, 1, PIPE_FIRST=0), **BLOCKED, **defaults)
