"""The route of one pass over an EM handle (gbrs_amd/csrc/em_step.h): which E-step kernel instance runs, whether the long-row
kernel runs, how much of `acc` the gather writes, whether gather and M-step share a launch, which M-step kernel runs and
whether an error pass rides on the tile launch or is left for the next one.  The header is host C++ only, so it is compiled
here with tests/native/em_step_driver.cpp by the host compiler and run once per row with the row's environment.  The
expected routes were derived by reading em.hip as it stood before the route existed: em_estep_tiles_h / em_estep_tiles /
em_estep, em_can_fuse_mstep, em_launch_mstep, em_finish_step, em_one_step and em_model_step."""
import pytest

from em_plan_tool import build_driver, route


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_step"), "em_step_driver")


# one model-4 iteration of an unweighted handle of 8 haplotypes: tiles, no long rows, no flag, no variable
FUSED = dict(estep="tiles", width=8, weighted=0, long_rows="none", gather="none", mstep="fused", mstep_adds_extra=0,
             counts_stale=1, err_rides=1, err_defer=1)
# gather and M-step as two launches over every element of acc
TWO_ALL = dict(gather="all", mstep="elem", counts_stale=0)
# the CSC kernels: they write acc themselves, nothing rides and nothing is deferred
CSC = dict(estep="csc", width=0, gather="none", mstep="elem", counts_stale=0, err_rides=0, err_defer=0)


def expect(got, **changes):
    want = dict(FUSED, **changes)
    assert {k: got[k] for k in want} == want


def test_h8_tiles_fused(driver):                                        # rows 1, 2
    expect(route(driver))
    expect(route(driver, n_long=3), long_rows="atomic")


def test_one_word_instance_at_8_unweighted_only(driver):                # rows 3a-c
    expect(route(driver, all_one_word=1), estep="tiles_one_word")
    expect(route(driver, all_one_word=1, counts=1), weighted=1)
    expect(route(driver, all_one_word=1, flags=["MERGE_IDENTICAL_ROWS"]), weighted=1)
    expect(route(driver, H=4, all_one_word=1), width=4)
    expect(route(driver, H=16, all_one_word=1), width=16)


def test_deterministic(driver):                                         # row 4
    expect(route(driver, flags=["DETERMINISTIC"], n_long=3), estep="tiles_deterministic", long_rows="serial")
    expect(route(driver, flags=["DETERMINISTIC"], counts=1, all_one_word=1), estep="tiles_deterministic", weighted=1)


@pytest.mark.parametrize("H", [3, 5, 6, 7, 9, 12, 15])
def test_other_haplotype_counts_up_to_16(driver, H):                    # row 5
    expect(route(driver, H=H, n_long=3), width=0, long_rows="atomic", gather="all", mstep="per_locus", counts_stale=0)


@pytest.mark.parametrize("H", [1, 2, 4, 16])
def test_template_widths(driver, H):
    expect(route(driver, H=H), width=H)


def test_half_loci(driver):                                             # row 6
    got = route(driver, H=16, HALF_LOCI=1)
    assert (got["tH"], got["view"]) == (8, 2)
    expect(got, **TWO_ALL)
    expect(route(driver, H=16, HALF_LOCI=1, n_long=2), long_rows="atomic", **TWO_ALL)


def test_no_fused_mstep(driver):                                        # rows 7, 7b
    two = dict(gather="written", mstep="elem", counts_stale=0)
    expect(route(driver, n_long=3, NO_FUSED_MSTEP=1), long_rows="atomic", mstep_adds_extra=1, **two)
    expect(route(driver, NO_FUSED_MSTEP=1), **two)
    expect(route(driver, n_long=3, NO_FUSED_MSTEP=0), long_rows="atomic")
    expect(route(driver, H=3, n_long=3, NO_FUSED_MSTEP=1), width=0, long_rows="atomic", gather="all", mstep="per_locus",
           counts_stale=0)


def test_tuning_variables_of_the_steps(driver):
    """NO_FUSED_MSTEP counts when set and non-zero, NO_FLOAT_CHECK when set at all."""
    for env, want in [({}, (0, 0)), (dict(NO_FUSED_MSTEP=0), (0, 0)), (dict(NO_FUSED_MSTEP=1), (1, 0)),
                      (dict(NO_FUSED_MSTEP=2, NO_FLOAT_CHECK=1), (1, 1)), (dict(NO_FLOAT_CHECK=0), (0, 1)),
                      (dict(NO_FLOAT_CHECK=""), (0, 1))]:
        got = route(driver, **env)
        assert (got["no_fused_mstep"], got["no_float_check"]) == want, env


def test_partial(driver):                                               # rows 8a, 8b
    for acc_out in (0, 1):
        expect(route(driver, "partial", n_long=3, acc_out=acc_out), long_rows="atomic", **TWO_ALL)
    expect(route(driver, "partial", H=3, acc_out=1), width=0, gather="all", mstep="per_locus", counts_stale=0)
    # a step of the handle's own after acc was handed out
    expect(route(driver, "step", n_long=3, acc_out=1), long_rows="atomic", **TWO_ALL)
    expect(route(driver, "step", acc_out=1), **TWO_ALL)


def test_prepare(driver):                                               # row 9
    ones = dict(err_rides=0, err_defer=0, **TWO_ALL)
    expect(route(driver, "prepare"), **ones)
    expect(route(driver, "prepare", PERSISTENT=1), **ones)
    expect(route(driver, "prepare", all_one_word=1, n_long=0), estep="tiles_one_word", **ones)
    expect(route(driver, "prepare", flags=["DETERMINISTIC"], n_long=2), estep="tiles_deterministic", long_rows="serial", **ones)
    expect(route(driver, "prepare", H=3), width=0, **dict(ones, mstep="per_locus"))
    expect(route(driver, "prepare", NO_FUSED_MSTEP=1, n_long=2), long_rows="atomic", **ones)


def test_persistent(driver):                                            # rows 10a-d
    expect(route(driver, PERSISTENT=1), estep="persistent")
    expect(route(driver, PERSISTENT=1, counts=1), estep="persistent", weighted=1)
    expect(route(driver, PERSISTENT=1, all_one_word=1), estep="persistent_one_word")
    expect(route(driver, PERSISTENT=1, all_one_word=1, counts=1), estep="persistent", weighted=1)
    expect(route(driver, PERSISTENT=1, H=4, all_one_word=1), estep="persistent", width=4)
    expect(route(driver, PERSISTENT=1, H=16), width=16)
    expect(route(driver, PERSISTENT=1, H=3), width=0, gather="all", mstep="per_locus", counts_stale=0)
    expect(route(driver, PERSISTENT=1, flags=["DETERMINISTIC"]), estep="tiles_deterministic")
    expect(route(driver, "partial", PERSISTENT=1, acc_out=1), estep="persistent", **TWO_ALL)
    expect(route(driver, PERSISTENT=0, PERSISTENT_GROUPS=4))


def test_csc(driver):                                                   # rows 11a-c
    expect(route(driver, H=17), **dict(CSC, mstep="per_locus"))
    expect(route(driver, H=32), **CSC)
    expect(route(driver, H=24), **dict(CSC, mstep="per_locus"))
    for kind in ("step", "partial", "prepare"):
        expect(route(driver, kind, flags=["LAYOUT_CSC"], n_long=3, all_one_word=1, PERSISTENT=1), **CSC)
    expect(route(driver, H=17, N=0), **dict(CSC, estep="none", mstep="per_locus"))


def test_no_tile_to_launch(driver):                                     # row 12
    expect(route(driver, n_tiles=0, n_long=1), estep="none", long_rows="atomic", err_rides=0)
    expect(route(driver, "partial", n_tiles=0, n_long=1, acc_out=1), estep="none", long_rows="atomic", err_rides=0, **TWO_ALL)
    expect(route(driver, n_tiles=0, n_long=1, PERSISTENT=1), estep="none", long_rows="atomic", err_rides=0)
    # a handle without entries
    expect(route(driver, N=0, n_tiles=0), estep="none", err_rides=0)


def test_models_1_to_3(driver):                                         # row 13
    model = dict(estep="models", width=0, gather="none", mstep="elem", counts_stale=0, err_rides=0, err_defer=0)
    expect(route(driver, "model", n_long=3), **model)
    expect(route(driver, "model", H=6), **dict(model, mstep="per_locus"))
    expect(route(driver, "model", flags=["LAYOUT_CSC"]), **model)
    expect(route(driver, "model", H=32), **model)
