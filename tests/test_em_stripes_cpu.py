"""Stripes in the plan of an EM handle (gbrs_amd/csrc/em_plan.h): which layouts take them (em_take_stripes), what
GBRS_TUNING_STRIPES means, and which stripe S a run of one tile gets under the padding cap (em_stripe_pick).  Host C++ only:
tests/native/em_stripes_driver.cpp is compiled by the host compiler, as tests/test_em_plan_cpu.py compiles its driver.

The size clause is em_take_fold's: the layout's words, times the handles side by side, over the chip's places for E-step
workgroups (3 per CU for unweighted rows of up to 8 haplotypes) must reach TILE_WORDS = 2048."""
import pytest

from em_plan_tool import N_CU, build_driver, plan

ROUND = 3 * N_CU * 2048        # words that give every place of the chip one tile of TILE_WORDS


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_stripes"), "em_stripes_driver")


def stripes(got):
    return got["stripes_one"], got["stripes_two"], got["stripes_forced"]


def test_default_is_the_rule_where_the_kernels_read_counted_runs(driver):
    for H in (1, 2, 4, 8):
        got = plan(driver, H=H)
        assert got["counted_pairs"] == 1 and stripes(got) == (-1, -1, 0)


def test_size_clause(driver):
    assert plan(driver, rule="take=%d" % ROUND)["take"] == 1
    assert plan(driver, rule="take=%d" % (ROUND - 1))["take"] == 0
    assert plan(driver, rule="take=0")["take"] == 0
    # handles side by side fill the places together
    assert plan(driver, flags=["SIDE_BY_SIDE"], rule="take=%d" % (ROUND // 2))["take"] == 1
    assert plan(driver, flags=["SIDE_BY_SIDE"], rule="take=%d" % (ROUND // 2 - 1))["take"] == 0
    # fewer compute units, fewer places
    assert plan(driver, n_cu=8, rule="take=%d" % (3 * 8 * 2048))["take"] == 1
    assert plan(driver, n_cu=8, rule="take=%d" % (3 * 8 * 2048 - 1))["take"] == 0


EXCLUDED = [dict(counts=1), dict(flags=["MERGE_IDENTICAL_ROWS"]), dict(flags=["RESAMPLE"]), dict(flags=["DETERMINISTIC"]),
            dict(H=16), dict(H=16, HALF_LOCI=1), dict(H=3), dict(H=5), dict(flags=["NO_STREAMS"]), dict(flags=["FORCE_INTERLEAVE"]),
            dict(flags=["LAYOUT_CSC"]), dict(H=17)]


@pytest.mark.parametrize("kind", EXCLUDED, ids=lambda k: "-".join(str(v) for v in k.values()).replace("'", ""))
def test_excluded_layouts_never_take_stripes_and_ignore_the_variable(driver, kind):
    for tuning in ({}, {"STRIPES": 4}, {"STRIPES": "8,2"}):
        got = plan(driver, rule="take=%d" % (10 * ROUND), **kind, **tuning)
        assert got["counted_pairs"] == 0 and stripes(got) == (0, 0, 0) and got["take"] == 0


@pytest.mark.parametrize("S", [2, 4, 8])
def test_the_variable_forces_a_stripe_whatever_the_size(driver, S):
    got = plan(driver, STRIPES=S, rule="take=1")
    assert stripes(got) == (S, S, 1) and got["take"] == 1
    # ... and whatever the cap: the forced value is the pick
    assert plan(driver, rule="pick=%d,100,400,200" % S)["pick"] == S


def test_the_variable_switches_stripes_off(driver):
    got = plan(driver, STRIPES=0, rule="take=%d" % (10 * ROUND))
    assert stripes(got) == (0, 0, 0) and got["take"] == 0
    assert plan(driver, rule="pick=0,800,800,800")["pick"] == 0


def test_other_values_leave_the_rule_in_charge(driver):
    for v in (1, 3, 16, -4, "x", ""):
        got = plan(driver, STRIPES=v, rule="take=%d" % ROUND)
        assert stripes(got) == (-1, -1, 0) and got["take"] == 1


def test_one_value_per_run(driver):
    """"S1,S2": the one-word runs and the pair runs apart (the candidates of profiles/estep_stripes.txt)."""
    assert stripes(plan(driver, STRIPES="4,2")) == (4, 2, 1)
    assert stripes(plan(driver, STRIPES="0,4")) == (0, 4, 1)
    assert stripes(plan(driver, STRIPES="8,0")) == (8, 0, 1)
    got = plan(driver, STRIPES="0,0", rule="take=%d" % (10 * ROUND))
    assert stripes(got) == (0, 0, 0) and got["take"] == 0


def test_padding_cap(driver):
    """The largest of 4 and 2 whose padded cells stay within (1 + c) x the run's words, c = cap_num / cap_den."""
    got = plan(driver)
    num, den = got["cap_num"], got["cap_den"]
    assert (num, den) == (1, 4)
    words = 8000
    edge = words * (den + num) // den          # 10,000: the most cells the cap lets through
    assert plan(driver, rule="pick=-1,%d,%d,%d" % (words, edge, words))["pick"] == 4
    assert plan(driver, rule="pick=-1,%d,%d,%d" % (words, edge + 1, edge))["pick"] == 2
    assert plan(driver, rule="pick=-1,%d,%d,%d" % (words, edge + 1, edge + 1))["pick"] == 0
    # ids of one word each: 4 and 2 cells a word
    assert plan(driver, rule="pick=-1,%d,%d,%d" % (words, 4 * words, 2 * words))["pick"] == 0
    # no padding at all
    assert plan(driver, rule="pick=-1,%d,%d,%d" % (words, words, words))["pick"] == 4
