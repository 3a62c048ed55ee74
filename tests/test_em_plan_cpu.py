"""The plan of an EM handle (gbrs_amd/csrc/em_plan.h): what gbrs_em_create* resolves from the handle's shape, its flags and
the GBRS_TUNING_* variables before any device work, and the rules the tile layout's build applies to the numbers it reads
back from the device.  The header is host C++ only, so it is compiled here with tests/native/em_plan_driver.cpp by the
host compiler and run once per row with the row's environment.  The expected values were derived by reading
em_create_impl and build_tile_layout as they stood before the plan existed, with the constants of em_layout.h:
TILE_WORDS 2048, GBRS_TILE_CAP 32768, 3072 / 4608 / 4800 doubles of theta in LDS (unweighted / weighted / 16 haplotypes),
rows of up to 32 (H <= 8) or 8 words, 8 waves per workgroup."""
import pytest

from em_plan_tool import N_CU, build_driver, plan

TILE_WORDS, TILE_WORDS_MAX = 2048, 32768 - 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_plan"))


# an unweighted handle of 8 haplotypes on 256 CUs, no flag, no variable
DEFAULT = dict(tiled=1, view=1, tH=8, tL=400, row_order=2, merge=0, deterministic=0, weighted=0, side_by_side=1, locus_sets=1,
               whole_row_sets=0, group_sets=1, group_sets_forced=0, sets_forced=-1, set_min_rows=192, counted_pairs=1, fold=1,
               fold_mode=3, fold_forced=0, per_cu=3, places=3 * N_CU, tile_words_forced=0, reorder_tiles=1, d_max=384, dseg=352,
               dict_room=1, persist_groups=0, lead_mask=0xFFFFFFFF, resample_cut=256)
# what per-row weights change: two workgroups per CU, the larger dictionaries, no locus sets, no folds
WEIGHTED = dict(weighted=1, per_cu=2, places=2 * N_CU, d_max=576, dseg=544, locus_sets=0, group_sets=0, counted_pairs=0, fold=0)


def expect(got, **changes):
    want = dict(DEFAULT, **changes)
    assert {k: got[k] for k in want} == want


# ---- the plan ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,d_max,counted", [(1, 1024, 1), (2, 1024, 1), (3, 1024, 0), (4, 768, 1), (8, 384, 1)])
def test_defaults_up_to_8_haplotypes(driver, H, d_max, counted):
    # min(1024, 3072 / H) dictionary entries, 32 of them a row's own; the folds where the kernels read the counts
    expect(plan(driver, H=H), tH=H, d_max=d_max, dseg=d_max - 32, counted_pairs=counted, fold=counted)


def test_defaults_16_haplotypes(driver):
    # 4800 / 16 entries, rows of 8 words, two workgroups per CU, no kernel that reads a two-word count
    expect(plan(driver, H=16), tH=16, d_max=300, dseg=292, per_cu=2, places=2 * N_CU, counted_pairs=0, fold=0)


def test_17_haplotypes_take_the_csc_kernels(driver):
    got = plan(driver, H=17)
    assert (got["tiled"], got["persist_groups"], got["lead_mask"], got["resample_cut"]) == (0, 0, 0xFFFFFFFF, 256)
    assert plan(driver, flags=["LAYOUT_CSC"])["tiled"] == 0
    assert plan(driver, N=0xFFFFFFFF)["tiled"] == 0
    assert plan(driver, N=0xFFFFFFFE)["tiled"] == 1


def test_create_flags(driver):
    expect(plan(driver, flags=["MERGE_IDENTICAL_ROWS"]), merge=1, **WEIGHTED)
    expect(plan(driver, counts=1), **WEIGHTED)
    # one private copy of a tile's sums per wavefront: ((3072 + 64) / 8 - 1) / 8 entries
    expect(plan(driver, flags=["DETERMINISTIC"]), deterministic=1, d_max=48, dseg=16, counted_pairs=0, fold=0)
    expect(plan(driver, flags=["DETERMINISTIC"], counts=1), deterministic=1, **dict(WEIGHTED, d_max=72, dseg=40))
    expect(plan(driver, flags=["SIDE_BY_SIDE"]), side_by_side=2)
    expect(plan(driver, flags=["NO_LOCUS_SETS"]), locus_sets=0, group_sets=0)
    expect(plan(driver, flags=["NO_RUN_WORDS"]), fold=0)
    expect(plan(driver, flags=["ONE_SHOT"]))
    # a resampling handle is a weighted one; the cut is its own
    expect(plan(driver, flags=["RESAMPLE"]), **WEIGHTED)
    expect(plan(driver, flags=["RESAMPLE"], counts=1), **WEIGHTED)


def test_row_orders(driver):
    # without the streams: distinct rows (counts, merged) interleave unless told not to, raw reads stay sorted
    off = dict(counted_pairs=0, fold=0)
    expect(plan(driver, flags=["NO_STREAMS"]), row_order=0, **off)
    expect(plan(driver, flags=["NO_STREAMS", "NO_INTERLEAVE"]), row_order=0, **off)
    expect(plan(driver, flags=["NO_STREAMS"], counts=1), row_order=1, **WEIGHTED)
    expect(plan(driver, flags=["NO_STREAMS", "MERGE_IDENTICAL_ROWS"]), row_order=1, merge=1, **WEIGHTED)
    expect(plan(driver, flags=["NO_STREAMS", "NO_INTERLEAVE"], counts=1), row_order=0, **WEIGHTED)
    expect(plan(driver, flags=["FORCE_INTERLEAVE"]), row_order=1, **off)
    expect(plan(driver, flags=["FORCE_INTERLEAVE", "NO_STREAMS", "NO_INTERLEAVE"]), row_order=1, **off)


def test_tile_words_variable(driver):
    assert plan(driver, TILE_WORDS=63)["tile_words_forced"] == 0
    assert plan(driver, TILE_WORDS=64)["tile_words_forced"] == 64
    assert plan(driver, TILE_WORDS=1000)["tile_words_forced"] == 1000
    assert plan(driver, TILE_WORDS=TILE_WORDS_MAX + 1)["tile_words_forced"] == TILE_WORDS_MAX
    assert plan(driver, TILE_WORDS=63, rule="tile=%d" % (3 * N_CU * 5000))["tile"] == 4992
    assert plan(driver, TILE_WORDS=1000, rule="tile=%d" % (3 * N_CU * 5000))["tile"] == 1000
    assert plan(driver, TILE_WORDS=40000, rule="tile=1")["tile"] == TILE_WORDS_MAX


def test_dict_cap_variable(driver):
    # taken only when it leaves room beside a row's 32 (8 at 16 haplotypes) words
    expect(plan(driver, DICT_CAP=32))
    expect(plan(driver, DICT_CAP=33), d_max=33, dseg=1)
    expect(plan(driver, DICT_CAP=1000))
    expect(plan(driver, H=16, DICT_CAP=8), tH=16, d_max=300, dseg=292, per_cu=2, places=2 * N_CU, counted_pairs=0, fold=0)
    expect(plan(driver, H=16, DICT_CAP=9), tH=16, d_max=9, dseg=1, per_cu=2, places=2 * N_CU, counted_pairs=0, fold=0)


def test_locus_set_variables(driver):
    expect(plan(driver, SET_MIN_ROWS=0))
    expect(plan(driver, SET_MIN_ROWS=1), set_min_rows=1)
    expect(plan(driver, SET_MIN_ROWS=16), set_min_rows=16)
    # LOCUS_SETS=1: the whole-row form, taken (the mask groups run only when it found no set); 0: that form's rule says no
    expect(plan(driver, LOCUS_SETS=1), whole_row_sets=1, sets_forced=1)
    expect(plan(driver, LOCUS_SETS=0), sets_forced=0)
    expect(plan(driver, LOCUS_SETS=1, counts=1), **dict(WEIGHTED, sets_forced=1))
    expect(plan(driver, GROUP_SETS=0), group_sets=0)
    expect(plan(driver, GROUP_SETS=1), group_sets_forced=1)
    expect(plan(driver, GROUP_SETS=1, flags=["NO_LOCUS_SETS"]), locus_sets=0, group_sets=0, group_sets_forced=1)


def test_run_words_variable(driver):
    expect(plan(driver, RUN_WORDS=0), fold=0, fold_forced=1)
    expect(plan(driver, RUN_WORDS=1), fold_mode=2, fold_forced=1)
    expect(plan(driver, RUN_WORDS=2), fold_forced=1)
    # forces the choice where the fold exists, not the fold where the kernels do not read counts
    expect(plan(driver, RUN_WORDS=2, counts=1), **dict(WEIGHTED, fold_forced=1))
    expect(plan(driver, RUN_WORDS=2, flags=["NO_RUN_WORDS"]), fold=0, fold_forced=1)


def test_half_loci(driver):
    h16 = dict(tH=16, d_max=300, dseg=292, per_cu=2, places=2 * N_CU, counted_pairs=0, fold=0)
    # 2 L half-loci of 8 haplotypes on the 8-haplotype kernels' dictionaries and places, without their folds
    expect(plan(driver, H=16, HALF_LOCI=1), view=2, tH=8, tL=800, counted_pairs=0, fold=0)
    expect(plan(driver, H=16, HALF_LOCI=0), **h16)
    expect(plan(driver, H=8, HALF_LOCI=1))
    expect(plan(driver, H=16, HALF_LOCI=1, counts=1), **dict(WEIGHTED, tH=16, d_max=288, dseg=280))
    expect(plan(driver, H=16, HALF_LOCI=1, flags=["MERGE_IDENTICAL_ROWS"]), merge=1, **dict(WEIGHTED, tH=16, d_max=288, dseg=280))
    # ((4800 + 64) / 8 - 1) / 16 entries
    expect(plan(driver, H=16, HALF_LOCI=1, flags=["DETERMINISTIC"]), deterministic=1, **dict(h16, d_max=37, dseg=29))
    expect(plan(driver, H=16, L=(1 << 26) - 1, HALF_LOCI=1), view=2, tH=8, tL=(1 << 27) - 2, counted_pairs=0, fold=0)
    expect(plan(driver, H=16, L=1 << 26, HALF_LOCI=1), tL=1 << 26, **h16)


def test_persistent_groups(driver):
    expect(plan(driver, PERSISTENT=0, PERSISTENT_GROUPS=5))
    expect(plan(driver, PERSISTENT_GROUPS=5))
    expect(plan(driver, PERSISTENT=1), persist_groups=3 * N_CU)
    expect(plan(driver, PERSISTENT=1, counts=1), **dict(WEIGHTED, persist_groups=2 * N_CU))
    expect(plan(driver, PERSISTENT=1, flags=["SIDE_BY_SIDE"]), side_by_side=2, persist_groups=3 * N_CU // 2)
    expect(plan(driver, PERSISTENT=1, PERSISTENT_GROUPS=5), persist_groups=5)
    expect(plan(driver, PERSISTENT=1, PERSISTENT_GROUPS=5, flags=["SIDE_BY_SIDE"]), side_by_side=2, persist_groups=5)
    expect(plan(driver, PERSISTENT=1, PERSISTENT_GROUPS=0), persist_groups=3 * N_CU)
    # a device that reports no CU count still gets one workgroup
    expect(plan(driver, PERSISTENT=1, n_cu=0, flags=["SIDE_BY_SIDE"]), side_by_side=2, places=3, persist_groups=1)


def test_other_switches(driver):
    expect(plan(driver, TILE_ORDER=0), reorder_tiles=0)
    expect(plan(driver, TILE_ORDER=1))
    expect(plan(driver, NO_PHASE_SPLIT=1), lead_mask=0)
    expect(plan(driver, NO_PHASE_SPLIT=0))
    # read by a resampling handle with counts only
    expect(plan(driver, RESAMPLE_CUT=16))
    expect(plan(driver, RESAMPLE_CUT=16, flags=["RESAMPLE"]), **WEIGHTED)
    expect(plan(driver, RESAMPLE_CUT=16, flags=["RESAMPLE"], counts=1), **dict(WEIGHTED, resample_cut=16))
    expect(plan(driver, RESAMPLE_CUT=0, flags=["RESAMPLE"], counts=1), **WEIGHTED)


# ---- the rules that take a number from the device -------------------------------------------------------------------------

def test_tile_size_rule(driver):
    """As many words as leave one round of the chip's places (3 * 256 here, 2 * 256 for weighted rows), between TILE_WORDS
    and the cap, a multiple of 64."""
    places = 3 * N_CU
    assert plan(driver, rule="tile=%d" % (places * 2047))["tile"] == TILE_WORDS
    assert plan(driver, rule="tile=0")["tile"] == TILE_WORDS
    assert plan(driver, rule="tile=%d" % (places * 5000))["tile"] == 4992
    assert plan(driver, rule="tile=%d" % (places * 5056 - 1))["tile"] == 4992
    assert plan(driver, rule="tile=%d" % (places * 5056))["tile"] == 5056
    assert plan(driver, rule="tile=%d" % (places * 40000))["tile"] == TILE_WORDS_MAX
    # handles side by side fill the rounds together
    assert plan(driver, flags=["SIDE_BY_SIDE"], rule="tile=%d" % (places * 2500))["tile"] == 4992
    # weighted rows stay at 16,320
    assert plan(driver, counts=1, rule="tile=%d" % (2 * N_CU * 16320))["tile"] == 16320
    assert plan(driver, counts=1, rule="tile=%d" % (2 * N_CU * 20000))["tile"] == 16320
    assert plan(driver, counts=1, rule="tile=%d" % (2 * N_CU * 16319))["tile"] == 16256


def test_fold_rule(driver):
    """Taken from 15 % of the words on, when the words left still fill one round of places with tiles of TILE_WORDS."""
    assert plan(driver, rule="fold=2000000,300000")["fold_taken"] == 1
    assert plan(driver, rule="fold=2000000,299999")["fold_taken"] == 0
    round_words = 3 * N_CU * TILE_WORDS
    assert plan(driver, rule="fold=%d,400000" % (round_words + 400000))["fold_taken"] == 1
    assert plan(driver, rule="fold=%d,400001" % (round_words + 400000))["fold_taken"] == 0
    assert plan(driver, rule="fold=1800000,300000")["fold_taken"] == 0
    assert plan(driver, flags=["SIDE_BY_SIDE"], rule="fold=1800000,300000")["fold_taken"] == 1
    for forced in (1, 2):
        assert plan(driver, RUN_WORDS=forced, rule="fold=1800000,1")["fold_taken"] == 1


def test_whole_row_set_rule(driver):
    """At most 85 % of the pairs left, at least 100 pairs per id (loci + sets), at most two sets per locus."""
    assert plan(driver, rule="whole=100000,85000,400,100")["whole"] == 1
    assert plan(driver, rule="whole=100000,85001,400,100")["whole"] == 0
    assert plan(driver, rule="whole=1000000,850000,400,800")["whole"] == 1
    assert plan(driver, rule="whole=1000000,850000,400,801")["whole"] == 0
    assert plan(driver, rule="whole=100000,50000,400,100")["whole"] == 1
    assert plan(driver, rule="whole=100000,49999,400,100")["whole"] == 0
    assert plan(driver, LOCUS_SETS=1, rule="whole=100000,99999,400,5000")["whole"] == 1
    assert plan(driver, LOCUS_SETS=0, rule="whole=100000,50000,400,100")["whole"] == 0


def test_group_set_rules(driver):
    """At most 95 % of the pairs left; no more sets than half the loci, or the rows a set needs double."""
    assert plan(driver, rule="group=100000,95000")["group"] == 1
    assert plan(driver, rule="group=100000,95001")["group"] == 0
    assert plan(driver, GROUP_SETS=1, rule="group=100000,100000")["group"] == 1
    assert plan(driver, rule="fit=200,400")["fit"] == 1
    assert plan(driver, rule="fit=201,400")["fit"] == 0
    assert plan(driver, GROUP_SETS=1, rule="fit=201,400")["fit"] == 1
