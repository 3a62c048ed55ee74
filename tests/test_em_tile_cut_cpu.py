"""The pure functions of the exact tile cut (gbrs_amd/csrc/em_plan.h): the number of tiles the cut aims at, the first tile
size, the rescale step and the pass bound, and which handles take the cut at all.  tests/native/em_tile_cut_driver.cpp is
compiled with the host compiler, as em_plan_driver.cpp is; every expected value is a literal derived by hand from the rule:

  target  = places / side_by_side - err_blocks  (all the places when there are no more of them than error workgroups),
            places = 3 workgroups per CU (2: weighted rows, 16 haplotypes) x CUs; GBRS_TUNING_TILE_TARGET overrides
  first   = ceil(words / target), rounded UP to a multiple of 64, clamped to [2,048, cap]   (cap 32,704; weighted 16,320)
  rescale = ceil(tile_words x tiles / target), rounded and clamped the same way, never smaller; unchanged when
            tiles <= target
  passes  = 3 at most
"""
import subprocess

import pytest

from em_plan_tool import FLAG, build_driver, tuned_env


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_tile_cut"), "em_tile_cut_driver")


def cut(driver, H=8, flags=(), counts=0, n_cu=256, err_blocks=64, rules=(), **tuning):
    args = [driver, H, sum(FLAG[f] for f in flags), counts, n_cu, err_blocks] + list(rules)
    run = subprocess.run([str(a) for a in args], capture_output=True, text=True, env=tuned_env(tuning), timeout=60)
    assert run.returncode == 0, run.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in run.stdout.split())}


def test_target(driver):
    # 3 x 256 = 768 places, 64 error workgroups ride the launch
    assert cut(driver)["tile_target"] == 704
    assert cut(driver, err_blocks=0)["tile_target"] == 768
    assert cut(driver, err_blocks=2)["tile_target"] == 766
    # two handles side by side share the places; each launch carries its own error workgroups: 768 / 2 - 64
    got = cut(driver, flags=("SIDE_BY_SIDE",))
    assert (got["places"], got["side_by_side"], got["tile_target"]) == (768, 2, 320)
    # weighted rows and 16 haplotypes: two workgroups per CU
    assert cut(driver, counts=1)["tile_target"] == 448
    assert cut(driver, H=16)["tile_target"] == 448
    # a chip with no more places than error workgroups keeps them all: 3 x 8 = 24
    assert cut(driver, n_cu=8)["tile_target"] == 24
    assert cut(driver, n_cu=8, err_blocks=24)["tile_target"] == 24
    assert cut(driver, n_cu=8, err_blocks=23)["tile_target"] == 1
    # the function itself
    got = cut(driver, rules=["target=768,1,64,0"])
    assert got["target"] == 704
    assert cut(driver, rules=["target=768,2,64,0"])["target"] == 320
    assert cut(driver, rules=["target=768,1,64,5"])["target"] == 5
    assert cut(driver, rules=["target=1,2,64,0"])["target"] == 1


def test_target_forced(driver):
    for n in (1, 3, 7, 100000):
        assert cut(driver, TILE_TARGET=n)["tile_target"] == n
    assert cut(driver, TILE_TARGET=0)["tile_target"] == 704          # values below 1 are not taken
    assert cut(driver, TILE_TARGET=-3)["tile_target"] == 704


def test_first_size(driver):
    # the bench sample: 5,503,680 / 704 = 7,817.7 -> 7,818 -> the next multiple of 64
    assert cut(driver, rules=["first=5503680"])["first"] == 7872
    assert cut(driver, rules=["first=5503680"], err_blocks=0)["first"] == 7168       # / 768 = 7,166.25
    assert cut(driver, rules=["first=1000"])["first"] == 2048                        # never below TILE_WORDS
    assert cut(driver, rules=["first=1441792"])["first"] == 2048                     # 704 x 2,048 exactly
    assert cut(driver, rules=["first=1441793"])["first"] == 2112
    assert cut(driver, rules=["first=100000000"])["first"] == 32704                  # the cap
    assert cut(driver, rules=["first=100000000"], counts=1)["first"] == 16320        # weighted rows: their cap
    assert cut(driver, rules=["first=70000"], TILE_TARGET=1)["first"] == 32704
    assert cut(driver, rules=["first=5000"], TILE_TARGET=1)["first"] == 5056
    assert cut(driver, rules=["first=5000"], TILE_TARGET=100000)["first"] == 2048


def test_rescale(driver):
    # 880 tiles where 704 were aimed at: 7,872 x 880 / 704 = 9,840 -> 9,856
    assert cut(driver, rules=["rescale=7872,880"])["rescale"] == 9856
    assert cut(driver, rules=["rescale=7872,704"])["rescale"] == 7872                # met: unchanged
    assert cut(driver, rules=["rescale=7872,1"])["rescale"] == 7872
    assert cut(driver, rules=["rescale=7872,705"])["rescale"] == 7936                # 7,883.2 -> 7,936
    assert cut(driver, rules=["rescale=30016,1408"])["rescale"] == 32704             # 60,032: clamped to the cap
    assert cut(driver, rules=["rescale=32704,2000"])["rescale"] == 32704             # at the cap: nothing larger is left
    assert cut(driver, rules=["rescale=8000,600"], counts=1)["rescale"] == 10752     # / 448 = 10,714.3
    assert cut(driver, rules=["rescale=8000,2000"], counts=1)["rescale"] == 16320
    assert cut(driver, rules=["rescale=2048,14"], TILE_TARGET=8)["rescale"] == 3584  # 2,048 x 14 / 8
    for rule, tuning in ((["rescale=7872,880"], {}), (["rescale=2048,9"], {"TILE_TARGET": 8})):
        assert cut(driver, rules=rule, **tuning)["rescale"] % 64 == 0


def test_pass_bound(driver):
    assert cut(driver)["passes"] == 3


def test_which_cut(driver):
    got = cut(driver)
    assert (got["exact_cut"], got["tile_words_forced"], got["d_max"], got["dseg"]) == (1, 0, 384, 352)
    got = cut(driver, TILE_WORDS=4096)
    assert (got["exact_cut"], got["tile_words_forced"]) == (0, 4096)
    assert cut(driver, TILE_WORDS=4096, TILE_TARGET=3)["exact_cut"] == 0
    assert cut(driver, TILE_WORDS=63)["exact_cut"] == 1                              # below 64: not taken, nothing is forced
    assert cut(driver, TILE_CUT=0)["exact_cut"] == 0
    assert cut(driver, TILE_CUT=0, TILE_TARGET=3)["exact_cut"] == 0
    assert cut(driver, TILE_CUT=1)["exact_cut"] == 1
    for kind in (dict(flags=("DETERMINISTIC",)), dict(counts=1), dict(H=16), dict(H=4), dict(flags=("SIDE_BY_SIDE",)),
                 dict(flags=("MERGE_IDENTICAL_ROWS",))):
        assert cut(driver, **kind)["exact_cut"] == 1
        assert cut(driver, TILE_CUT=0, **kind)["exact_cut"] == 0
    got = cut(driver, flags=("DETERMINISTIC",))
    assert (got["d_max"], got["dseg"]) == (48, 16)


def test_one_round_only(driver):
    """The exact cut is taken when the words fit one round under the cap: 704 x 32,704 = 23,023,616 words (weighted rows:
    448 x 16,320 = 7,311,360).  Larger samples keep the two-grid cut, unless GBRS_TUNING_TILE_TARGET asks for the exact one."""
    assert cut(driver, rules=["take=5503680"])["take"] == 1
    assert cut(driver, rules=["take=1"])["take"] == 1
    assert cut(driver, rules=["take=23023616"])["take"] == 1
    assert cut(driver, rules=["take=23023617"])["take"] == 0
    assert cut(driver, rules=["take=59600000"])["take"] == 0
    assert cut(driver, rules=["take=7311360"], counts=1)["take"] == 1
    assert cut(driver, rules=["take=7311361"], counts=1)["take"] == 0
    assert cut(driver, rules=["take=28500000"], H=16)["take"] == 0                  # 448 x 32,704 = 14,651,392
    assert cut(driver, rules=["take=14651392"], H=16)["take"] == 1
    assert cut(driver, rules=["take=70000"], TILE_TARGET=1)["take"] == 1             # forced target: whatever the size
    assert cut(driver, rules=["take=59600000"], TILE_TARGET=704)["take"] == 1
    assert cut(driver, rules=["take=5503680"], TILE_CUT=0)["take"] == 0
    assert cut(driver, rules=["take=5503680"], TILE_WORDS=7104)["take"] == 0
    assert cut(driver, rules=["take=70000"], TILE_TARGET=1, TILE_CUT=0)["take"] == 0
