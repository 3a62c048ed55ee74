"""The tiny EM cases (tests/em_tiny_cases.py) without a device: oracle/em_oracle.py - the float64 restatement every EM
test compares the device with - against the 60-digit Model-4 EM of tests/em_exact.py, em_exact's two number types against
each other, the table's limits against em_plan(), and the cases against what they claim to be.

Bounds: theta and the expected counts rtol 1e-9 (RTOL of tests/test_em_gpu.py, what the kernels are held to) with atol
1e-300 - an exact zero stays an exact zero; the err history rtol 1e-7 as everywhere in the suite, plus atol 4e-3: the sum
runs over per-locus values scaled to a total of 1e6; each is within 1e-9 relative on both sides of the difference (2e-3
over values that total 1e6) and so are the two totals they are scaled by (2e-3 more).  The oracle is nowhere near them: the largest relative deviation
of any theta or count from em_exact over all cases is 1.2e-15 (printed by every test; run with -s to see it)."""
from fractions import Fraction

import numpy as np
import pytest

import em_tiny_cases as tc
from em_exact import ExactEM, max_relative_difference
from em_plan_tool import build_driver, plan
from oracle.em_oracle import EMOracle

RTOL, ATOL = 1e-9, 1e-300
ERR_RTOL, ERR_ATOL = 1e-7, 4e-3
CASES = tc.all_cases()
LIVE = [n for n, c in CASES.items() if not c.no_entries]
SMALL = [n for n in LIVE if sum(bin(m).count("1") for _, pairs in CASES[n].rows for _, m in pairs) <= 40]


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


def deviation(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def make_oracle(case):
    csc = tc.csc_of(case)
    o = EMOracle(case.R, case.L, case.H, csc.indptr, csc.indices, case.count)
    if case.allowed is not None:
        o.apply_genotype_mask(tc.gtmask_of(case))
    return o


def check_history(got, want):
    """A run at tol = 0 stops before max_iters exactly when its err_sum is 0.0 (err_sum > 0 is the loop's condition): the
    history may be shorter than the exact one only by ending in such a zero, which the exact value must justify."""
    assert 1 <= len(got) <= len(want)
    np.testing.assert_allclose(got, want[:len(got)], rtol=ERR_RTOL, atol=ERR_ATOL)
    if len(got) < len(want):
        assert got[-1] == 0.0


@pytest.mark.parametrize("name", LIVE)
def test_oracle_matches_exact(name):
    case = CASES[name]
    want = tc.expected_of(case)
    o = make_oracle(case)
    o.prepare(tc.PSEUDOCOUNT, case.eff_len)
    worst = deviation(o.theta, want.theta0_pc)
    close(o.theta, want.theta0_pc)
    o = make_oracle(case)
    o.prepare(0.0, case.eff_len)
    worst = max(worst, deviation(o.theta, want.theta0))
    close(o.theta, want.theta0)
    seen = []
    n = o.run(tol=0.0, max_iters=tc.STEPS, on_iter=lambda k, theta, err: seen.append(theta.copy()))
    for k, theta in enumerate(seen):
        worst = max(worst, deviation(theta, want.theta[k]))
        close(theta, want.theta[k])
    check_history(o.err_history, want.err)
    if n == tc.STEPS:
        worst = max(worst, deviation(o.expected_read_counts(), want.counts))
        close(o.expected_read_counts(), want.counts)
    # (a run that stopped at an exact fixed point holds the counts of that point: the same theta, one E-step earlier)
    print(f"ORACLE_DEVIATION {name} H={case.H} {worst:.3e}")
    assert worst < 1e-12, "ill-conditioned case: replace it"


@pytest.mark.parametrize("name", SMALL)
def test_decimal_matches_fraction(name):
    """The same code path in exact rational arithmetic: 60 digits lose nothing that matters in two iterations."""
    case = CASES[name]
    for pc in (0.0, tc.PSEUDOCOUNT):
        dec, fra = tc.exact_of(case).prepare(pc), tc.exact_of(case, Fraction).prepare(pc)
        assert max_relative_difference(dec.theta, fra.theta) < 1e-50
        dec.run(2)
        fra.run(2)
        assert all(isinstance(v, Fraction) for v in fra.theta.values())
        assert max_relative_difference(dec.theta, fra.theta) < 1e-50
        assert max_relative_difference(dec.expected_counts(), fra.expected_counts()) < 1e-50
        assert max_relative_difference(dec.posterior(), fra.posterior()) < 1e-50
        for a, b in zip(dec.err_history, fra.err_history):
            assert abs(Fraction(a) - b) < Fraction(1, 10 ** 44)        # values on a scale of 1e6


def test_exact_em_by_hand():
    """Two reads, two loci, one haplotype, lengths 1 and 2, counts 3 and 1: worked by hand in rationals."""
    em = ExactEM(2, 2, 1, [(0, [(0, 1), (1, 1)]), (1, [(1, 1)])], count=[3, 1], eff_len=[[1, 2]], number=Fraction)
    em.prepare(0.0)
    assert em.theta == {(0, 0): Fraction(3, 2), (0, 1): Fraction(5, 4)}            # 3/2 ; (3/2 + 1) / 2
    em.run(1)
    # read 0 splits 6/11 : 5/11
    assert em.posterior() == {(0, 0, 0): Fraction(6, 11), (0, 1, 0): Fraction(5, 11), (1, 1, 0): Fraction(1)}
    assert em.expected_counts() == {(0, 0): Fraction(18, 11), (0, 1): Fraction(26, 11)}
    assert em.theta == {(0, 0): Fraction(18, 11), (0, 1): Fraction(13, 11)}
    # totals 3/2, 5/4 of 11/4 against 18/11, 13/11 of 31/11, each scaled to 1e6
    assert em.err_history == [2 * abs(Fraction(18, 31) - Fraction(6, 11)) * 1000000]
    em.prepare(0.5)
    assert em.theta == {(0, 0): Fraction(2) * Fraction(11, 15), (0, 1): Fraction(7, 4) * Fraction(11, 15)}


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.no_entries])
def test_no_entries_on_the_oracle(name):
    """prepare gives zeros, a run divides by the zero total at its first iteration: what the device test demands."""
    case = CASES[name]
    assert tc.exact_of(case).num_entries == 0
    o = make_oracle(case)
    o.prepare(0.0, case.eff_len)
    assert o.theta.shape == (case.H, case.L) and not o.theta.any()
    # (with a pseudocount the reference rescales by 0 / 0 and numpy hands back NaN under a warning; em_exact and the
    # device have nothing to rescale and keep the zeros)
    with pytest.raises(FloatingPointError, match="divide by zero"):
        o.run(tol=0.0, max_iters=tc.STEPS)
    assert o.num_iters == 0
    want = tc.expected_of(case)
    assert not want.theta0.any() and not want.theta0_pc.any()


# ---- the limits the cases were aimed at ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("em_plan_tiny"))


@pytest.mark.parametrize("key", list(tc.PLAN), ids=lambda k: f"h{k[0]}" + ("_weighted" if k[1] else "") + ("_det" if k[2] else ""))
def test_plan_literals(driver, key):
    H, weighted, det = key
    got = plan(driver, H=H, counts=int(weighted), flags=["DETERMINISTIC"] if det else [])
    assert got["tiled"] == 1 and got["dict_room"] == 1 and got["weighted"] == int(weighted)
    want = tc.PLAN[key]
    assert (got["d_max"], got["dseg"], got["d_max"] - got["dseg"], got["per_cu"]) == tuple(want)


def test_haplotype_counts_above_16_have_no_tiles(driver):
    for H in range(17, 33):
        assert plan(driver, H=H)["tiled"] == 0


@pytest.mark.parametrize("name,H,weighted,det", tc.DICTIONARY_FLAVOURS)
def test_dictionary_cases_follow_the_plan(driver, name, H, weighted, det):
    """L = dseg - 1, dseg, dseg + 1, d_max, d_max + 1 of the flavour's plan, under the tile size the cases set; read r's
    locus is dictionary entry r, and a tile ends where the entries before a row pass a multiple of dseg."""
    got = plan(driver, H=H, counts=int(weighted), flags=["DETERMINISTIC"] if det else [], TILE_WORDS=tc.TILE_WORDS_HIGH,
               rule="tile=1025")
    d_max, dseg = got["d_max"], got["dseg"]
    assert (d_max, dseg) == tc.PLAN[(H, weighted, det)][:2]
    assert got["tile"] == tc.TILE_WORDS_HIGH > d_max + 1
    table = tc.DICTIONARY_TILES[name]
    assert list(table) == [dseg - 1, dseg, dseg + 1, d_max, d_max + 1]
    for L, tiles in table.items():
        assert tiles == len({r // dseg for r in range(L)})
        case = CASES[f"dictionary_{name}_L{L}"]
        assert (case.R, case.L, case.H) == (L, L, H) and (case.count is not None) == weighted
        assert case.home_flags == (tc.FLAG_DETERMINISTIC if det else 0) and case.facts["num_tiles"] == tiles
        assert [(r, [l for l, _ in pairs]) for r, pairs in case.rows] == [(l, [l]) for l in range(L)]
    assert table[dseg + 1] == table[dseg] + 1


# ---- the cases are what they say -----------------------------------------------------------------------------------------------

def _row_words(case):
    """row -> loci left after the mask."""
    out = {}
    for r, pairs in case.rows:
        n = sum(1 for l, m in pairs if case.allowed is None or m & int(case.allowed[l]))
        if n:
            out[r] = n
    return out


def test_every_case_is_well_formed():
    assert len(CASES) == len(set(CASES))
    for case in CASES.values():
        assert case.H <= 32 and all(pairs for _, pairs in case.rows)
        csc = tc.csc_of(case)
        assert csc.N == sum(bin(m).count("1") for _, pairs in case.rows for _, m in pairs)
        assert (tc.exact_of(case).num_entries == 0) == case.no_entries
        if "num_entries" in case.facts:
            assert tc.exact_of(case).num_entries == case.facts["num_entries"]


def test_long_rows_are_where_the_cases_say():
    for case in CASES.values():
        if "num_long_rows" not in case.facts:
            continue
        weighted, det = case.count is not None, case.home_flags == tc.FLAG_DETERMINISTIC
        limit = tc.PLAN[(case.H, False, False)].max_row_words        # the limit depends on the haplotype count alone
        if (case.H, weighted, det) in tc.PLAN:
            assert tc.PLAN[(case.H, weighted, det)].max_row_words == limit
        words = _row_words(case)
        assert sum(1 for n in words.values() if n > limit) == case.facts["num_long_rows"], case.name
        if case.facts.get("num_tiles") == 0:
            assert all(n > limit for n in words.values())
    for H in (8, 16, 11):
        limit = tc.PLAN[(H, False, False)].max_row_words
        assert max(_row_words(CASES[f"row_of_{limit}_words_h{H}"]).values()) == limit
        assert max(_row_words(CASES[f"row_of_{limit + 1}_words_h{H}"]).values()) == limit + 1


def test_corner_ids_need_bit_16():
    big = CASES["corners_65537x65537"]
    assert (big.R - 1) >> 16 == 1 and (big.L - 1) >> 16 == 1 and (big.R - 2) >> 16 == 0
    cells = {(r, l) for r, pairs in big.rows for l, _ in pairs}
    assert cells == {(0, 0), (65536, 65536), (65536, 0), (65535, 65535)}
    assert {m for _, pairs in big.rows for _, m in pairs} == {0x01, 0x80, 0x81}
    for L in (31, 32, 33):
        c = CASES[f"corners_L{L}"]
        assert {(r, l) for r, pairs in c.rows for l, _ in pairs} == {(0, 0), (65536, L - 1), (65536, 0), (65535, L - 2)}
    # the l * 32 + h keys of the last locus sit below, at and above a multiple of 1024
    assert [(L - 1) * 32 + 7 for L in (31, 32, 33)] == [967, 999, 1031]


def test_mask_cases():
    c = CASES["mask_empties_some_rows"]
    assert sorted(_row_words(c)) == [0, 3, 5] and len(c.rows) == 5
    assert tc.csc_of(c).N > tc.exact_of(c).num_entries == sum(len(i) for i in tc.masked_csc_of(c)[1]) == 5
    assert tc.csc_of(CASES["mask_removes_everything"]).N == 4


def test_sweep_shape():
    assert tc.SWEEP_H == list(range(1, 33)) and tc.SWEEP_L % 2 == 1
    for H in tc.SWEEP_H:
        assert (tc.SWEEP_L * H) % 256 != 0
        plain, counted = CASES[f"sweep_h{H}"], CASES[f"sweep_h{H}_counts"]
        assert plain.rows == counted.rows and plain.count is None
        assert set(np.unique(counted.count)) == {1.0, 2.0, 3.0, 4.0}
        assert (plain.R, plain.L) == (200, 37) and plain.eff_len.min() >= 1 and plain.eff_len.max() <= 900
        aligned = {r for r, _ in plain.rows}
        assert len(aligned) == 180 and 0 not in aligned and 199 not in aligned
        by_pairs = {}
        for r, pairs in plain.rows:
            by_pairs.setdefault(tuple(pairs), []).append(r)
        full = [(l, (1 << H) - 1) for l in range(37)]
        assert len(by_pairs[tuple(full)]) == 1
        assert any(len(k) == 1 and len(v) >= 19 for k, v in by_pairs.items())
        assert all(1 <= len(pairs) <= 6 for r, pairs in plain.rows if pairs != full)
        if H > 1:
            assert plain.rows != CASES[f"sweep_h{H - 1}"].rows          # seeded per H


def test_batch_and_identical_cases():
    for H in (1, 8):
        for R in (63, 64, 65):
            c = CASES[f"batch_{R}_reads_h{H}_counts"]
            assert c.L == 1 and len(c.rows) == R and len({tuple(p) for _, p in c.rows}) == 1
            assert list(c.count) == list(range(1, R + 1)) and CASES[f"batch_{R}_reads_h{H}"].count is None
    c = CASES["fifty_identical_rows"]
    assert len(c.rows) == 50 and len({tuple(p) for _, p in c.rows}) == 1 and len(c.rows[0][1]) == 3
    for H in (8, 16, 32):
        assert {m for _, pairs in CASES[f"full_masks_h{H}"].rows for _, m in pairs} == {(1 << H) - 1}
