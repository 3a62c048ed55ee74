"""The exact tile cut (em_layout.hip stage 7, em_plan.h): a tile ends at tile_words words or at d_max DISTINCT dictionary ids,
whichever comes first, and the tile size is rescaled until about the aimed-at number of tiles comes out.

The rule, as the expected tile counts below are derived from it (never from a run):
  * first size  tw = ceil(W / target) rounded up to a multiple of 64, in [2,048, cap] (cap 32,704; weighted rows 16,320);
  * candidates: a new one at every row whose first word lies in another cell of tw words than the row before it - with
    rows of at most 32 words and cells of at least 2,048 that is ceil(W / tw) candidates;
  * a candidate whose distinct ids are <= d_max is one tile.  Any other is split at every row where the running count of
    FRESH ids (ids of a row that the row before it, in the layout's order, does not have) passes a multiple of dseg;
  * T > target: the next pass takes tw' = ceil(tw T / target), rounded and clamped the same way; 3 passes at most, the
    pass with the fewest tiles stands.
  * the rule takes this cut for the samples whose words fit one round under the cap, GBRS_TUNING_TILE_TARGET - set by every
    case here - whatever the size (em_take_exact_cut; tests/test_em_tile_cut_cpu.py);
  * GBRS_TUNING_TILE_WORDS or GBRS_TUNING_TILE_CUT=0: the two-grid cut (a tile starts where the word offset passes a
    multiple of the tile size, or the entries counted per locus LIST pass a multiple of dseg), unchanged.
At 8 haplotypes d_max = 384 and dseg = 352; deterministic 48 and 16.  The rows of the layout are ordered by their first
locus, then by a hash of their locus list: the cases whose counts are asserted do not depend on the hash.

Every case compares theta after the prepare pass and after 1, 2 and 5 iterations, and the expected counts, against the numpy
oracle and against the same rows under GBRS_TUNING_TILE_CUT=0, each at rtol 1e-9.  Folds and locus sets are off unless a case
says otherwise.

The 27 cases take about three seconds together on an MI355X.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ITERS = (1, 2, 5)
DETERMINISTIC, SIDE_BY_SIDE = 32, 128
NO_LOCUS_SETS, NO_RUN_WORDS = 512, 8192
TILE_WORDS, CAP = 2048, 32704
TUNING = ("TILE_WORDS", "TILE_CUT", "TILE_TARGET", "LOCUS_SETS", "GROUP_SETS", "RUN_WORDS", "NO_PHASE_SPLIT", "PERSISTENT",
          "PERSISTENT_GROUPS", "DICT_CAP", "TILE_ORDER")


def first_size(words, target, cap=CAP):
    """The first pass's tile size (em_cut_tile_words)."""
    return min(max(-(-(-(-words // target)) // 64) * 64, TILE_WORDS), cap)


def mask(i, H=8):
    return 1 + i * 37 % ((1 << H) - 1)         # 37 is coprime to 255, 15 and 65,535


_CSC, _ORACLE = {}, {}


def to_csc(key, rows, L, H):
    if key not in _CSC:
        loc = np.array([l for row in rows for l, m in row], dtype=np.int64)
        msk = np.array([m for row in rows for l, m in row], dtype=np.int64)
        rid = np.repeat(np.arange(len(rows)), [len(row) for row in rows])
        indptr, indices = [], []
        for h in range(H):
            sel = np.flatnonzero((msk >> h) & 1)
            order = sel[np.lexsort((rid[sel], loc[sel]))]
            indices.append(rid[order].astype(np.uint32))
            indptr.append(np.searchsorted(loc[order], np.arange(L + 1)).astype(np.uint32))
        _CSC[key] = (indptr, indices)
    return _CSC[key]


def oracle_states(key, rows, L, H, count=None):
    """theta of the prepare pass, after 1, 2 and 5 oracle iterations and the expected counts of the fifth: once per data set."""
    if key not in _ORACLE:
        from oracle.em_oracle import EMOracle
        indptr, indices = to_csc(key, rows, L, H)
        o = EMOracle(len(rows), L, H, indptr, indices, count)
        o.prepare(0.0, None)
        out = {0: o.theta.copy()}
        for it in range(1, max(ITERS) + 1):
            o.em_step()
            if it in ITERS:
                out[it] = o.theta.copy()
        out["counts"] = o.expected_read_counts().copy()
        for v in out.values():
            v.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def make_engine(key, rows, L, H, monkeypatch, target=None, cut=True, tile_words=None, flags=0, sets=False, fold=False,
                count=None):
    from gbrs_amd.engine import EmEngine
    for k in TUNING:
        monkeypatch.delenv("GBRS_TUNING_" + k, raising=False)
    if target is not None:
        monkeypatch.setenv("GBRS_TUNING_TILE_TARGET", str(target))
    if not cut:
        monkeypatch.setenv("GBRS_TUNING_TILE_CUT", "0")
    if tile_words is not None:
        monkeypatch.setenv("GBRS_TUNING_TILE_WORDS", str(tile_words))
    if sets:
        monkeypatch.setenv("GBRS_TUNING_LOCUS_SETS", "1")
    if fold:
        monkeypatch.setenv("GBRS_TUNING_RUN_WORDS", "2")
    indptr, indices = to_csc(key, rows, L, H)
    return EmEngine.from_host(len(rows), L, H, indptr, indices, count, None,
                              flags=flags | (0 if sets else NO_LOCUS_SETS) | (0 if fold else NO_RUN_WORDS))


def step_states(eng):
    eng.prepare(0.0)
    out = {0: eng.theta()}
    for it in range(1, max(ITERS) + 1):
        eng.step(1)
        if it in ITERS:
            out[it] = eng.theta()
    out["counts"] = eng.expected_counts()
    return out


def close(a, b, rtol=RTOL):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def check_case(key, rows, L, monkeypatch, H=8, target=1, **kw):
    """The exact cut against the oracle and against the two-grid cut of the same rows.  Returns (tiles, passes, tile words,
    largest dictionary) of the exact cut and the tiles of the two-grid cut."""
    ref = oracle_states(key, rows, L, H, kw.get("count"))
    eng = make_engine(key, rows, L, H, monkeypatch, target=target, **kw)
    inf = eng.info()
    assert inf.layout == 1 and inf.num_long_rows == 0
    passes, words = eng.tile_cut()
    largest = int(eng.tile_shapes()[1].max())
    got = step_states(eng)
    eng.close()
    old = make_engine(key, rows, L, H, monkeypatch, target=target, cut=False, **kw)
    old_tiles = int(old.info().num_tiles)
    assert old.tile_cut()[0] == 0
    two_grid = step_states(old)
    old.close()
    print(f"{key}: tiles {int(inf.num_tiles)} (two-grid cut {old_tiles}), passes {passes}, tile words {words}, largest dictionary {largest}")
    assert 1 <= passes <= 3
    for k in [0] + list(ITERS) + ["counts"]:
        close(got[k], ref[k])
        close(two_grid[k], ref[k])
        close(got[k], two_grid[k])
    return int(inf.num_tiles), passes, words, largest, old_tiles


def test_overcounted_lists(monkeypatch):
    """300 loci, two single-locus reads on each and two two-word reads on every adjacent pair: 1,796 words, one candidate of
    2,048, 300 distinct ids <= 384: ONE tile.  The two-grid cut counts every list's loci again - (l) and (l, l + 1) bring 3
    entries per locus, ~897 against dseg = 352 - and cuts several."""
    rows = []
    for l in range(300):
        rows += [[(l, mask(l))], [(l, mask(l + 7))]]
        if l < 299:
            rows += [[(l, mask(l)), (l + 1, mask(l + 1))], [(l, mask(l + 3)), (l + 1, mask(l + 5))]]
    assert sum(len(r) for r in rows) == 1796
    tiles, passes, words, largest, old_tiles = check_case("cut-overcounted", rows, 300, monkeypatch)
    assert (tiles, passes, words, largest) == (1, 1, 2048, 300)
    assert old_tiles > 1


# distinct loci -> tiles.  Two one-word reads per locus, in locus order: the row of locus k brings the fresh id k + 1, so a
# sample of more than d_max = 384 loci is cut where that count passes 352 - once below 704 loci
BINDING_TILES = {351: 1, 352: 1, 353: 1, 384: 1, 385: 2}
# the two-grid cut of the same rows (tests/em_tiny_cases.py DICTIONARY_TILES, h8)
BINDING_TILES_TWO_GRID = {351: 1, 352: 1, 353: 2, 384: 2, 385: 2}


@pytest.mark.parametrize("D", list(BINDING_TILES))
def test_dictionary_binds(D, monkeypatch):
    rows = [[(l, mask(l + j))] for l in range(D) for j in (0, 11)]
    tiles, passes, words, largest, old_tiles = check_case(f"cut-binds-{D}", rows, D, monkeypatch)
    assert tiles == BINDING_TILES[D] and old_tiles == BINDING_TILES_TWO_GRID[D]
    assert passes == (1 if D <= 384 else 3) and largest == (D if D <= 384 else 351)
    # (385 loci: 2 tiles for a target of 1, so the size is doubled twice - 2,048 already holds the sample, a larger size
    # changes nothing - and the first pass stands)
    assert words == 2048


# (one-word loci before the row, one-word loci behind it) -> tiles.  A row of 32 words (max_row_words at 8 haplotypes) on 32
# loci of its own sits behind `before` one-word loci (two reads each): its fresh ids take the count from `before` to
# `before` + 32, across 352 or across d_max = 384.  Up to 384 distinct ids in all: one tile.  More: the sample is cut at the
# row that passes 352 - the long row - and nowhere else.
STRADDLE_TILES = {(340, 12): 1, (340, 13): 2, (351, 1): 1, (351, 2): 2, (360, 0): 2, (383, 0): 2, (320, 32): 1, (321, 32): 2}


@pytest.mark.parametrize("before,behind", list(STRADDLE_TILES))
def test_dictionary_binds_across_a_long_row(before, behind, monkeypatch):
    L = before + 32 + behind
    rows = [[(l, mask(l + j))] for l in range(before) for j in (0, 11)]
    rows.append([(before + j, mask(j)) for j in range(32)])
    rows += [[(l, mask(l + j))] for l in range(before + 32, L) for j in (0, 11)]
    tiles, passes, words, largest, old_tiles = check_case(f"cut-straddle-{before}-{behind}", rows, L, monkeypatch)
    assert tiles == STRADDLE_TILES[(before, behind)]
    # more than 384: the tiles are the rows before the cut and those from it on; the cut is the long row, or the one-word
    # row of locus 351 when the one-word loci alone pass 352
    assert largest == (L if L <= 384 else max(before, 32 + behind) if before < 352 else 351)
    assert largest <= 384 and tiles <= old_tiles


def test_word_cap_binds(monkeypatch):
    """One locus, 70,000 one-word reads: a target of one tile asks for 70,016 words, the cap gives 32,704: three candidates,
    each with a dictionary of one."""
    rows = [[(0, mask(i))] for i in range(70000)]
    tiles, passes, words, largest, _ = check_case("cut-cap", rows, 1, monkeypatch)
    assert first_size(70000, 1) == CAP
    assert (tiles, words, largest) == (3, CAP, 1) and tiles >= 3
    assert passes == 1          # at the cap no larger size is left: one pass


def sample_5000():
    rng = np.random.default_rng(41)
    rows = []
    for _ in range(5000):
        loci = np.sort(rng.choice(40, size=int(rng.integers(1, 4)), replace=False))
        masks = rng.integers(1, 256, size=len(loci)).tolist()
        rows.append([(int(l), int(m)) for l, m in zip(loci, masks)])
    return rows


def test_target_extremes(monkeypatch):
    """5,000 reads over 40 loci (the dictionary never binds): the tiles are the cells of the first size, never below 2,048
    words however many tiles are asked for.  Targets 1, 3, 7 and one above the number of rows agree with one another."""
    rows = sample_5000()
    W = sum(len(r) for r in rows)
    assert 3 * TILE_WORDS < W < 7 * TILE_WORDS
    states = {}
    for target in (1, 3, 7, 1_000_000):
        tw = first_size(W, target)
        assert tw >= TILE_WORDS and (target > 3 or tw > TILE_WORDS)
        eng = make_engine("cut-5000", rows, 40, 8, monkeypatch, target=target)
        tiles = int(eng.info().num_tiles)
        batches, entries = eng.tile_shapes()
        print(f"target {target}: tiles {tiles}, cut {eng.tile_cut()}, batches {batches.tolist()}")
        assert eng.tile_cut() == (1, tw)
        assert tiles == -(-W // tw) <= max(target, -(-W // TILE_WORDS))
        # no tile below the minimum but the last cell: a tile of 2,048 words is at least 32 batches
        assert np.sum(batches < TILE_WORDS // 64) <= 1 and entries.max() <= 40
        states[target] = step_states(eng)
        eng.close()
    ref = oracle_states("cut-5000", rows, 40, 8)
    for target, got in states.items():
        for k in [0] + list(ITERS) + ["counts"]:
            close(got[k], ref[k])
            close(got[k], states[1][k])


def test_rescale_path(monkeypatch):
    """2,000 loci with one read each, then 4 loci with 20,000 reads each, all one word; target 8.  W = 82,000.
    Pass 1: tw = 10,304, 8 candidates; the first holds the 2,000 sparse loci (2,001 ids > 384) and is split where the fresh
    ids pass 352, 704, 1,056, 1,408 and 1,760: 13 tiles.  Pass 2: tw = ceil(10,304 x 13 / 8) = 16,744 -> 16,768, 5 candidates
    + 5 = 10 tiles.  Pass 3: 16,768 x 10 / 8 = 20,960 -> 20,992, 4 candidates + 5 = 9 tiles, and the passes end.
    The rule's bound: target + floor(fresh ids / dseg) = 8 + floor(2,004 / 352) = 13 tiles, 3 passes."""
    rows = [[(l, mask(l))] for l in range(2000)]
    rows += [[(l, mask(i))] for l in range(2000, 2004) for i in range(20000)]
    assert first_size(82000, 8) == 10304
    tiles, passes, words, largest, _ = check_case("cut-rescale", rows, 2004, monkeypatch, target=8)
    assert passes <= 3 and tiles <= 8 + 2004 // 352
    assert (tiles, passes, words) == (9, 3, 20992)
    assert largest == 352          # fresh ids 352 .. 703 of the sparse part (the first tile holds 351)


def flavour_rows(H, duplicates=False, same_mask_pairs=False):
    """About 2,000 reads over 700 loci: a single-locus read on every locus, a two-word read on every adjacent pair and 600
    more single-locus reads: 2,698 words."""
    rows = []
    for l in range(700):
        rows.append([(l, mask(l, H))])
        if l < 699:
            rows.append([(l, mask(l, H)), (l + 1, mask(l, H) if same_mask_pairs else mask(l + 1, H))])
    rows += [[(l, mask(l if duplicates else l + 5, H))] for l in range(0, 600)]
    assert len(rows) == 1999 and sum(len(r) for r in rows) == 2698
    return rows


@pytest.mark.parametrize("name,H,kw", [
    ("weighted", 8, dict(count=True)), ("h16", 16, {}), ("h4", 4, {}), ("folds", 8, dict(fold=True)),
    ("locus_sets", 8, dict(sets=True)), ("side_by_side", 8, dict(flags=SIDE_BY_SIDE))])
def test_flavours(name, H, kw, monkeypatch):
    rows = flavour_rows(H, duplicates=name == "folds", same_mask_pairs=name == "locus_sets")
    kw = dict(kw)
    if kw.get("count"):
        kw["count"] = np.random.default_rng(5).integers(1, 6, size=len(rows)).astype(np.float64)
    tiles, passes, words, largest, old_tiles = check_case(f"cut-flavour-{name}", rows, 700, monkeypatch, H=H, target=4, **kw)
    # 2,698 words for 4 tiles: the first pass takes the minimum size, two candidates; the dictionary splits them further
    # where it binds (the list entries the two-grid cut counts are at least the fresh ids of the same rows)
    d_max = {"weighted": 576, "h16": 300, "h4": 768}.get(name, 384)
    assert words >= TILE_WORDS and 1 <= tiles <= old_tiles and largest <= d_max
    if name == "folds":
        a = make_engine("cut-flavour-folds", rows, 700, H, monkeypatch, target=4, fold=True)
        b = make_engine("cut-flavour-folds", rows, 700, H, monkeypatch, target=4, fold=True, cut=False)
        assert a.fold_counts() == b.fold_counts() == (600, 0)
        a.close()
        b.close()
    if name == "locus_sets":
        a = make_engine("cut-flavour-locus_sets", rows, 700, H, monkeypatch, target=4, sets=True)
        assert a.info().num_locus_sets == 699
        a.close()


def test_deterministic(monkeypatch):
    """Capacity 48, dseg 16: every candidate is dictionary-bound, and the fresh ids - at most 2 per locus here, where the
    two-grid cut counts 3 - cut fewer tiles.  Two handles of the same build are bit-identical."""
    rows = flavour_rows(8)
    tiles, passes, words, largest, old_tiles = check_case("cut-flavour-det", rows, 700, monkeypatch, target=4, flags=DETERMINISTIC)
    assert largest <= 48 and tiles < old_tiles
    # the two-grid cut: 700 + 2 x 699 = 2,098 entries in lists / 16; the exact cut: at most 1,400 fresh ids / 16, 2 candidates
    assert old_tiles >= 2098 // 16 - 1 and tiles <= 1400 // 16 + 2
    out = []
    for _ in range(2):
        eng = make_engine("cut-flavour-det", rows, 700, 8, monkeypatch, target=4, flags=DETERMINISTIC)
        out.append(step_states(eng))
        eng.close()
    for k in [0] + list(ITERS) + ["counts"]:
        np.testing.assert_array_equal(out[0][k], out[1][k])


@pytest.mark.parametrize("tile_words", [64, 512, 4096])
def test_forced_size_keeps_the_two_grid_cut(tile_words, monkeypatch):
    """GBRS_TUNING_TILE_WORDS: the same tiles with and without GBRS_TUNING_TILE_CUT=0, whatever the target says.  At 512
    words both grids cut the 700-locus sample (2,698 words; 2,098 list entries against dseg = 352); the 5,000-read sample
    over 40 loci is cut by its words alone."""
    for key, rows, L in (("cut-flavour-plain", flavour_rows(8), 700), ("cut-5000", sample_5000(), 40)):
        seen = []
        for cut in (True, False):
            eng = make_engine(key, rows, L, 8, monkeypatch, target=3, cut=cut, tile_words=tile_words)
            assert eng.tile_cut() == (0, tile_words)
            seen.append((int(eng.info().num_tiles), eng.tile_shapes()[0].tolist(), eng.tile_shapes()[1].tolist()))
            eng.close()
        assert seen[0] == seen[1]
        W = sum(len(r) for r in rows)
        assert seen[0][0] >= -(-W // (tile_words + 31))
        if L == 700 and tile_words == 512:
            assert seen[0][0] > -(-W // 512)          # more tiles than the word grid alone cuts: the dictionary grid cut too
