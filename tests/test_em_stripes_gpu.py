"""Stripes in a tile's counted runs (em_plan.h, em_layout.hip: tile_pad_kernel, fill_one_word_cells_kernel): the rows of one
group - one dictionary id in the run of one-word rows, one (first id, second id) pair in the run of two-word rows - start
only at a cell that is a multiple of the stripe S, a group of n rows takes ceil(n / S) * S cells, the run's batches B are
rounded up to a multiple of S, and cell c sits on lane (or lane pair) c / B at batch c % B.  The empty cells of a group's
last stripe carry the dictionary index of the word above them, no haplotype bit and a count of 0.  The E-step kernels are
the ones that read the layout without stripes.

Every case forces the stripe (GBRS_TUNING_STRIPES in {2, 4, 8}) and both folds (GBRS_TUNING_RUN_WORDS=2) and compares theta
after the prepare pass and after 1, 2 and 5 iterations, and the expected counts, against the numpy oracle on the expanded
rows (1e-9) and against the same build under GBRS_TUNING_STRIPES=0 (1e-12: the same arithmetic per word, the order of the
LDS atomics differs).  Without the variable every case here is far below the size em_take_stripes asks for and has the words of
GBRS_TUNING_STRIPES=0.

The geometry is computed from the input: K kept one-word rows in groups of n_g take B1 = ceil(sum(ceil(n_g / S) * S) / 64)
batches, rounded up to a multiple of S; two-word rows the same with 32 lane pairs; three-word rows follow 21 to a batch,
five-word rows 12.  A class of m identical reads keeps ceil(m / 1024) rows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9            # against the numpy oracle
RTOL_S0 = 1e-12        # against the same build without stripes
ITERS = (1, 2, 5)
KEYS = [0] + list(ITERS) + ["counts"]
DETERMINISTIC, NO_STREAMS, NO_LOCUS_SETS = 32, 16, 512
ONE_TILE = 16000       # words: every single-tile case below fits
CAP = 1024             # reads a row can stand for at <= 8 haplotypes
STRIPES = (2, 4, 8)
TUNING = ("GBRS_TUNING_NO_PHASE_SPLIT", "GBRS_TUNING_PERSISTENT", "GBRS_TUNING_PERSISTENT_GROUPS", "GBRS_TUNING_RUN_WORDS",
          "GBRS_TUNING_STRIPES", "GBRS_TUNING_NO_GATHER_MSTEP", "GBRS_TUNING_TILE_WORDS", "GBRS_TUNING_LOCUS_SETS",
          "GBRS_TUNING_TILE_TARGET", "GBRS_TUNING_TILE_CUT")


# ---- rows ------------------------------------------------------------------------------------------------------------------

def one_word_groups(sizes, first=0, H=8):
    """Locus first + g gets sizes[g] distinct masks: sizes[g] classes of one (locus, mask) pair."""
    full = (1 << H) - 1
    assert max(sizes) <= full
    return [[(first + g, 1 + (g + 37 * i) % full)] for g, n in enumerate(sizes) for i in range(n)]


def pair_groups(sizes, first=0, H=8):
    """Locus pair (first + 2g, first + 2g + 1) gets sizes[g] distinct mask pairs, the two masks of a pair different where the
    haplotypes allow it."""
    full = (1 << H) - 1
    assert max(sizes) <= full
    return [[(first + 2 * g, 1 + i % full), (first + 2 * g + 1, 1 + (i + 1 + g % max(full - 1, 1)) % full)]
            for g, n in enumerate(sizes) for i in range(n)]


def multi_word_rows(n3=0, n5=0, loci=(32, 64), seed=1, H=8):
    """Rows on 3 / 5 distinct loci, a few locus lists per length."""
    rng = np.random.default_rng(seed)
    a, b = loci
    rows = []
    for n, k in ((n3, 3), (n5, 5)):
        pool = [sorted(rng.choice(np.arange(a, b), size=k, replace=False).tolist()) for _ in range(8)]
        for _ in range(n):
            lst = pool[int(rng.integers(0, len(pool)))]
            masks = rng.integers(1, 1 << H, size=k).tolist()
            if len(set(masks)) == 1 and H > 1:
                masks[0] = masks[0] % ((1 << H) - 1) + 1
            rows.append(list(zip(lst, masks)))
    return rows


def expand(classes, mult, extra=(), seed=2):
    """Every class repeated mult[i] times, the extra rows once, shuffled: the layout sorts them itself."""
    rows = [list(c) for c, m in zip(classes, mult) for _ in range(m)] + [list(r) for r in extra]
    order = np.random.default_rng(seed).permutation(len(rows))
    return [rows[i] for i in order]


def to_csc(rows, L, H):
    r = np.repeat(np.arange(len(rows)), [len(row) for row in rows])
    loc = np.array([l for row in rows for l, _ in row], dtype=np.int64)
    mask = np.array([m for row in rows for _, m in row], dtype=np.int64)
    indptr, indices = [], []
    for h in range(H):
        sel = np.flatnonzero((mask >> h) & 1)
        sel = sel[np.lexsort((r[sel], loc[sel]))]
        indices.append(r[sel].astype(np.uint32))
        indptr.append(np.searchsorted(loc[sel], np.arange(L + 1)).astype(np.uint32))
    return indptr, indices


def geometry(rows, S):
    """(batches of the one-word run, of the two-word run, of the tile, padding cells of the two counted runs) of ONE tile
    that holds `rows`, at stripe S (0: none)."""
    sizes = {}
    for r in rows:
        sizes[tuple(r)] = sizes.get(tuple(r), 0) + 1
    groups = ({}, {})
    longer = {}
    for key, n in sizes.items():
        if len(key) <= 2:
            g = tuple(l for l, _ in key)
            groups[len(key) - 1][g] = groups[len(key) - 1].get(g, 0) + -(-n // CAP)     # the rows the fold keeps
        else:
            longer[len(key)] = longer.get(len(key), 0) + n
    batches, padding = [], 0
    for g, lanes in zip(groups, (64, 32)):
        n = sum(g.values())
        if S:
            B = -(-sum(-(-k // S) * S for k in g.values()) // lanes)
            B = -(-B // S) * S
        else:
            B = -(-n // lanes)
        batches.append(B)
        padding += (B * lanes - n) * (64 // lanes)
    off = 0
    for k in sorted(longer):                  # rows that do not divide 64 pack in order and never straddle a batch
        for _ in range(longer[k]):
            if off % 64 + k > 64:
                off = -(-off // 64) * 64
            off += k
    return batches[0], batches[1], batches[0] + batches[1] + -(-off // 64), padding


# ---- engines and states ----------------------------------------------------------------------------------------------------

_ORACLE = {}


def oracle_states(key, rows, L, H):
    """theta of the prepare pass, after 1, 2 and 5 oracle iterations and the expected counts of the fifth: once per data set."""
    if key not in _ORACLE:
        from oracle.em_oracle import EMOracle
        indptr, indices = to_csc(rows, L, H)
        o = EMOracle(len(rows), L, H, indptr, indices, None)
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


def make_engine(rows, L, H, monkeypatch, stripes, tile_words=ONE_TILE, env=(), flags=NO_LOCUS_SETS, count=None, fold="2"):
    """stripes: the value of GBRS_TUNING_STRIPES, None: the variable is not set."""
    from gbrs_amd.engine import EmEngine
    for k in TUNING:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GBRS_TUNING_TILE_WORDS", str(tile_words))
    monkeypatch.setenv("GBRS_TUNING_LOCUS_SETS", "0")
    if fold is not None:
        monkeypatch.setenv("GBRS_TUNING_RUN_WORDS", fold)
    if stripes is not None:
        monkeypatch.setenv("GBRS_TUNING_STRIPES", str(stripes))
    for k, v in env:
        monkeypatch.setenv(k, v)
    indptr, indices = to_csc(rows, L, H)
    return EmEngine.from_host(len(rows), L, H, indptr, indices, count, None, flags=flags)


def step_states(eng, partial=False):
    eng.prepare(0.0)
    out = {0: eng.theta()}
    for it in range(1, max(ITERS) + 1):
        if partial:
            eng.estep_partial()
            eng.finish_step(want_err=False)
        else:
            eng.step(1)
        if it in ITERS:
            out[it] = eng.theta()
    out["counts"] = eng.expected_counts()
    return out


def close(a, b, rtol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


_PLAIN = {}


def plain_states(key, rows, L, H, monkeypatch, tile_words, env, partial):
    """The same build under GBRS_TUNING_STRIPES=0: (states, words, census), once per data set and way of running it."""
    if key not in _PLAIN:
        eng = make_engine(rows, L, H, monkeypatch, 0, tile_words, env)
        _PLAIN[key] = (step_states(eng, partial), int(eng.info().num_device_words), eng.stripe_census(0))
        eng.close()
    return _PLAIN[key]


def check_case(key, rows, L, S, monkeypatch, H=8, tile_words=ONE_TILE, env=(), partial=False, one_tile=True):
    """The striped handle against the oracle and against GBRS_TUNING_STRIPES=0; its words and its census against the formula
    (one tile) or against the invariants (several).  Returns (info, census) of the striped handle."""
    ref = oracle_states(key, rows, L, H)
    eng = make_engine(rows, L, H, monkeypatch, S, tile_words, env)
    inf, census = eng.info(), eng.stripe_census(S)
    got = step_states(eng, partial)
    eng.close()
    plain, plain_words, plain_census = plain_states((key, tile_words, tuple(env), partial), rows, L, H, monkeypatch, tile_words, env, partial)
    unset = make_engine(rows, L, H, monkeypatch, None, tile_words, env)
    assert unset.info().num_device_words == plain_words          # the size rule declines a sample this small
    unset.close()
    assert census[5] == 0
    if one_tile:
        assert inf.num_tiles == 1
        b1, b2, nb, padding = geometry(rows, S)
        assert inf.num_device_words == 64 * nb
        assert census[0] == b1 + b2 and census[4] == padding
        p1, p2, pnb, ppadding = geometry(rows, 0)
        assert plain_words == 64 * pnb and plain_census[0] == p1 + p2 and plain_census[4] == ppadding
    else:
        assert inf.num_tiles > 1 and inf.num_device_words >= plain_words and census[4] >= plain_census[4]
    for k in KEYS:
        close(got[k], ref[k], RTOL)
        close(plain[k], ref[k], RTOL)
        close(got[k], plain[k], RTOL_S0)
    return inf, census


# ---- one-word groups, pair groups ----------------------------------------------------------------------------------------

def one_word_case():
    """64 ids of 1 ... 12 distinct masks in turn: groups one short of, on and one past a stripe of 2, 4 and 8.  The ids of one
    mask stand for 1,024 reads: a count field at its cap above the group's padding cells.  63 three-word rows behind them."""
    sizes = [1 + g % 12 for g in range(64)]
    classes = one_word_groups(sizes)
    mult, i = [], 0
    for n in sizes:
        mult += [CAP if n == 1 else 1 + (7 * (i + j)) % 13 for j in range(n)]
        i += n
    mult[5] = CAP + 1        # one class kept as two rows
    return expand(classes, mult, extra=multi_word_rows(n3=63, loci=(64, 80))), 80


@pytest.mark.parametrize("S", STRIPES)
def test_one_word_groups(S, monkeypatch):
    rows, L = one_word_case()
    inf, census = check_case("one", rows, L, S, monkeypatch)
    # 401 kept words: 7 batches without stripes; every group padded to whole stripes with them
    assert geometry(rows, 0)[:2] == (7, 0)
    assert geometry(rows, S)[0] == {2: 8, 4: 8, 8: 16}[S]


def pair_case():
    """40 (a, b) locus pairs of 1 ... 7 distinct mask pairs in turn; the pairs of one mask pair stand for 1,024 reads.  A few
    one-word rows in front (n_one = 1) and 42 three-word rows behind."""
    sizes = [1 + g % 7 for g in range(40)]
    classes = pair_groups(sizes)
    mult, i = [], 0
    for n in sizes:
        mult += [CAP if n == 1 else 1 + (5 * (i + j)) % 11 for j in range(n)]
        i += n
    ones = one_word_groups([3, 1, 2], first=80)
    return expand(classes + ones, mult + [2] * len(ones), extra=multi_word_rows(n3=42, loci=(86, 100))), 100


@pytest.mark.parametrize("S", STRIPES)
def test_pair_groups(S, monkeypatch):
    rows, L = pair_case()
    check_case("pairs", rows, L, S, monkeypatch)
    assert geometry(rows, 0)[:2] == (1, 5)
    assert geometry(rows, S)[:2] == {2: (2, 6), 4: (4, 8), 8: (8, 16)}[S]


# ---- lane boundaries -----------------------------------------------------------------------------------------------------

def lane_case(name, S):
    """crossing: 90 groups of S + 1 words, two stripes each, on lanes of B = 3 S cells: every other lane ends between the two
    stripes of a group.  empty: ten groups, the lanes behind them empty from the top.  single: one group is the whole run.
    exact: groups of S words that fill B = S batches exactly - nothing is rounded."""
    if name == "crossing":
        sizes = [S + 1] * 90
    elif name == "empty":
        sizes = [3] * 10
    elif name == "single":
        sizes = [5]
    else:
        sizes = [S] * 64                      # 64 S cells: B = S, every lane one group
    ones = one_word_groups(sizes)
    twos = pair_groups([min(n, 7) for n in sizes[:50]], first=len(sizes))
    L = len(sizes) + 2 * min(len(sizes), 50)
    mult = [1 + i % 3 for i in range(len(ones) + len(twos))]
    return expand(ones + twos, mult, extra=multi_word_rows(n3=21, loci=(L, L + 8))), L + 8


@pytest.mark.parametrize("S", STRIPES)
@pytest.mark.parametrize("name", ["crossing", "empty", "single", "exact"])
def test_lane_boundaries(name, S, monkeypatch):
    rows, L = lane_case(name, S)
    b1 = geometry(rows, S)[0]
    if name == "crossing":
        assert b1 == 3 * S
    if name == "exact":
        assert b1 == S and geometry(rows, 0)[0] == S
    if name == "single":
        assert b1 == S
    check_case(("lane", name, S), rows, L, S, monkeypatch)


# ---- both runs in front of the general loop --------------------------------------------------------------------------

def combined_case():
    """3,000 one-word classes on 100 loci in groups of 9 and 51, 2,000 two-word classes on 50 locus pairs in groups of 7 and
    73, 800 three-word and 400 five-word rows: 264 locus lists, one dictionary.  The classes of the small groups stand for
    several reads; those of the large groups for one each, so that the number of rows the fold keeps does not hang on two
    classes of one group sharing a sort key."""
    one_sizes = [9 + 42 * (g % 2) for g in range(100)]
    two_sizes = [7 + 66 * (g % 2) for g in range(50)]
    ones = one_word_groups(one_sizes)
    twos = pair_groups(two_sizes, first=100)
    mult = [1 + (i % 5 if n == 9 else 0) for n in one_sizes for i in range(n)] + [1 + (i % 4 if n == 7 else 0) for n in two_sizes for i in range(n)]
    return expand(ones + twos, mult, extra=multi_word_rows(n3=800, n5=400, loci=(200, 232), seed=5)), 232


WAYS = {
    "one_tile": dict(),
    "tiles": dict(tile_words=2560, one_tile=False),
    "partial": dict(tile_words=2560, one_tile=False, partial=True),
    "no_gather_mstep": dict(tile_words=2560, one_tile=False, env=(("GBRS_TUNING_NO_GATHER_MSTEP", "1"),)),
    "no_phase_split": dict(env=(("GBRS_TUNING_NO_PHASE_SPLIT", "1"),)),
    "persistent": dict(tile_words=2560, one_tile=False, env=(("GBRS_TUNING_PERSISTENT", "1"), ("GBRS_TUNING_PERSISTENT_GROUPS", "2"))),
}


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("way", list(WAYS))
def test_combined_layout(way, S, monkeypatch):
    rows, L = combined_case()
    check_case("combined", rows, L, S, monkeypatch, **WAYS[way])


# ---- other kernel instances ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 2, 4])
def test_fewer_haplotypes(H, monkeypatch):
    full = (1 << H) - 1
    sizes = [1 + g % full for g in range(30)]
    ones = one_word_groups(sizes, H=H)
    twos = pair_groups(sizes[:20], first=30, H=H)
    mult = [1 + i % 9 for i in range(len(ones) + len(twos))]
    rows = expand(ones + twos, mult, extra=multi_word_rows(n3=42, loci=(70, 86), H=H))
    check_case(("haps", H), rows, 86, 4, monkeypatch, H=H)


def test_all_one_word(monkeypatch):
    """Only one-word rows: the ONEWORD instance reads the striped run."""
    sizes = [1 + g % 12 for g in range(64)]
    classes = one_word_groups(sizes)
    rows = expand(classes, [1 + (3 * i) % 17 for i in range(len(classes))])
    check_case("oneword", rows, 64, 4, monkeypatch)


# ---- the float error -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", STRIPES)
def test_read_without_abundance_raises_and_padding_does_not(S, monkeypatch):
    """Locus 70 carries one read and nothing else; with theta zeroed there its denominator is 0.  The padding cells of the
    stripes divide the same guard value and add nothing."""
    rows, L = one_word_case()
    bad = 70                                   # (no three-word row's list need hold it: it is zeroed for both samples)
    rows = [r for r in rows if all(l != bad for l, _ in r)]
    for sample, raises in ((rows + [[(bad, 0x35)]], True), (rows, False)):
        eng = make_engine(sample, L, 8, monkeypatch, S)
        eng.prepare(0.0)
        theta = eng.theta()
        theta[:, bad] = 0.0
        eng.set_theta(theta)
        assert eng.stripe_census(S)[4] > 0
        if raises:
            with pytest.raises(FloatingPointError):
                eng.step(1)
        else:
            eng.step(1)
            assert np.isfinite(eng.theta()).all()
        eng.close()


# ---- layouts that must not move --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["counts", "deterministic", "h16", "no_streams"])
def test_other_layouts_ignore_the_variable(kind, monkeypatch):
    H = 16 if kind == "h16" else 8
    sizes = [1 + g % 12 for g in range(64)]
    ones = one_word_groups(sizes, H=H)
    twos = pair_groups([1 + g % 7 for g in range(20)], first=64, H=H)
    rows = expand(ones + twos, [1 + i % 4 for i in range(len(ones) + len(twos))], extra=multi_word_rows(n3=42, loci=(104, 120), H=H))
    count = np.arange(1, len(rows) + 1, dtype=np.float64) if kind == "counts" else None
    flags = NO_LOCUS_SETS | {"deterministic": DETERMINISTIC, "no_streams": NO_STREAMS}.get(kind, 0)
    shapes = []
    for stripes in (None, 4):
        eng = make_engine(rows, 120, H, monkeypatch, stripes, flags=flags, count=count, fold=None)
        b, d = eng.tile_shapes()
        shapes.append((int(eng.info().num_device_words), b.tolist(), d.tolist()))
        eng.close()
    assert shapes[0] == shapes[1]


# ---- the padding cap ---------------------------------------------------------------------------------------------------------

def test_ids_of_one_word_each_keep_their_layout():
    """1.6 M reads on as many loci, at a size em_take_stripes accepts on 256 compute units (768 places x 2,048 words): a
    stripe of 2 would double the run, so every tile's rule answers S = 0 and the layout is the one without stripes.  The same
    number of reads on ids of 15 words each pads a fifteenth at S = 4 and takes it."""
    import os
    from gbrs_amd.engine import EmEngine
    saved = {k: os.environ.pop(k) for k in TUNING if k in os.environ}
    try:
        got = {}
        for per_id in (1, 15):
            L = 1_600_005 // per_id
            n = L * per_id
            loc, mask = np.arange(n) // per_id, 1 + np.arange(n) % per_id
            rows_of = [np.flatnonzero((mask >> h) & 1) for h in range(8)]
            indptr = [np.searchsorted(loc[sel], np.arange(L + 1)).astype(np.uint32) for sel in rows_of]
            indices = [sel.astype(np.uint32) for sel in rows_of]
            for stripes in (None, "0"):
                os.environ.pop("GBRS_TUNING_STRIPES", None)
                if stripes is not None:
                    os.environ["GBRS_TUNING_STRIPES"] = stripes
                eng = EmEngine.from_host(n, L, 8, indptr, indices, None, None, flags=NO_LOCUS_SETS)
                got[per_id, stripes] = (int(eng.info().num_device_words), eng.stripe_census(4).tolist())
                eng.close()
        assert got[1, None] == got[1, "0"]
        assert got[15, None][1][5] == 0 and got[15, "0"][1][5] > 0
        assert got[15, "0"][0] < got[15, None][0] <= got[15, "0"][0] * 9 // 8 + 64 * 4 * 1024
    finally:
        os.environ.pop("GBRS_TUNING_STRIPES", None)
        os.environ.update(saved)
