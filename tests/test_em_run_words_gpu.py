"""The fold of identical one-word reads (em_layout.h, em_tiles.inc): reads that are one word in the tiles - one locus or
one locus set - and carry the same (entry, mask) keep ONE word whose pos / rem bits hold how many further reads it stands
for, up to 1,023 at 8 haplotypes; the kernels read those bits as a count in every batch below TileHdr::n_one.  The cases
sit where that can go wrong: a count at and past the cap, counted batches that the general loop takes, set words, many
tiles, the prepare pass, a second template instance, the float error of a folded row without abundance, and the rule that
keeps a small sample on one word per read.

Every case forces the fold (GBRS_TUNING_RUN_WORDS=1) and compares theta after 1, 2 and 5 iterations and the expected
counts against the numpy oracle on the expanded rows (1e-9), against the same handle built with GBRS_EM_NO_RUN_WORDS
(1e-9, the cross-layout tolerance) and against the same build under GBRS_TUNING_NO_PHASE_SPLIT=1 (1e-12: the same
arithmetic, only the LDS-atomic order differs).

Geometry (tests/test_em_phase_split_gpu.py): 8 wavefronts per tile, rings of 4 batches, wavefront w owns batches
[nb*w/8, nb*(w+1)/8); K one-word rows take the tile's first ceil(K/64) batches, lane g holding rows g*B .. g*B+B-1; two-word
rows follow 32 to a batch, three-word rows 21, five-word rows 12.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9            # against the numpy oracle, and between two layouts of one sample
RTOL_SPLIT = 1e-12     # two loops against one in the same build
ITERS = (1, 2, 5)
NO_LOCUS_SETS = 512    # GBRS_EM_NO_LOCUS_SETS
NO_RUN_WORDS = 8192    # GBRS_EM_NO_RUN_WORDS
ONE_TILE = 16000       # words: every single-tile case below fits
CAP = 1024             # reads a word can stand for at <= 8 haplotypes: 1 << (2 * pos_bits)


def one_word_classes(k, loci, H=8):
    """k distinct (locus, mask) pairs, spread evenly over the loci [a, b)."""
    a, b = loci
    full = (1 << H) - 1
    assert k <= (b - a) * full
    return [[(a + i % (b - a), 1 + (i // (b - a)) * 37 % full)] for i in range(k)]      # 37 is coprime to 255, 15 and 3


def multi_word_rows(n2=0, n3=0, n5=0, loci=(32, 64), seed=1, H=8):
    """Rows on 2 / 3 / 5 distinct loci with a different mask at each (no locus set can replace them by one word), a few
    locus lists per length so that a case stays in the tile it was laid out for."""
    rng = np.random.default_rng(seed)
    a, b = loci
    rows = []
    for n, k in ((n2, 2), (n3, 3), (n5, 5)):
        pool = [sorted(rng.choice(np.arange(a, b), size=k, replace=False).tolist()) for _ in range(8)]
        for _ in range(n):
            lst = pool[int(rng.integers(0, len(pool)))]
            masks = rng.choice(np.arange(1, 1 << H), size=k, replace=False).tolist()
            rows.append(list(zip(lst, masks)))
    return rows


def expand(classes, mult, extra=(), seed=2):
    """Every class repeated mult[i] times, the extra rows once, shuffled: the layout sorts them itself."""
    rows = [list(c) for c, m in zip(classes, mult) for _ in range(m)] + [list(r) for r in extra]
    order = np.random.default_rng(seed).permutation(len(rows))
    return [rows[i] for i in order]


def to_csc(rows, L, H):
    indptr, indices = [], []
    for h in range(H):
        ent = sorted((l, r) for r, row in enumerate(rows) for l, m in row if (m >> h) & 1)
        col = np.array([e[0] for e in ent], dtype=np.int64)
        indices.append(np.array([e[1] for e in ent], dtype=np.uint32))
        indptr.append(np.searchsorted(col, np.arange(L + 1)).astype(np.uint32))
    return indptr, indices


_ORACLE = {}


def oracle_states(key, rows, L, H, eff=None):
    """theta of the prepare pass, after 1, 2 and 5 oracle iterations and the expected counts of the fifth: once per data set."""
    if key not in _ORACLE:
        from oracle.em_oracle import EMOracle
        indptr, indices = to_csc(rows, L, H)
        o = EMOracle(len(rows), L, H, indptr, indices, None)
        o.prepare(0.0, eff)
        old = np.seterr(all="raise", under="ignore")
        try:
            out = {0: o.theta.copy()}
            for it in range(1, max(ITERS) + 1):
                o.em_step()
                if it in ITERS:
                    out[it] = o.theta.copy()
            out["counts"] = o.expected_read_counts().copy()
        finally:
            np.seterr(**old)
        for v in out.values():
            v.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def make_engine(rows, L, H, monkeypatch, tile_words=ONE_TILE, sets=False, flags=0, env=(), eff=None, fold="1"):
    from gbrs_amd.engine import EmEngine
    monkeypatch.setenv("GBRS_TUNING_TILE_WORDS", str(tile_words))
    monkeypatch.setenv("GBRS_TUNING_LOCUS_SETS", "1" if sets else "0")
    for k in ("GBRS_TUNING_NO_PHASE_SPLIT", "GBRS_TUNING_PERSISTENT", "GBRS_TUNING_PERSISTENT_GROUPS", "GBRS_TUNING_RUN_WORDS"):
        monkeypatch.delenv(k, raising=False)
    if fold is not None:
        monkeypatch.setenv("GBRS_TUNING_RUN_WORDS", fold)
    for k, v in env:
        monkeypatch.setenv(k, v)
    indptr, indices = to_csc(rows, L, H)
    return EmEngine.from_host(len(rows), L, H, indptr, indices, None, eff, flags=flags | (0 if sets else NO_LOCUS_SETS))


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


def check_case(key, rows, L, monkeypatch, H=8, tile_words=ONE_TILE, sets=False, env=(), eff=None, partial=False,
               batches=None, words=None, tiles=None, min_tiles=None, one_loop=True):
    """The folded handle against the oracle, against one word per read and against one batch loop.  Returns the folded
    and the unfolded handle's info."""
    ref = oracle_states(key, rows, L, H, eff)
    eng = make_engine(rows, L, H, monkeypatch, tile_words, sets, env=env, eff=eff)
    inf = eng.info()
    assert inf.num_device_rows == len(rows)
    if words is not None:
        assert inf.num_folded_rows == len(rows) - words
    if batches is not None:
        assert inf.num_device_words == 64 * batches
    if tiles is not None:
        assert inf.num_tiles == tiles
    if min_tiles is not None:
        assert inf.num_tiles >= min_tiles
    got = step_states(eng, partial)
    eng.close()
    plain = make_engine(rows, L, H, monkeypatch, tile_words, sets, flags=NO_RUN_WORDS, env=env, eff=eff)
    pinf = plain.info()
    assert pinf.num_folded_rows == 0 and pinf.num_device_rows == len(rows)
    unfolded = step_states(plain, partial)
    plain.close()
    keys = [0] + list(ITERS) + ["counts"]
    for k in keys:
        close(got[k], ref[k], RTOL)
        close(unfolded[k], ref[k], RTOL)
        close(got[k], unfolded[k], RTOL)
    if one_loop:
        eng1 = make_engine(rows, L, H, monkeypatch, tile_words, sets, env=tuple(env) + (("GBRS_TUNING_NO_PHASE_SPLIT", "1"),), eff=eff)
        assert eng1.info().num_device_words == inf.num_device_words
        one = step_states(eng1, partial)
        eng1.close()
        for k in keys:
            close(one[k], ref[k], RTOL)
            close(got[k], one[k], RTOL_SPLIT)
    return inf, pinf


def test_counts_at_the_cap(monkeypatch):
    """One tile, 8 loci.  Runs of 1, 2, 1,024, 1,025 and 2,500 identical reads keep 1, 1, 1, 2 and 3 words (a run is cut every
    1,024 rows); four single reads keep the other loci in the sample.  12 words: one batch."""
    classes = [[(0, 0x35)], [(1, 0x0F)], [(1, 0xF0)], [(2, 0xFF)], [(3, 0x81)], [(4, 0x01)], [(5, 0x7E)], [(6, 0x18)], [(7, 0xC3)]]
    mult = [1, 2, CAP, CAP + 1, 2500, 1, 1, 1, 1]
    rows = expand(classes, mult)
    words = sum(-(-m // CAP) for m in mult)
    assert words == 1 + 1 + 1 + 2 + 3 + 4
    check_case("cap", rows, 8, monkeypatch, tiles=1, batches=1, words=words)


@pytest.mark.parametrize("k,n2", [(2305, 736), (130, 57 * 32)], ids=["n_one_37", "n_one_3"])
def test_boundary_inside_a_wavefronts_share(k, n2, monkeypatch):
    """80 batches, 10 per wavefront.  2,305 classes: n_one = 37, strictly inside wavefront 3's [30, 40) - one ring in the
    first loop, three counted batches and the first multi-word ones in the general loop.  130 classes: n_one = 3, no whole
    ring of wavefront 0 in the first loop - every counted batch goes through the general loop."""
    classes = one_word_classes(k, (0, 32))
    mult = [1 + i % 5 for i in range(k)]
    rows = expand(classes, mult, extra=multi_word_rows(n2=n2, n3=210, n5=120))
    n_one = -(-k // 64)
    check_case(("boundary", k), rows, 64, monkeypatch, tiles=1, batches=n_one + n2 // 32 + 10 + 10, words=k + n2 + 210 + 120)


def test_all_multiplicities_one(monkeypatch):
    """Nothing to fold with the fold forced: the words and batches of the handle that never folds."""
    classes = one_word_classes(2305, (0, 32))
    rows = expand(classes, [1] * len(classes), extra=multi_word_rows(n2=736, n3=210, n5=120))
    inf, pinf = check_case("all_one", rows, 64, monkeypatch, tiles=1, batches=80, words=len(rows))
    assert inf.num_folded_rows == 0
    assert (inf.num_device_words, inf.num_tiles, inf.num_slots) == (pinf.num_device_words, pinf.num_tiles, pinf.num_slots)


def test_locus_sets_fold_too(monkeypatch):
    """600 two-locus reads on one mask, drawn from 40 (set, mask) classes: with the sets on each is one word on a set entry,
    and those words fold like any other - both member loci receive the counted sums.  The other rows are all distinct."""
    rng = np.random.default_rng(3)
    set_classes = [[(32 + 2 * p, m), (33 + 2 * p, m)] for p in range(8) for m in (0x11, 0x2E, 0x47, 0x9C, 0xF3)]
    mult = np.bincount(rng.integers(0, 40, size=600 - 40), minlength=40) + 1      # every class at least once, 600 in all
    assert mult.sum() == 600 and len(set_classes) == 40
    singles = one_word_classes(1750, (0, 32))
    rows = expand(set_classes + singles, mult.tolist() + [1] * len(singles), extra=multi_word_rows(n2=640, n3=210, n5=120, seed=3))
    eng = make_engine(rows, 64, 8, monkeypatch, sets=True)
    assert eng.info().num_locus_sets > 0
    eng.close()
    check_case("sets", rows, 64, monkeypatch, sets=True, tiles=1, words=len(rows) - (600 - 40))


MANY_K = 9000


def many_rows():
    classes = one_word_classes(MANY_K, (0, 64))
    return expand(classes, [1 + i % 5 for i in range(MANY_K)], extra=multi_word_rows(n2=2400, n3=800, n5=400, loci=(64, 128), seed=5))


@pytest.mark.parametrize("mode", ["step", "partial", "persistent"])
def test_many_tiles(mode, monkeypatch):
    """2,560-word tiles over 9,000 folded classes and 3,600 multi-word rows on other loci: tiles of counted batches only, tiles
    without any, and the ones in between - through gbrs_em_step, through estep_partial + finish_step (the stand-alone gather),
    and on two persistent workgroups, whose one loop reads a batch below the header's n_one in count form too."""
    rows = many_rows()
    env = (("GBRS_TUNING_PERSISTENT", "1"), ("GBRS_TUNING_PERSISTENT_GROUPS", "2")) if mode == "persistent" else ()
    check_case("many", rows, 128, monkeypatch, tile_words=2560, env=env, partial=mode == "partial", min_tiles=7,
               words=MANY_K + 3600, one_loop=mode != "persistent")     # (the persistent kernel has one loop as it is)


def test_prepare_spreads_one_unit_per_read(monkeypatch):
    """The prepare pass runs the same tiles with theta = 1: a folded word spreads 1 + count units of mass.  theta_0 against
    the oracle (inside check_case), and sum(theta_0 * length) = R with an effective-length table."""
    classes = one_word_classes(700, (0, 32))
    rows = expand(classes, [1 + (i * 7) % 40 for i in range(700)], extra=multi_word_rows(n2=320, n3=105, n5=60))
    eff = 50.0 + 10.0 * np.random.default_rng(11).integers(0, 200, size=(8, 64)).astype(np.float64)
    check_case("prepare", rows, 64, monkeypatch, eff=eff, tiles=1, words=700 + 485)
    eng = make_engine(rows, 64, 8, monkeypatch, eff=eff)
    eng.prepare(0.0)
    theta0 = eng.theta()
    eng.close()
    assert abs((theta0 * eff).sum() - len(rows)) <= 1e-9 * len(rows)


def test_four_haplotypes(monkeypatch):
    """A second template instance (no theta registers, no 0/1 tables): 300 classes over 15 masks, runs up to 9."""
    classes = one_word_classes(300, (0, 20), H=4)
    rows = expand(classes, [1 + i % 9 for i in range(300)], extra=multi_word_rows(n2=320, n3=105, n5=60, loci=(20, 40), H=4))
    check_case("h4", rows, 40, monkeypatch, H=4, tiles=1, batches=5 + 10 + 5 + 5, words=300 + 485)


# A read whose alignments all have zero abundance, three times: theta of its locus set to zero by hand, the three reads
# folded into one word with count 2.  80 batches, n_one = 40, wavefront 0 owns [0, 10): rings 0-3 and 4-7 in the first
# loop, batches 8 and 9 - counted - in the general one.  Lane 0 holds sorted rows 0 .. 39 at batches 0 .. 39, and the
# one-word rows sort by locus first:
#   first_loop    the read's locus is 0 and carries nothing else: row 0, batch 0
#   general_loop  loci 0-7 carry one class each, the read's locus is 8: row 8, batch 8
def _bad_case(where, with_row):
    zero = 0 if where == "first_loop" else 8
    first = zero + 1
    head = [[(l, 0x5A)] for l in range(zero)]
    classes = head + one_word_classes(2500 - len(head), (first, 32))
    bad = [(zero, 0x35)]
    # the same locus kept alive by a read that also aligns elsewhere: theta there is zero, the row's abundance is not
    extra = multi_word_rows(n2=640, n3=210, n5=120, seed=7) + ([bad] * 3 if with_row else [[(zero, 0x35), (40, 0x53)]] * 3)
    rows = expand(classes, [1] * len(classes), extra=extra)
    return rows, zero


@pytest.mark.parametrize("where", ["first_loop", "general_loop"])
def test_folded_row_without_abundance_raises_from_either_loop(where, monkeypatch):
    for with_row in (True, False):
        rows, zero = _bad_case(where, with_row)
        eng = make_engine(rows, 64, 8, monkeypatch)
        inf = eng.info()
        assert inf.num_tiles == 1 and inf.num_folded_rows == (2 if with_row else 0)
        if with_row:
            assert inf.num_device_words == 64 * 80
        eng.prepare(0.0)
        theta = eng.theta()
        theta[:, zero] = 0.0
        eng.set_theta(theta)
        den = [sum(theta[h, l] for l, m in row for h in range(8) if (m >> h) & 1) for row in rows]
        assert sum(d == 0.0 for d in den) == (3 if with_row else 0)
        if with_row:
            with pytest.raises(FloatingPointError):
                eng.step(1)
        else:
            eng.step(1)
            assert np.isfinite(eng.theta()).all()
        eng.close()


def test_small_sample_keeps_one_word_per_read(monkeypatch):
    """The size rule: 20,000 reads do not give every workgroup place of the device a tile - default flags, no switch, no fold."""
    from gbrs_amd import synth
    from gbrs_amd.engine import EmEngine
    for k in ("GBRS_TUNING_RUN_WORDS", "GBRS_TUNING_TILE_WORDS", "GBRS_TUNING_LOCUS_SETS"):
        monkeypatch.delenv(k, raising=False)
    inc = synth.make_em_problem(R=20_000, H=8, L=400, seed=3)
    eng = EmEngine.from_host(inc.num_rows, inc.num_loci, inc.num_haps, inc.indptr, inc.indices, None, None)
    inf = eng.info()
    eng.close()
    assert inf.num_folded_rows == 0 and inf.num_device_rows == inf.num_rows
