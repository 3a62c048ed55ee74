"""The fold of identical two-word reads (em_layout.h, em_tiles.inc): reads of exactly two (locus, mask) pairs that agree
pair for pair keep ONE row whose two words both carry, in their pos / rem bits, how many further reads the row stands for
(up to 1,023 at <= 8 haplotypes).  A tile's run of two-word rows follows its one-word batches on (even, odd) lane pairs
(TileHdr::n_two), so the lane's parity stands for a word's position; the kernels read those batches as den = s + s of the
partner lane and v = (1 + count) / den - in the first batch loop under a wave-uniform scalar (batch >= n_one), in the
general loop and the persistent kernel under count_form = 2.

Every case forces both folds (GBRS_TUNING_RUN_WORDS=2) and compares theta after the prepare pass and after 1, 2 and 5
iterations, and the expected counts, against the numpy oracle on the expanded rows (1e-9), against the same rows under
GBRS_EM_NO_RUN_WORDS (1e-9, the cross-layout tolerance) and against the same build under GBRS_TUNING_NO_PHASE_SPLIT=1
(1e-12: the same arithmetic, only the LDS-atomic order differs).

Geometry (tests/test_em_phase_split_gpu.py): 8 wavefronts per tile, rings of 4 batches, wavefront w owns batches
[nb*w/8, nb*(w+1)/8) and its first loop takes the whole rings of its share that lie below n_one + n_two; K one-word rows take
the tile's first ceil(K/64) batches; N two-word rows the next B = ceil(N/32), row k at batch k % B on lane pair k / B;
three-word rows follow 21 to a batch, five-word rows 12.

The row generators, the fold counts computed from the input and the oracle states have been run on the CPU; the file as a whole
has not yet run on a device.
"""
import numpy as np
import pytest

from conftest import em_case_inputs, em_case_values, golden_files, load_golden

pytestmark = pytest.mark.gpu

RTOL = 1e-9            # against the numpy oracle, and between two layouts of one sample
RTOL_SPLIT = 1e-12     # the first loop against one loop in the same build
ITERS = (1, 2, 5)
NO_LOCUS_SETS = 512    # GBRS_EM_NO_LOCUS_SETS
NO_RUN_WORDS = 8192    # GBRS_EM_NO_RUN_WORDS
ONE_TILE = 16000       # words: every single-tile case below fits
CAP = 1024             # reads a row can stand for at <= 8 haplotypes: 1 << (2 * pos_bits)


def one_word_classes(k, loci, H=8):
    """k distinct (locus, mask) pairs, spread evenly over the loci [a, b)."""
    a, b = loci
    full = (1 << H) - 1
    assert k <= (b - a) * full
    return [[(a + i % (b - a), 1 + (i // (b - a)) * 37 % full)] for i in range(k)]      # 37 is coprime to 255, 15 and 3


def two_word_classes(k, loci, H=8):
    """k distinct rows of two (locus, mask) pairs on the locus pairs (a, a+1), (a+2, a+3), ... of [a, b), the two masks
    different (no locus set can replace the row by one word)."""
    a, b = loci
    q = (b - a) // 2
    full = (1 << H) - 1
    assert k <= q * full and full >= 2
    out = []
    for i in range(k):
        m1 = 1 + (i // q) % full
        out.append([(a + 2 * (i % q), m1), (a + 2 * (i % q) + 1, m1 % full + 1)])
    return out


def multi_word_rows(n3=0, n5=0, loci=(32, 64), seed=1, H=8):
    """Rows on 3 / 5 distinct loci, a few locus lists per length so that a case stays in the tile it was laid out for."""
    rng = np.random.default_rng(seed)
    a, b = loci
    rows = []
    for n, k in ((n3, 3), (n5, 5)):
        pool = [sorted(rng.choice(np.arange(a, b), size=k, replace=False).tolist()) for _ in range(8)]
        for _ in range(n):
            lst = pool[int(rng.integers(0, len(pool)))]
            masks = rng.integers(1, 1 << H, size=k).tolist()
            if len(set(masks)) == 1:
                masks[0] = masks[0] % ((1 << H) - 1) + 1
            rows.append(list(zip(lst, masks)))
    return rows


def expand(classes, mult, extra=(), seed=2):
    """Every class repeated mult[i] times, the extra rows once, shuffled: the layout sorts them itself."""
    rows = [list(c) for c, m in zip(classes, mult) for _ in range(m)] + [list(r) for r in extra]
    order = np.random.default_rng(seed).permutation(len(rows))
    return [rows[i] for i in order]


def fold_counts_of(rows):
    """(one-word reads, two-word reads) that lose their words: per class of identical rows, size - ceil(size / CAP)."""
    sizes = {}
    for r in rows:
        if len(r) <= 2:
            sizes[tuple(r)] = sizes.get(tuple(r), 0) + 1
    lost = [0, 0, 0]
    for key, n in sizes.items():
        lost[len(key)] += n - -(-n // CAP)
    return lost[1], lost[2]


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


def make_engine(rows, L, H, monkeypatch, tile_words=ONE_TILE, sets=False, flags=0, env=(), eff=None, fold="2"):
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
               batches=None, folded=None, tiles=None, min_tiles=None, one_loop=True):
    """The folded handle against the oracle, against one word per read and against one batch loop.  `folded`: the expected
    (one-word, two-word) fold counts; fold_counts_of(rows) when not given.  Returns the folded handle's info."""
    ref = oracle_states(key, rows, L, H, eff)
    eng = make_engine(rows, L, H, monkeypatch, tile_words, sets, env=env, eff=eff)
    inf = eng.info()
    assert inf.num_device_rows == len(rows)
    want = fold_counts_of(rows) if folded is None else folded
    assert eng.fold_counts() == want
    assert inf.num_folded_rows == want[0]
    if batches is not None:
        assert inf.num_device_words == 64 * batches
    if tiles is not None:
        assert inf.num_tiles == tiles
    if min_tiles is not None:
        assert inf.num_tiles >= min_tiles
    got = step_states(eng, partial)
    eng.close()
    plain = make_engine(rows, L, H, monkeypatch, tile_words, sets, flags=NO_RUN_WORDS, env=env, eff=eff)
    assert plain.fold_counts() == (0, 0) and plain.info().num_device_rows == len(rows)
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
    return inf


def test_counts_at_the_cap(monkeypatch):
    """One tile.  Two-word classes repeated 1, 2, 1,024, 1,025 and 2,500 times keep 1, 1, 1, 2 and 3 rows (a run is cut every
    1,024 rows); four single one-word reads beside them.  4 one-word words and 8 two-word rows: two batches."""
    classes = two_word_classes(5, (0, 10)) + [[(10, 0x01)], [(11, 0x7E)], [(12, 0x18)], [(13, 0xC3)]]
    mult = [1, 2, CAP, CAP + 1, 2500, 1, 1, 1, 1]
    rows = expand(classes, mult)
    kept = [-(-m // CAP) for m in mult[:5]]
    assert kept == [1, 1, 1, 2, 3]
    two = sum(mult[:5]) - sum(kept)
    assert fold_counts_of(rows) == (0, two)
    check_case("cap", rows, 14, monkeypatch, tiles=1, batches=2, folded=(0, two))


@pytest.mark.parametrize("k,n2,n3,n5", [(800, 440, 630, 276), (0, 440, 756, 360), (866, 90, 630, 396)],
                         ids=["n_one_13_n_two_14", "n_one_0", "n_two_3_general_loop"])
def test_boundaries_inside_a_wavefronts_share(k, n2, n3, n5, monkeypatch):
    """80 batches, 10 per wavefront.
    n_one = 13, n_two = 14: wavefront 1 [10, 20) takes 10-12 as one-word and 13-17 as pair batches in its first loop and
    18, 19 - counted pairs - in the general loop; wavefront 2 [20, 30) takes 20-23 in the first loop, 24-26 counted and
    27-29 multi-word in the general one.
    n_one = 0: the two-word run opens the tile; wavefront 0 runs two pair rings, wavefront 1 one, 14-19 in the general loop.
    n_one = 14, n_two = 3: wavefront 1's first loop ends at batch 14 - every counted pair batch (14, 15, 16) goes through
    the general loop."""
    ones = one_word_classes(k, (0, 32))
    twos = two_word_classes(n2, (32, 48))
    mult = [1 + i % 5 for i in range(k)] + [1 + (i * 3) % 7 for i in range(n2)]
    rows = expand(ones + twos, mult, extra=multi_word_rows(n3=n3, n5=n5, loci=(48, 64)))
    n_one, n_two = -(-k // 64), -(-n2 // 32)
    assert n_one + n_two + n3 // 21 + n5 // 12 == 80 and n3 % 21 == 0 and n5 % 12 == 0
    check_case(("boundary", k, n2), rows, 64, monkeypatch, tiles=1, batches=80)


def test_padding_pairs(monkeypatch):
    """33 distinct two-word rows, B = 2: lane pairs 0-15 hold two rows, pair 16 holds row 32 at the first batch and ends early
    (its cells of the second batch carry the dictionary index above them, no haplotype bit, count 0), pairs 17-31 are
    empty from the top.  Every third row stands for several reads.  100 one-word rows and 42 three-word rows around them."""
    ones = one_word_classes(100, (0, 16))
    twos = two_word_classes(33, (16, 32))
    mult = [1 + i % 3 for i in range(100)] + [1 + (5 + i if i % 3 == 0 else 0) for i in range(33)]
    rows = expand(ones + twos, mult, extra=multi_word_rows(n3=42, loci=(32, 48)))
    check_case("padding", rows, 48, monkeypatch, tiles=1, batches=2 + 2 + 2)


MANY_K, MANY_N2 = 6000, 4000


def many_rows():
    ones = one_word_classes(MANY_K, (0, 64))
    twos = two_word_classes(MANY_N2, (64, 128))
    mult = [1 + i % 5 for i in range(MANY_K)] + [1 + i % 4 for i in range(MANY_N2)]
    return expand(ones + twos, mult, extra=multi_word_rows(n3=800, n5=400, loci=(128, 160), seed=5))


@pytest.mark.parametrize("mode", ["step", "partial", "persistent"])
def test_many_tiles(mode, monkeypatch):
    """2,560-word tiles: tiles of one-word batches only, of pair batches only, of both, and of neither - through gbrs_em_step,
    through estep_partial + finish_step, and on two persistent workgroups, whose one loop reads the counted pair batches
    under count_form = 2."""
    rows = many_rows()
    env = (("GBRS_TUNING_PERSISTENT", "1"), ("GBRS_TUNING_PERSISTENT_GROUPS", "2")) if mode == "persistent" else ()
    check_case("many", rows, 160, monkeypatch, tile_words=2560, env=env, partial=mode == "partial", min_tiles=7,
               one_loop=mode != "persistent")     # (the persistent kernel has one loop as it is)


def test_prepare_spreads_one_unit_per_read(monkeypatch):
    """The prepare pass runs the same tiles with theta = 1: a folded two-word row spreads 1 + count units of mass over its
    two loci.  theta_0 against the oracle (inside check_case); the expected counts sum to R, and so does
    sum(theta_0 * length) with an effective-length table."""
    ones = one_word_classes(300, (0, 32))
    twos = two_word_classes(500, (32, 48))
    mult = [1 + i % 4 for i in range(300)] + [1 + (i * 7) % 40 for i in range(500)]
    rows = expand(ones + twos, mult, extra=multi_word_rows(n3=105, n5=60, loci=(48, 64)))
    eff = 50.0 + 10.0 * np.random.default_rng(11).integers(0, 200, size=(8, 64)).astype(np.float64)
    check_case("prepare", rows, 64, monkeypatch, eff=eff, tiles=1)
    eng = make_engine(rows, 64, 8, monkeypatch, eff=eff)
    eng.prepare(0.0)
    theta0 = eng.theta()
    eng.step(1)
    counts = eng.expected_counts()
    eng.close()
    assert abs((theta0 * eff).sum() - len(rows)) <= 1e-9 * len(rows)
    assert abs(counts.sum() - len(rows)) <= 1e-9 * len(rows)


@pytest.mark.parametrize("H,n5", [(4, 60), (2, 0)], ids=["h4", "h2"])
def test_fewer_haplotypes(H, n5, monkeypatch):
    """Template instances without theta registers and 0/1 tables: their first loop keeps the padding test and the
    zero-denominator vote and takes the pair form of the row sum the same way."""
    full = (1 << H) - 1
    ones = one_word_classes(20 * full, (0, 20), H=H)
    twos = two_word_classes(8 * full, (20, 36), H=H)
    mult = [1 + i % 9 for i in range(len(ones))] + [1 + i % 6 for i in range(len(twos))]
    rows = expand(ones + twos, mult, extra=multi_word_rows(n3=105, n5=n5, loci=(36, 52), H=H))
    check_case(("haps", H), rows, 52, monkeypatch, H=H, tiles=1)


def test_locus_sets_on(monkeypatch):
    """Two-locus reads on ONE mask are one word on a set entry when the set is kept, and fold as one-word reads; two-locus
    reads whose masks differ stay two-word rows and fold as such.  Both member loci receive the counted sums."""
    rng = np.random.default_rng(3)
    set_classes = [[(32 + 2 * p, m), (33 + 2 * p, m)] for p in range(8) for m in (0x11, 0x2E, 0x47, 0x9C, 0xF3)]
    set_mult = (np.bincount(rng.integers(0, 40, size=600 - 40), minlength=40) + 1).tolist()
    twos = two_word_classes(300, (32, 48))
    two_mult = [1 + i % 5 for i in range(300)]
    singles = one_word_classes(1000, (0, 32))
    rows = expand(set_classes + twos + singles, set_mult + two_mult + [1] * len(singles),
                  extra=multi_word_rows(n3=210, n5=120, loci=(48, 64), seed=3))
    eng = make_engine(rows, 64, 8, monkeypatch, sets=True)
    assert eng.info().num_locus_sets > 0
    eng.close()
    check_case("sets", rows, 64, monkeypatch, sets=True, tiles=1, folded=(600 - 40, sum(two_mult) - 300))


# A two-word read whose two loci both have zero abundance, three times: folded into one row with count 2.  Its first locus
# is 0, below every other two-word row's, so it is row 0 of the two-word run: batch n_one, lane pair 0.  80 batches,
# wavefront 1 owns [10, 20):
#   first_loop    n_one = 13, n_two = 14: batch 13 is a pair batch of wavefront 1's first loop (whole rings up to 18); the
#                 tile epilogue finds the >= 4.49e307 in the sums
#   general_loop  n_one = 14, n_two = 3: wavefront 1's first loop ends at batch 14, the general loop's vote flags it
def _bad_case(where):
    k, n2, n3, n5 = (800, 440 - 1, 630, 276) if where == "first_loop" else (866, 90 - 1, 630, 396)
    ones = one_word_classes(k, (2, 32))
    twos = two_word_classes(n2, (32, 48))
    bad = [(0, 0x35), (1, 0x53)]
    rows = expand(ones + twos, [1] * (k + n2), extra=multi_word_rows(n3=n3, n5=n5, loci=(48, 64), seed=7) + [bad] * 3)
    return rows


@pytest.mark.parametrize("where", ["first_loop", "general_loop"])
def test_folded_row_without_abundance_raises_from_either_loop(where, monkeypatch):
    rows = _bad_case(where)
    for zeroed in ((0, 1), (0,)):
        eng = make_engine(rows, 64, 8, monkeypatch)
        inf = eng.info()
        assert inf.num_tiles == 1 and eng.fold_counts() == (0, 2) and inf.num_device_words == 64 * 80
        eng.prepare(0.0)
        theta = eng.theta()
        theta[:, list(zeroed)] = 0.0
        eng.set_theta(theta)
        den = [sum(theta[h, l] for l, m in row for h in range(8) if (m >> h) & 1) for row in rows]
        assert sum(d == 0.0 for d in den) == (3 if len(zeroed) == 2 else 0)
        if len(zeroed) == 2:
            with pytest.raises(FloatingPointError):
                eng.step(1)
        else:
            eng.step(1)
            assert np.isfinite(eng.theta()).all()
        eng.close()


@pytest.mark.parametrize("path", golden_files("em"), ids=lambda p: p.split("/")[-1][:-4])
def test_goldens_with_both_folds_forced(path, monkeypatch):
    """The reference's em_* fixtures with both folds forced: theta, the iteration count and the err sequence of a full run."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.em import EMfactory
    for k in ("GBRS_TUNING_NO_PHASE_SPLIT", "GBRS_TUNING_PERSISTENT", "GBRS_TUNING_TILE_WORDS", "GBRS_TUNING_LOCUS_SETS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GBRS_TUNING_RUN_WORDS", "2")
    g = load_golden(path)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)], values=em_case_values(g))
    apm.groups = groups
    apm.gname = np.array([f"G{i:07d}" for i in range(len(groups))])
    apm.num_groups = len(groups)
    if gtmask is not None:
        apm.set_haplotype_mask(((gtmask != 0).astype(np.uint32) << np.arange(H, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32))
    em = EMfactory(apm)
    em.target_lengths = eff_len
    pc = float(g["pseudocount"])
    em.prepare(pseudocount=pc)
    close(em.allelic_expression, g["theta0"], RTOL)
    em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    np.testing.assert_allclose(em.err_history, g["err_history"], rtol=1e-7)
    close(em.allelic_expression, g["theta_final"], RTOL)
    close(em.expected_read_counts(), g["expected_counts"], RTOL)
    em.close()
