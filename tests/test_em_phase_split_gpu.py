"""The E-step's two batch loops (em_tiles.inc): a tile header records how many of the tile's first batches hold one-word
rows only (TileHdr::n_one), and a wavefront runs the whole word rings of its share that lie in them through a loop without
the row-length vote, the padding test and the zero-denominator vote.  The cases sit where that can go wrong: where the
boundary falls in a wavefront's share, what the empty cells of the one-word batches hold, what the second loop starts
from, and the float error a row without abundance must still raise from either loop.

Geometry (em_layout.h, em_layout.hip): 8 wavefronts per tile, wavefront w owns batches [nb*w/8, nb*(w+1)/8) of the tile's
nb, its word ring holds PD = 4 batches; n one-word rows take the tile's first B = ceil(n/64) batches, lane g holding rows
g*B .. g*B+B-1; two-word rows follow 32 to a batch, three-word rows 21 to a batch, five-word rows 12 to a batch.  A case
states the batch counts it was built for and checks them against the handle (num_device_words), so a layout change
that moves the boundary elsewhere fails here instead of passing on other ground.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 8
RTOL = 1e-9            # against the numpy oracle: the tolerance of test_em_gpu.py
RTOL_SPLIT = 1e-12     # two loops against one in the same build: the same arithmetic, only the LDS-atomic order differs
ITERS = (1, 2, 5)
NO_LOCUS_SETS = 512    # GBRS_EM_NO_LOCUS_SETS


def build_rows(n1=0, n2=0, n3=0, n5=0, n_same=0, loci1=(0, 32), loci_m=(32, 64), L=64, seed=1, extra=()):
    """Reads as lists of (locus, haplotype mask): n1 on one locus of loci1, n2 / n3 / n5 on 2 / 3 / 5 distinct loci of loci_m
    with a different mask at each (so that no locus set can replace them by one word), n_same on two loci of loci_m with one
    mask (a two-member locus set when the sets are on: one word; two words otherwise).  `extra` rows are appended as given.
    The rows are shuffled: the layout sorts them itself."""
    rng = np.random.default_rng(seed)
    rows = []
    a, b = loci1
    for i in range(n1):
        rows.append([(a + (i * (b - a)) // max(n1, 1), int(rng.integers(1, 256)))])
    a, b = loci_m
    for n, k in ((n2, 2), (n3, 3), (n5, 5)):
        # (a tile's dictionary is budgeted by the distinct locus lists of its rows, em_layout.hip tile_flag_kernel: a few
        # lists per row length keep a case in the one tile it was laid out for)
        pool = [sorted(rng.choice(np.arange(a, b), size=k, replace=False).tolist()) for _ in range(8)]
        for _ in range(n):
            loci = pool[int(rng.integers(0, len(pool)))]
            masks = rng.choice(np.arange(1, 256), size=k, replace=False).tolist()
            rows.append(list(zip(loci, masks)))
    for _ in range(n_same):
        l = a + 2 * int(rng.integers(0, 8))    # eight pairs of neighbouring loci: eight sets, the dictionary stays small
        m = int(rng.integers(1, 256))
        rows.append([(l, m), (l + 1, m)])
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order] + [list(r) for r in extra]
    return rows, L


def to_csc(rows, L):
    """indptr / indices per haplotype (column = locus, entries = read ids ascending), as AlignmentPropertyMatrix takes them."""
    indptr, indices = [], []
    for h in range(H):
        ent = sorted((l, r) for r, row in enumerate(rows) for l, m in row if (m >> h) & 1)
        col = np.array([e[0] for e in ent], dtype=np.int64)
        indices.append(np.array([e[1] for e in ent], dtype=np.uint32))
        indptr.append(np.searchsorted(col, np.arange(L + 1)).astype(np.uint32))
    return indptr, indices


_ORACLE = {}


def oracle_states(key, rows, L):
    """theta after 1, 2 and 5 oracle iterations and the expected counts of the fifth, computed once per data set."""
    if key not in _ORACLE:
        from oracle.em_oracle import EMOracle
        indptr, indices = to_csc(rows, L)
        o = EMOracle(len(rows), L, H, indptr, indices, None)
        o.prepare(0.0, None)
        old = np.seterr(all="raise", under="ignore")
        try:
            out = {}
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


def make_em(rows, L, monkeypatch, tile_words, sets=False, env=()):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.em import EMfactory
    indptr, indices = to_csc(rows, L)
    apm = AlignmentPropertyMatrix(shape=(L, H, len(rows)), indptr=indptr, indices=indices,
                                  haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:03d}" for l in range(L)])
    monkeypatch.setenv("GBRS_TUNING_TILE_WORDS", str(tile_words))
    monkeypatch.setenv("GBRS_TUNING_LOCUS_SETS", "1" if sets else "0")
    for k in ("GBRS_TUNING_NO_PHASE_SPLIT", "GBRS_TUNING_PERSISTENT", "GBRS_TUNING_PERSISTENT_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    em = EMfactory(apm, extra_flags=0 if sets else NO_LOCUS_SETS)
    em.prepare(0.0)
    return em


def step_states(em):
    out = {}
    for it in range(1, max(ITERS) + 1):
        em.update_allelic_expression(model=4)
        if it in ITERS:
            out[it] = em.allelic_expression.copy()
    out["counts"] = em.expected_read_counts()
    return out


def close(a, b, rtol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def check_case(key, rows, L, monkeypatch, tile_words, sets=False, env=(), tiles=None, batches=None):
    """Two loops against the oracle (1e-9) and against one loop on a handle built the same way (1e-12)."""
    ref = oracle_states(key, rows, L)
    em = make_em(rows, L, monkeypatch, tile_words, sets, env)
    inf = em.info()
    if tiles is not None:
        assert inf.num_tiles == tiles
    if batches is not None:
        assert inf.num_device_words == 64 * batches
    got = step_states(em)
    em.close()
    em1 = make_em(rows, L, monkeypatch, tile_words, sets, tuple(env) + (("GBRS_TUNING_NO_PHASE_SPLIT", "1"),))
    one = step_states(em1)
    em1.close()
    for k in list(ITERS) + ["counts"]:
        close(got[k], ref[k], RTOL)
        close(one[k], ref[k], RTOL)
        close(got[k], one[k], RTOL_SPLIT)


ONE_TILE = 16000       # words: every single-tile case below fits

# name -> (build_rows arguments, batches of the one tile).  nb = batches; wavefront w owns [nb*w/8, nb*(w+1)/8).
SINGLE = {
    # one-word rows only.  65 rows: two batches, lanes 33-63 empty in both - padding in every batch, no ring inside n_one
    "one_word_65": (dict(n1=65), 2),
    # 64 * 64 rows exactly: no empty cell; 8 batches = two whole rings per wavefront, all through the first loop
    "one_word_64x64": (dict(n1=4096), 64),
    # 2,500 rows: B = 40, 5 per wavefront (one ring through the first loop, one batch through the second); lanes 0-61 are
    # full, lane 62 ends after 20 rows (its cells below carry its last row's entry), lane 63 is empty from the top
    # (all-zero words: entry 0)
    "one_word_padded": (dict(n1=2500), 40),
    # no one-word row at all: n_one = 0
    "no_one_word": (dict(n2=640, n3=210, n5=120), 40),
    # nb = 80, 10 per wavefront, n_one = 3 and 6: smaller than wavefront 0's share; no ring / one ring of it inside n_one
    "n_one_3": (dict(n1=130, n2=57 * 32, n3=210, n5=120), 3 + 57 + 20),
    "n_one_6": (dict(n1=6 * 64 - 10, n2=54 * 32, n3=210, n5=120), 6 + 54 + 20),
    # nb = 80, 10 per wavefront.  n_one = 40: the boundary is the edge between wavefronts 3 and 4 (wavefront 3: two rings
    # in the first loop, batches 38-39 - one-word rows - in the second)
    "edge_between_waves": (dict(n1=2500, n2=640, n3=210, n5=120), 80),
    # n_one = 37, not a multiple of 4: strictly inside wavefront 3's [30, 40) - one ring (30-33) in the first loop,
    # three one-word batches and the first multi-word ones in the second.  2,305 rows: lane 62 ends after 11, lane 63 is empty
    "inside_a_wave": (dict(n1=2305, n2=736, n3=210, n5=120), 37 + 23 + 20),
    # the same boundary with three loci under the one-word rows: a lane's first word of the second loop is on the entry its
    # last word of the first loop was on (above: 32 loci under 2,305 rows, 72 to a locus - every other lane changes entry
    # inside its 37 rows, and one in ten between batches 33 and 34)
    "inside_a_wave_same_entry": (dict(n1=2305, n2=736, n3=210, n5=120, loci1=(0, 3)), 37 + 23 + 20),
}


@pytest.mark.parametrize("name", list(SINGLE))
def test_one_tile_boundaries(name, monkeypatch):
    spec, nb = SINGLE[name]
    rows, L = build_rows(**spec)
    check_case(name, rows, L, monkeypatch, ONE_TILE, tiles=1, batches=nb)


@pytest.mark.parametrize("sets", [False, True], ids=["no_locus_sets", "locus_sets"])
def test_locus_sets_on_and_off(sets, monkeypatch):
    """600 reads on two loci with one mask: two-word rows without the sets (n_one = 28 of 28 + 20 + 19 + 10 + 10), one-word
    rows on a set entry with them (the first loop then runs on dictionary entries that are locus sets)."""
    rows, L = build_rows(n1=1750, n2=640, n3=210, n5=120, n_same=600, seed=3)
    check_case("sets", rows, L, monkeypatch, ONE_TILE, sets=sets, tiles=1,
               batches=None if sets else 28 + 39 + 20)


MANY = dict(n1=9000, n2=2400, n3=800, n5=400, seed=5)


@pytest.mark.parametrize("env", [(), (("GBRS_TUNING_PERSISTENT", "1"), ("GBRS_TUNING_PERSISTENT_GROUPS", "2"))],
                         ids=["tile_per_workgroup", "persistent_two_workgroups"])
def test_many_tiles_headers_of_both_kinds(env, monkeypatch):
    """2,560-word tiles (40 batches, 5 per wavefront) over reads whose one-word rows and multi-word rows live on different
    loci: tiles of one-word rows only, tiles without any, and the ones in between, side by side in one launch - and walked
    in turn by two persistent workgroups, which read the new header but keep one loop."""
    rows, L = build_rows(**MANY)
    ref = oracle_states("many", rows, L)
    em = make_em(rows, L, monkeypatch, 2560, env=env)
    assert em.info().num_tiles >= 7
    got = step_states(em)
    em.close()
    for k in list(ITERS) + ["counts"]:
        close(got[k], ref[k], RTOL)
    if not env:
        em1 = make_em(rows, L, monkeypatch, 2560, env=(("GBRS_TUNING_NO_PHASE_SPLIT", "1"),))
        one = step_states(em1)
        em1.close()
        for k in list(ITERS) + ["counts"]:
            close(got[k], one[k], RTOL_SPLIT)


# A read whose alignments all have zero abundance: theta of its loci set to zero by hand.  Locus 0 carries one one-word
# read - the first row of the tile's one-word run: lane 0, batch 0, inside wavefront 0's first ring; loci 62 and 63 carry
# one two-word read and nothing else - behind the boundary.
BAD_BASE = dict(n1=2500, n2=640, n3=210, n5=120, loci1=(1, 32), loci_m=(32, 62), seed=7)
BAD_ROWS = {"first_loop": [[(0, 0x35)]], "second_loop": [[(62, 0x0F), (63, 0xF0)]]}


@pytest.mark.parametrize("where", list(BAD_ROWS))
def test_row_without_abundance_raises_from_either_loop(where, monkeypatch):
    zero_loci = [0] if where == "first_loop" else [62, 63]
    for with_row in (True, False):
        rows, L = build_rows(**BAD_BASE, extra=BAD_ROWS[where] if with_row else
                             # the same loci kept alive by a read that also aligns elsewhere: theta there is zero, the row is not
                             [[(zero_loci[0], 0x35), (40, 0x53)]])
        em = make_em(rows, L, monkeypatch, ONE_TILE)
        assert em.info().num_tiles == 1
        theta = em.allelic_expression.copy()
        theta[:, zero_loci] = 0.0
        em.allelic_expression = theta
        # the abundance every read is left with: zero for the appended read of the first variant and for no other
        den = [sum(theta[h, l] for l, m in row for h in range(H) if (m >> h) & 1) for row in rows]
        assert all(d > 0.0 for d in den[:-1]) and (den[-1] == 0.0) == with_row
        if with_row:
            with pytest.raises(FloatingPointError):
                em.update_allelic_expression(model=4)
        else:
            em.update_allelic_expression(model=4)
            assert np.isfinite(em.allelic_expression).all()
        em.close()
