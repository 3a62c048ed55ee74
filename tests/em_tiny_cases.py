"""Tiny EM inputs: degenerate and boundary shapes, and one input per haplotype count from 1 to 32.  Plain data and
generators: no GPU and no import of the library.  tests/test_em_tiny_cpu.py holds oracle/em_oracle.py to tests/em_exact.py
on every case, the table's limits to em_plan() and the cases to the preconditions they name; tests/test_em_tiny_gpu.py runs
every case on the device against em_exact.

A case is a `TinyCase`: `rows` is the explicit input, [(row, [(locus, mask), ...]), ...] (rows that are not listed have no
alignments); `allowed` is a `-G` mask (haplotype bits per locus); `env` the GBRS_TUNING_* variables (short names) the case
needs on every create; `facts` what gbrs_em_info must report for a handle created with `home_flags` and no other variable.
Every read that has alignments keeps positive abundance: theta starts positive wherever a read aligns and Model 4 keeps
it so.  The exceptions are the `no_entries` cases, which have no read with alignments at all.
"""
import collections

import numpy as np

from em_exact import ExactEM
from small_ops_cases import csc_from_rows

# What the plan (gbrs_amd/csrc/em_plan.h) resolves for (haplotypes, weighted rows, deterministic): dictionary capacity
# d_max, what is left of it beside one row's loci (dseg: a tile is cut where the running dictionary count passes a multiple
# of it), the longest row the tiles hold (max_row_words; a longer one is a long row) and the resident E-step workgroups
# per CU.  Literals: tests/test_em_tiny_cpu.py holds each row to em_plan(), so a changed limit fails there by row.
Limits = collections.namedtuple("Limits", "d_max dseg max_row_words per_cu")
PLAN = {
    (1, False, False): Limits(1024, 992, 32, 3),
    (2, False, False): Limits(1024, 992, 32, 3),
    (3, False, False): Limits(1024, 992, 32, 3),
    (4, False, False): Limits(768, 736, 32, 3),
    (5, False, False): Limits(614, 582, 32, 3),
    (6, False, False): Limits(512, 480, 32, 3),
    (7, False, False): Limits(438, 406, 32, 3),
    (8, False, False): Limits(384, 352, 32, 3),
    (9, False, False): Limits(341, 333, 8, 2),
    (10, False, False): Limits(307, 299, 8, 2),
    (11, False, False): Limits(279, 271, 8, 2),
    (12, False, False): Limits(256, 248, 8, 2),
    (13, False, False): Limits(236, 228, 8, 2),
    (14, False, False): Limits(219, 211, 8, 2),
    (15, False, False): Limits(204, 196, 8, 2),
    (16, False, False): Limits(300, 292, 8, 2),
    (8, True, False): Limits(576, 544, 32, 2),
    (8, False, True): Limits(48, 16, 32, 3),
}
TILE_WORDS_HIGH = 32704          # GBRS_TUNING_TILE_WORDS of the dictionary cases: their tiles end at their dictionaries
FLAG_DETERMINISTIC = 32

TinyCase = collections.namedtuple("TinyCase", "name R L H rows count eff_len allowed env home_flags facts no_entries")


def _case(name, R, L, H, rows, count=None, eff_len=None, allowed=None, env=None, home_flags=0, facts=None, no_entries=False):
    rows = [(int(r), [(int(l), int(m)) for l, m in pairs]) for r, pairs in rows]
    if count is not None:
        count = np.asarray(count, dtype=np.float64)
    if allowed is not None:
        allowed = np.asarray(allowed, dtype=np.uint32)
    return TinyCase(name, R, L, H, rows, count, eff_len, allowed, dict(env or {}), home_flags, dict(facts or {}), no_entries)


def _ramp(H, L):
    """Small integer effective lengths that differ between the haplotypes and the loci."""
    return 1.0 + (np.arange(H)[:, None] * 5 + np.arange(L)[None, :] * 3) % 11


def _triplet_rows(entries):
    """[(row, locus, hap)] -> the rows form."""
    by_row = collections.OrderedDict()
    for r, l, h in entries:
        by_row.setdefault(r, collections.OrderedDict()).setdefault(l, 0)
        by_row[r][l] |= 1 << h
    return [(r, list(loci.items())) for r, loci in by_row.items()]


# ---- degenerate shapes ---------------------------------------------------------------------------------------------------

def _first_cases():
    """The five inputs the project's first device check of degenerate shapes ran (effective lengths of one)."""
    full8 = [(0, l, h) for l in range(4) for h in range(8)] + [(1, 3, 7)]
    return [
        _case("single_entry", 1, 1, 1, [(0, [(0, 1)])], eff_len=np.ones((1, 1))),
        _case("one_empty_row", 3, 2, 2, _triplet_rows([(0, 0, 0), (0, 1, 1), (2, 1, 0)]), eff_len=np.ones((2, 2))),
        # the only entry is (last row, last locus, last haplotype)
        _case("last_corner_only", 5, 3, 2, [(4, [(2, 2)])], eff_len=np.ones((2, 3))),
        _case("full_masks_and_one_bit", 2, 4, 8, _triplet_rows(full8), eff_len=np.ones((8, 4))),
        _case("seventy_counted_rows", 70, 3, 1, [(r, [(r % 3, 1)]) for r in range(70)], count=np.arange(1, 71),
              eff_len=np.ones((1, 3))),
    ]


BIG = 65537                      # the first size whose last id needs bit 16


def corner_rows(R, L):
    """Entries at (0, 0), (R - 1, L - 1), (R - 1, 0) and (R - 2, L - 2), on haplotype bits 0 and 7."""
    return [(0, [(0, 0x01)]), (R - 1, [(0, 0x81), (L - 1, 0x80)]), (R - 2, [(L - 2, 0x81)])]


def _corner_cases():
    out = [_case("corners_65537x65537", BIG, BIG, 8, corner_rows(BIG, BIG))]
    # l * 32 + h keys: the loci around the 5-bit haplotype field
    for L in (31, 32, 33):
        out.append(_case(f"corners_L{L}", BIG, L, 8, corner_rows(BIG, L), eff_len=_ramp(8, L)))
    return out


def _no_entry_cases():
    some = [(0, [(0, 1), (2, 1)]), (1, [(1, 1)]), (3, [(0, 1)])]
    partly = [(0, [(0, 1), (1, 1)]), (1, [(1, 1)]), (2, [(2, 2)]), (3, [(0, 2), (2, 3)]), (5, [(1, 2), (2, 1)])]
    return [
        _case("empty_columns", 3, 2, 2, [], eff_len=_ramp(2, 2), facts=dict(num_entries=0), no_entries=True),
        # every entry is on haplotype 0 and the mask allows haplotype 1 alone
        _case("mask_removes_everything", 4, 3, 2, some, allowed=[2, 2, 2], facts=dict(num_entries=0), no_entries=True),
        # the mask empties rows 1 and 2 and shortens rows 0, 3 and 5: an ordinary case with values
        _case("mask_empties_some_rows", 6, 3, 2, partly, count=[2, 1, 4, 1, 9, 3], eff_len=_ramp(2, 3), allowed=[3, 2, 1],
              facts=dict(num_entries=5)),
    ]


def _long_row_cases():
    out = []
    for H in (8, 16, 11):
        full = (1 << H) - 1
        out.append(_case(f"only_a_long_row_h{H}", 2, 40, H, [(0, [(l, full) for l in range(40)])], eff_len=_ramp(H, 40),
                         facts=dict(num_tiles=0, num_long_rows=1)))
    return out


def _row_limit_cases():
    """A row of exactly max_row_words loci stays in the tiles, one locus more makes it a long row; beside ordinary rows."""
    out = []
    for H in (8, 16, 11):
        limit = PLAN[(H, False, False)].max_row_words
        for extra in (0, 1):
            n = limit + extra
            rng = np.random.default_rng(700 + 2 * H + extra)
            rows = [(1, [(l, int(rng.integers(1, 1 << H))) for l in range(3, 3 + n)])]
            for r in (0, 2, 4, 5, 6):
                loci = np.sort(rng.choice(40, size=int(rng.integers(1, 4)), replace=False))
                rows.append((r, [(int(l), int(rng.integers(1, 1 << H))) for l in loci]))
            out.append(_case(f"row_of_{n}_words_h{H}", 7, 40, H, rows, eff_len=_ramp(H, 40),
                             facts=dict(num_tiles=1, num_long_rows=extra)))
    return out


# (name, H, counts given, deterministic): one one-word read on each of L loci, in locus order; read r fills dictionary
# entry r, and a tile ends where r passes a multiple of dseg
DICTIONARY_FLAVOURS = [("h1", 1, False, False), ("h8", 8, False, False), ("h16", 16, False, False),
                       ("h8_weighted", 8, True, False), ("h8_deterministic", 8, False, True)]
# name -> {L: num_tiles} at L = dseg - 1, dseg, dseg + 1, d_max, d_max + 1
DICTIONARY_TILES = {
    "h1": {991: 1, 992: 1, 993: 2, 1024: 2, 1025: 2},
    "h8": {351: 1, 352: 1, 353: 2, 384: 2, 385: 2},
    "h16": {291: 1, 292: 1, 293: 2, 300: 2, 301: 2},
    "h8_weighted": {543: 1, 544: 1, 545: 2, 576: 2, 577: 2},
    "h8_deterministic": {15: 1, 16: 1, 17: 2, 48: 3, 49: 4},
}


def _dictionary_cases():
    out = []
    for name, H, weighted, det in DICTIONARY_FLAVOURS:
        for L, tiles in DICTIONARY_TILES[name].items():
            rng = np.random.default_rng(900 + L)
            rows = [(l, [(l, int(rng.integers(1, 1 << H)))]) for l in range(L)]
            count = rng.integers(1, 5, size=L) if weighted else None
            out.append(_case(f"dictionary_{name}_L{L}", L, L, H, rows, count=count, env=dict(TILE_WORDS=TILE_WORDS_HIGH),
                             home_flags=FLAG_DETERMINISTIC if det else 0, facts=dict(num_tiles=tiles, num_long_rows=0)))
    return out


def _batch_cases():
    """One batch of 64 one-word reads, one less, one more: one locus, one mask."""
    out = []
    for H, mask in ((1, 1), (8, 0xA5)):
        for R in (63, 64, 65):
            for counted in (False, True):
                out.append(_case(f"batch_{R}_reads_h{H}" + ("_counts" if counted else ""), R, 1, H,
                                 [(r, [(0, mask)]) for r in range(R)], count=np.arange(1, R + 1) if counted else None,
                                 eff_len=_ramp(H, 1)))
    return out


def _identical_rows_case():
    return _case("fifty_identical_rows", 50, 5, 4, [(r, [(0, 0b0101), (2, 0b0011), (4, 0b1000)]) for r in range(50)],
                 eff_len=_ramp(4, 5))


def _full_mask_cases():
    out = []
    for H in (8, 16, 32):
        full = (1 << H) - 1
        rows = [(0, [(0, full)]), (1, [(0, full), (1, full)]), (2, [(1, full), (2, full), (3, full)]), (4, [(3, full)]),
                (5, [(0, full), (3, full)])]
        out.append(_case(f"full_masks_h{H}", 6, 4, H, rows, count=[1, 2, 3, 4, 5, 6], eff_len=_ramp(H, 4)))
    return out


# ---- every haplotype count -------------------------------------------------------------------------------------------------

SWEEP_R, SWEEP_L = 200, 37      # L * H is a multiple of 256 for no H <= 32, and the locus count is odd
SWEEP_H = list(range(1, 33))


def sweep_case(H, counted):
    """160 random rows of 1-6 loci with random non-zero masks, 20 empty rows (row 0 and the last among them), 19 copies
    of one one-word read, one row on every locus with the full mask (a long row at every H), integer lengths of 1-900."""
    rng = np.random.default_rng(3200 + H)
    R, L = SWEEP_R, SWEEP_L
    order = rng.permutation(np.arange(1, R - 1))
    empty = {0, R - 1} | {int(r) for r in order[:18]}
    copies = [int(r) for r in order[18:37]]
    long_row = int(order[37])
    rows = []
    top = 1 << H
    for r in sorted(int(x) for x in order[38:]):
        loci = np.sort(rng.choice(L, size=int(rng.integers(1, 7)), replace=False))
        rows.append((r, [(int(l), int(rng.integers(1, top))) for l in loci]))
    one_word = (int(rng.integers(0, L)), int(rng.integers(1, top)))
    rows += [(r, [one_word]) for r in copies]
    rows.append((long_row, [(l, top - 1) for l in range(L)]))
    rows.sort()
    assert len(rows) == R - len(empty) == 180 and not empty & {r for r, _ in rows}
    eff = rng.integers(1, 901, size=(H, L)).astype(np.float64)
    count = rng.integers(1, 5, size=R) if counted else None
    facts = dict(num_long_rows=1) if H <= 16 else {}
    return _case(f"sweep_h{H}" + ("_counts" if counted else ""), R, L, H, rows, count=count, eff_len=eff, facts=facts)


def degenerate_cases():
    return (_first_cases() + _corner_cases() + _no_entry_cases() + _long_row_cases() + _row_limit_cases()
            + _dictionary_cases() + _batch_cases() + [_identical_rows_case()] + _full_mask_cases())


_cases = {}


def all_cases():
    """name -> case, degenerate shapes first; built once."""
    if not _cases:
        for c in degenerate_cases() + [sweep_case(H, counted) for H in SWEEP_H for counted in (False, True)]:
            assert c.name not in _cases
            _cases[c.name] = c
    return _cases


def case_names():
    return list(all_cases())


# ---- a case in the forms its users take ------------------------------------------------------------------------------------

def csc_of(case):
    """The unmasked CSC arrays (small_ops_cases.Case) of a case."""
    row_list = [[] for _ in range(case.R)]
    for r, pairs in case.rows:
        row_list[r] = pairs
    return csc_from_rows(case.L, case.H, row_list)


def gtmask_of(case):
    """(H x L) 0/1 matrix of the case's `-G` mask, or None."""
    if case.allowed is None:
        return None
    return ((case.allowed[None, :].astype(np.int64) >> np.arange(case.H)[:, None]) & 1).astype(np.float64)


def masked_csc_of(case):
    """(indptr, indices) per haplotype with the masked columns dropped: what a host that carries the mask out hands over."""
    csc, keep = csc_of(case), gtmask_of(case)
    indptr, indices = [], []
    for h in range(case.H):
        width = np.diff(csc.indptr[h].astype(np.int64))
        keep_col = keep[h] != 0
        indices.append(csc.indices[h][np.repeat(keep_col, width)])
        indptr.append(np.concatenate(([0], np.cumsum(np.where(keep_col, width, 0)))).astype(np.uint32))
    return indptr, indices


def exact_of(case, number=None):
    kw = {} if number is None else dict(number=number)
    return ExactEM(case.R, case.L, case.H, case.rows, case.count, case.eff_len, case.allowed, **kw)


def dense(d, H, L):
    """A dict (hap, locus) -> number as a float64 (H x L) matrix."""
    out = np.zeros((H, L), dtype=np.float64)
    for (h, l), v in d.items():
        out[h, l] = float(v)
    return out


Expected = collections.namedtuple("Expected", "theta0 theta0_pc theta counts err posterior")
PSEUDOCOUNT, STEPS = 0.5, 3
_expected = {}


def expected_of(case):
    """What em_exact gives for a case, rounded to float64 once and shared by every test; never written to.
    theta0 / theta0_pc: after prepare(0) / prepare(0.5); theta[k]: after k + 1 steps from theta0; counts, err, posterior
    (dict (row, locus, hap) -> float): of those three steps, the posterior of the last."""
    if case.name not in _expected:
        H, L = case.H, case.L
        em = exact_of(case)
        theta0_pc = dense(em.prepare(PSEUDOCOUNT).theta, H, L)
        theta0 = dense(em.prepare(0.0).theta, H, L)
        thetas, err, counts, post = [], [], None, {}
        if not case.no_entries:
            start = dict(em.theta)
            for _ in range(STEPS):
                thetas.append(dense(em.step().theta, H, L))
            counts = dense(em.expected_counts(), H, L)
            post = {k: float(v) for k, v in em.posterior().items()}
            em.set_theta(start)
            err = [float(e) for e in em.run(STEPS).err_history]
            assert np.array_equal(dense(em.theta, H, L), thetas[-1])
        for a in [theta0, theta0_pc, counts] + thetas:
            if a is not None:
                a.setflags(write=False)
        _expected[case.name] = Expected(theta0, theta0_pc, thetas, counts, err, post)
    return _expected[case.name]
