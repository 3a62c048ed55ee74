"""The M-step kernels with a compile-time haplotype count (gbrs_amd/csrc/em_mstep.inc): mstep_gather_kernel<H, EXTRA, LEN>,
the fused gather + M-step of a single-GPU step, and mstep_elem_kernel<MODE, H>, the M-step of the sharded path and of
prepare.  A thread owns two adjacent haplotypes of a locus (one at H = 1); an elementwise workgroup of the fused launch
takes MSTEP_EPT * 256 such pairs.

Shapes: H in 1, 2, 4, 8, 16, with and without effective lengths, and L so that the elementwise part is one locus row short
of a workgroup's share, exactly one share, one row past it, three workgroups with a ragged end, and L = 1.  Every handle
with six loci or more holds every class of locus: no read, one slot, exactly 2 slots, exactly HEAVY_SLOTS, HEAVY_SLOTS + 1;
the ragged handle also has a locus with more slot rows than one round of the heavy workgroup takes and three long rows
that cross loci of every class, so that acc_extra is live in all three parts of the kernel.  The folds are off
(GBRS_TUNING_RUN_WORDS=0) and the tiles hold 64 words (GBRS_TUNING_TILE_WORDS=64): every read is one word, the reads of a
locus are adjacent, so a locus with n reads that start at word a has (a + n - 1) // 64 - a // 64 + 1 slots.

Compared: theta after prepare and after 1, 2 and 5 steps and the expected counts against the numpy oracle (1e-9), the error
history (1e-7), and theta against the same input under GBRS_TUNING_NO_FUSED_MSTEP=1 at 1e-12: every sum has non-negative
terms, and the two builds differ in the order of a few hundred of them at most (n * 2^-53), beside the E-step's LDS
atomics (1e-15 from run to run).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9             # against the numpy oracle (tests/test_em_gpu.py)
RTOL_ERR = 1e-7         # the error history (tests/test_em_gpu.py)
ATOL_ERR = 1e-8         # the error sums differences of values up to 1e6, each rounded at 1e6 * 2^-52 = 2e-10: its floor at L = 1 and
                        # at one haplotype, where the oracle's error is 0 or 1e-10
RTOL_FORMS = 1e-12      # one launch against two in the same build
ITERS = (1, 2, 5)
NO_LOCUS_SETS = 512     # GBRS_EM_NO_LOCUS_SETS
MSTEP_EPT, THREADS = 2, 256      # em_mstep.inc: pairs per thread and threads of an elementwise workgroup
HEAVY_SLOTS, HEAVY_ROWS = 16, 16           # em_layout.h, em_mstep.inc
TILE = 64
HAPS = (1, 2, 4, 8, 16)
LONG_LOCI = 40          # loci of a long row: past max_row_words (32 up to 8 haplotypes, 8 at 16)


def share(H):
    """Loci of one elementwise workgroup: a locus takes H / 2 threads (one at H = 1)."""
    return MSTEP_EPT * THREADS // max(H // 2, 1)


def shapes(H):
    s = share(H)
    return {"short": s - 1, "exact": s, "past": s + 1, "ragged": 2 * s + 37, "one": 1}


def make_problem(H, L, ragged, seed):
    """(reads per locus, locus and mask of every one-word read, long rows).  The special loci lead, each a multiple of 64
    reads, so their slots do not depend on the rest."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 4, size=L)
    if L >= 6:
        big = TILE * (HEAVY_ROWS * THREADS // H + 1) if ragged else TILE * 3       # ragged: one round of the heavy workgroup and a row
        n[:6] = [TILE * 2, TILE * HEAVY_SLOTS, TILE * (HEAVY_SLOTS + 1), big, 0, 3]
    else:
        n[:] = 5
    locus = np.repeat(np.arange(L), n)
    mask = rng.integers(1, 1 << H, size=len(locus))
    order = rng.permutation(len(locus))               # the layout sorts the reads itself
    long_rows = []
    if ragged:
        for _ in range(3):
            loci = np.concatenate([[0, 1, 2, 3, 5], 6 + rng.choice(L - 6, size=LONG_LOCI - 5, replace=False)])
            long_rows.append((loci, rng.integers(1, 1 << H, size=LONG_LOCI)))
    return n, locus[order], mask[order], long_rows


def slot_classes(n):
    """(light, heavy) loci of the 64-word tiles over the sorted one-word reads."""
    end = np.cumsum(n)
    start = end - n
    slots = np.where(n > 0, (end - 1) // TILE - start // TILE + 1, 0)
    return int(((slots >= 2) & (slots <= HEAVY_SLOTS)).sum()), int((slots > HEAVY_SLOTS).sum()), slots


def to_csc(locus, mask, long_rows, L, H):
    row = np.arange(len(locus))
    rows, loci, masks = [row], [locus], [mask]
    for k, (ll, mm) in enumerate(long_rows):
        rows.append(np.full(len(ll), len(locus) + k))
        loci.append(ll)
        masks.append(mm)
    rows, loci, masks = np.concatenate(rows), np.concatenate(loci), np.concatenate(masks)
    indptr, indices = [], []
    for h in range(H):
        sel = ((masks >> h) & 1) == 1
        r, l = rows[sel], loci[sel]
        o = np.lexsort((r, l))
        indices.append(r[o].astype(np.uint32))
        indptr.append(np.searchsorted(l[o], np.arange(L + 1)).astype(np.uint32))
    return len(locus) + len(long_rows), indptr, indices


def eff_table(H, L):
    return 50.0 + 10.0 * np.random.default_rng(11).integers(0, 200, size=(H, L)).astype(np.float64)


_CACHE = {}


def problem(H, shape, with_len):
    """The input and the oracle's states of one case: made once, read-only."""
    key = (H, shape, with_len)
    if key not in _CACHE:
        from oracle.em_oracle import EMOracle
        L = shapes(H)[shape]
        n, locus, mask, long_rows = make_problem(H, L, shape == "ragged", seed=100 * H + len(shape))
        R, indptr, indices = to_csc(locus, mask, long_rows, L, H)
        eff = eff_table(H, L) if with_len else None
        o = EMOracle(R, L, H, indptr, indices, None)
        o.prepare(0.0, eff)
        states, err = {0: o.theta.copy()}, []
        for it in range(1, max(ITERS) + 1):             # EMOracle.run's loop without its stopping rule (L = 1: the error is 0)
            prev = o.theta.sum(axis=0)
            o.em_step()
            curr = o.theta.sum(axis=0)
            err.append(np.abs(curr * (1000000.0 / curr.sum()) - prev * (1000000.0 / prev.sum())).sum())
            if it in ITERS:
                states[it] = o.theta.copy()
        states["counts"] = o.expected_read_counts().copy()
        states["err"] = np.array(err)
        for v in states.values():
            v.setflags(write=False)
        _CACHE[key] = dict(L=L, R=R, n=n, indptr=indptr, indices=indices, eff=eff, ref=states)
    return _CACHE[key]


def make_engine(p, H, monkeypatch, fused=True):
    from gbrs_amd.engine import EmEngine
    monkeypatch.setenv("GBRS_TUNING_TILE_WORDS", str(TILE))
    monkeypatch.setenv("GBRS_TUNING_RUN_WORDS", "0")
    monkeypatch.setenv("GBRS_TUNING_LOCUS_SETS", "0")
    for k in ("GBRS_TUNING_NO_PHASE_SPLIT", "GBRS_TUNING_PERSISTENT", "GBRS_TUNING_PERSISTENT_GROUPS", "GBRS_TUNING_NO_FUSED_MSTEP"):
        monkeypatch.delenv(k, raising=False)
    if not fused:
        monkeypatch.setenv("GBRS_TUNING_NO_FUSED_MSTEP", "1")
    return EmEngine.from_host(p["R"], p["L"], H, p["indptr"], p["indices"], None, p["eff"], flags=NO_LOCUS_SETS)


def step_states(eng, partial=False):
    eng.prepare(0.0)
    out = {0: eng.theta()}
    err = []
    for it in range(1, max(ITERS) + 1):
        if partial:
            eng.estep_partial()
            err.append(eng.finish_step(want_err=True))
        else:
            err.append(eng.step(1, want_err=True))
        if it in ITERS:
            out[it] = eng.theta()
    out["counts"] = eng.expected_counts()
    out["err"] = np.array(err)
    return out


def close(a, b, rtol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def check_layout(eng, p, shape):
    """The handle holds the classes of locus the case was made for."""
    inf = eng.info()
    light, heavy, slots = slot_classes(p["n"])
    print(f"L={p['L']} R={p['R']} tiles={inf.num_tiles} slots={inf.num_slots} light={inf.num_light_loci} (model {light}) "
          f"heavy={inf.num_heavy_loci} (model {heavy}) long={inf.num_long_rows}")
    assert inf.num_folded_rows == 0 and inf.num_device_rows == p["R"]
    assert (inf.num_light_loci, inf.num_heavy_loci) == (light, heavy)
    assert inf.num_long_rows == (3 if shape == "ragged" else 0)
    if p["L"] >= 6:
        assert list(slots[:3]) == [2, HEAVY_SLOTS, HEAVY_SLOTS + 1] and slots[4] == 0 and slots[5] == 1
        assert slots[3] == (HEAVY_ROWS * THREADS // inf.num_haps + 1 if shape == "ragged" else 3)


def check_against(got, ref, rtol, with_err=True):
    for k in [0] + list(ITERS) + ["counts"]:
        close(got[k], ref[k], rtol)
    if with_err:
        np.testing.assert_allclose(got["err"], ref["err"], rtol=RTOL_ERR, atol=ATOL_ERR)


@pytest.mark.parametrize("with_len", [False, True], ids=["nolen", "len"])
@pytest.mark.parametrize("shape", ["short", "exact", "past", "ragged", "one"])
@pytest.mark.parametrize("H", HAPS)
def test_fused_mstep_against_oracle_and_two_launches(H, shape, with_len, monkeypatch):
    p = problem(H, shape, with_len)
    eng = make_engine(p, H, monkeypatch)
    check_layout(eng, p, shape)
    got = step_states(eng)
    eng.close()
    two = make_engine(p, H, monkeypatch, fused=False)
    unfused = step_states(two)
    two.close()
    check_against(got, p["ref"], RTOL)
    check_against(unfused, p["ref"], RTOL)
    for k in [0] + list(ITERS):
        close(got[k], unfused[k], RTOL_FORMS)
    # theta of a locus without a read stays exactly zero, and no element the launch does not own is written
    if p["L"] >= 6:
        assert (got[5][:, 4] == 0.0).all()


@pytest.mark.parametrize("H", HAPS)
def test_sharded_mstep_against_oracle(H, monkeypatch):
    """estep_partial + finish_step: the stand-alone gather, then mstep_elem_kernel<0, H> (prepare ran <1, H>)."""
    p = problem(H, "ragged", True)
    eng = make_engine(p, H, monkeypatch)
    got = step_states(eng, partial=True)
    eng.close()
    check_against(got, p["ref"], RTOL)
    q = problem(H, "past", False)
    eng = make_engine(q, H, monkeypatch)
    got = step_states(eng, partial=True)
    eng.close()
    check_against(got, q["ref"], RTOL)


@pytest.mark.parametrize("H,shape,k", [(1, "ragged", 2), (2, "exact", 5), (4, "exact", 5), (8, "exact", 5), (16, "exact", 5)])
def test_run_stops_where_the_oracle_stops(H, shape, k, monkeypatch):
    """gbrs_em_run with a tolerance between the errors of iterations k - 1 and k: the run enqueues its iterations ahead of
    the stop flag, and the stores of the launches behind the stop are guarded - theta is iteration k's.  (At one haplotype
    only the long rows move theta at all: the ragged handle, which is at rounding level from the third iteration on.)"""
    from oracle.em_oracle import EMOracle
    p = problem(H, shape, True)
    o = EMOracle(p["R"], p["L"], H, p["indptr"], p["indices"], None)
    o.prepare(0.0, p["eff"])
    o.run(tol=0.0, max_iters=k + 1)
    before, at = o.err_history[k - 2], o.err_history[k - 1]
    beyond = o.theta.copy()
    target = np.sqrt(before * at)
    assert at * (1 + 1e-3) < target < before * (1 - 1e-3)       # the stop is not within 1e-6 of the tolerance
    o = EMOracle(p["R"], p["L"], H, p["indptr"], p["indices"], None)
    o.prepare(0.0, p["eff"])
    assert o.run(tol=target / 1e6, max_iters=999) == k and k % 8 != 0
    # (one more iteration would show: it moves theta by far more than the tolerance of the comparison)
    assert (np.abs(beyond - o.theta) > 1e-6 * o.theta).any()
    eng = make_engine(p, H, monkeypatch)
    eng.prepare(0.0)
    n_it, hist = eng.run(tol=target / 1e6, max_iters=999)
    theta = eng.theta()
    eng.close()
    assert n_it == k
    np.testing.assert_allclose(hist, o.err_history, rtol=RTOL_ERR, atol=ATOL_ERR)
    close(theta, o.theta, RTOL)
