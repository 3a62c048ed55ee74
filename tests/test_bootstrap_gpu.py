"""Bootstrap replicates on the device (GBRS_EM_RESAMPLE, gbrs_em_resample, gbrs_em_bootstrap_*, `gbrs quantify
--bootstrap`) against the numpy restatement of the draw and the CPU oracles run on the restated input: the file in
which row r occurs w(b, r) times (needs an MI355X)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bootstrap_restate as br
from conftest import GOLD, em_case_inputs, golden_files, load_golden
from em_models_restate import ModelsEM, fixture_inputs

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SEEDS = (0, 2 ** 63 + 5)
REPLICATES = (0, 1, 2 ** 32 - 2)
# tiles: the default stream order; interleaved: GBRS_EM_NO_STREAMS | GBRS_EM_FORCE_INTERLEAVE
LAYOUTS = {"tiles": dict(), "csc": dict(csc_layout=True), "deterministic": dict(deterministic=True),
           "interleaved": dict(extra_flags=16 | 8), "grouped": dict(grouped_models=True)}
EM_FILES = [p for p in golden_files("em") if "values0" not in load_golden(p)]
MODEL_FILES = [p for p in golden_files("emmodel") if "values0" not in load_golden(p)]


def _id(p):
    return os.path.basename(p)[:-4]


def close(a, b, rtol=RTOL):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def pack_mask(gtmask):
    H = gtmask.shape[0]
    return ((gtmask != 0).astype(np.uint32) << np.arange(H, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32)


def make_apm(inputs):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = inputs[:9]
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)])
    apm.groups = groups
    apm.gname = np.array([f"G{i:07d}" for i in range(len(groups))])
    apm.num_groups = len(groups)
    if gtmask is not None:
        apm.set_haplotype_mask(pack_mask(gtmask))
    return apm


def make_em(inputs, layout="tiles", pseudocount=0.0, resample=True, **kw):
    from gbrs_amd.em import EMfactory
    em = EMfactory(make_apm(inputs), resample=resample, **LAYOUTS[layout], **kw)
    em.target_lengths = inputs[6]
    em.prepare(pseudocount=pseudocount)
    return em


def synthetic_inputs():
    """1537 rows x 97 loci x 8 haplotypes; counts 1-3 but for one row of 10,000, one of 0 and the last of 70,000."""
    from gbrs_amd import synth
    inc = synth.make_em_problem(R=1537, H=8, L=97, seed=77)
    count = (1 + np.arange(1537) % 3).astype(np.float64)
    count[5], count[6], count[1536] = 10000.0, 0.0, 70000.0
    return (inc.num_rows, inc.num_loci, inc.num_haps, inc.indptr, inc.indices, count, inc.effective_length(100), [], None)


@functools.lru_cache(maxsize=None)
def weight_case(name):
    inputs = synthetic_inputs() if name == "synthetic" else em_case_inputs(load_golden(os.path.join(GOLD, name + ".npz")))
    R, count = inputs[0], inputs[5]
    want = {(s, b): br.weights(s, b, R, count) for s in SEEDS for b in REPLICATES}
    return inputs, want


# ---------------------------------------------------------------------------------------------- weights, exact
@pytest.mark.parametrize("layout", ["tiles", "csc", "deterministic", "grouped"])
@pytest.mark.parametrize("name", ["em_h2_plain", "em_h8_count_len", "em_h8_emptyrows", "em_h8_mask", "synthetic"])
def test_weights_equal_the_restatement(name, layout):
    """Integer equality with the restatement for every (seed, replicate), the same vector on every layout, and
    GBRS_RESAMPLE_BASE restores the count exactly."""
    from gbrs_amd import _lib
    inputs, want = weight_case(name)
    R, count = inputs[0], inputs[5]
    base = np.ones(R) if count is None else np.asarray(count, dtype=np.float64)
    em = make_em(inputs, layout)
    assert np.array_equal(em.weights(), base)
    for (seed, b), w in want.items():
        em.resample(seed, b)
        got = em.weights()
        assert got.dtype == np.float64 and np.array_equal(got, w.astype(np.float64)), (seed, b)
    em.resample(SEEDS[1], _lib.GBRS_RESAMPLE_BASE)
    assert np.array_equal(em.weights(), base)
    em.close()
    if name == "synthetic":
        w = want[(0, 0)]
        assert w[6] == 0 and abs(w[5] - 10000) < 600 and abs(w[1536] - 70000) < 1600      # six standard deviations


def _raw_create(inputs, flags, count="file"):
    from gbrs_amd import _lib
    lib = _lib.load()
    R, L, H, indptr, indices, cnt, eff_len = inputs[:7]
    if not isinstance(count, str):
        cnt = count
    h = C.c_void_p()
    eff = None if eff_len is None else np.ascontiguousarray(eff_len)
    cnt = None if cnt is None else np.ascontiguousarray(cnt, dtype=np.float64)
    st = lib.gbrs_em_create(R, L, H, _lib.ptr_table(indptr), _lib.ptr_table(indices), _lib.ptr(cnt), _lib.ptr(eff), 0,
                            flags, C.byref(h))
    return lib, st, h


def test_abi_errors():
    from gbrs_amd import _lib
    inputs = em_case_inputs(load_golden(os.path.join(GOLD, "em_h8_count_len.npz")))
    R, count = inputs[0], inputs[5]
    out = np.zeros(R)
    # without the flag: resample and weights are a state error
    lib, st, h = _raw_create(inputs, 0)
    assert st == 0
    assert lib.gbrs_em_resample(h, 1, 0) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_weights(h, _lib.ptr(out)) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_resample_info(h, None, None, None) == _lib.GBRS_ERR_STATE
    lib.gbrs_em_destroy(h)
    # refused combinations
    for extra in (_lib.GBRS_EM_MERGE_IDENTICAL_ROWS, _lib.GBRS_EM_SIDE_BY_SIDE):
        lib, st, h = _raw_create(inputs, _lib.GBRS_EM_RESAMPLE | extra)
        assert st == _lib.GBRS_ERR_UNSUPPORTED and not h.value
    # counts that are no number of draws
    for r, bad in ((3, -1.0), (0, 2.5), (R - 1, 4294967296.0), (7, np.nan)):
        c = count.copy()
        c[r] = bad
        lib, st, h = _raw_create(inputs, _lib.GBRS_EM_RESAMPLE, count=c)
        assert st == _lib.GBRS_ERR_INVALID and not h.value, bad
    c = count.copy()
    c[0] = 4294967295.0                                     # the largest count is fine at create
    lib, st, h = _raw_create(inputs, _lib.GBRS_EM_RESAMPLE, count=c)
    assert st == 0
    lib.gbrs_em_destroy(h)
    # stored values have no place on a resampling handle
    lib, st, h = _raw_create(inputs, _lib.GBRS_EM_RESAMPLE | _lib.GBRS_EM_KEEP_CSC)
    assert st == 0
    vals = [np.ones(len(ix)) for ix in inputs[4]]
    assert lib.gbrs_em_set_initial_values(h, _lib.ptr_table(vals)) == _lib.GBRS_ERR_UNSUPPORTED
    # statistics: add and get before begin, get before any replicate
    assert lib.gbrs_em_bootstrap_add(h, None, None, None, None) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_bootstrap_get(h, 0, None, None, None, None, None, None, None, None, None) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_bootstrap_begin(h, 0, None, None) == 0
    assert lib.gbrs_em_bootstrap_get(h, 0, None, None, None, None, None, None, None, None, None) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_bootstrap_get(h, 1, None, None, None, None, None, None, None, None, None) == _lib.GBRS_ERR_INVALID
    # a run needs a prepare after a resample
    assert lib.gbrs_em_prepare(h, 0.0) == 0
    assert lib.gbrs_em_resample(h, 3, 1) == 0
    n = C.c_int(0)
    assert lib.gbrs_em_run(h, 4, 1e-4, 5, C.byref(n), None, 0, None) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_prepare(h, 0.0) == 0
    assert lib.gbrs_em_run(h, 4, 1e-4, 5, C.byref(n), None, 0, None) == 0 and n.value > 0
    extra, big, cut = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    assert lib.gbrs_em_resample_info(h, C.byref(extra), C.byref(big), C.byref(cut)) == 0
    assert extra.value >= 4 * R and cut.value > 0 and big.value == int((count > cut.value).sum())
    lib.gbrs_em_destroy(h)


# ---------------------------------------------------------------------------------------------- a replicate is a fit
@functools.lru_cache(maxsize=None)
def model4_reference(path):
    """EMOracle on the restated input of replicates 0..3, seed 2024, with the file's own pseudocount, tolerance and cap."""
    from oracle.em_oracle import EMOracle
    g = load_golden(path)
    inputs = em_case_inputs(g)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = inputs
    refs = []
    for b in range(4):
        w = br.weights(2024, b, R, count)
        ptr, idx, cnt = br.restate_input(indptr, indices, w)
        o = EMOracle(R, L, H, ptr, idx, cnt)
        if gtmask is not None:
            o.apply_genotype_mask(gtmask)
        o.prepare(float(g["pseudocount"]), eff_len)
        theta0 = o.theta.copy()
        n = o.run(tol=float(g["tol"]), max_iters=int(g["max_iters"]))        # raises on a float error
        refs.append(dict(w=w, theta0=theta0, theta=o.theta.copy(), counts=o.expected_read_counts(), n=n,
                         hist=list(o.err_history)))
    return g, inputs, refs


@pytest.mark.parametrize("layout", ["tiles", "csc", "deterministic", "interleaved"])
@pytest.mark.parametrize("path", EM_FILES, ids=_id)
def test_model4_replicate_is_the_fit_of_the_restated_file(path, layout):
    g, inputs, refs = model4_reference(path)
    pc = float(g["pseudocount"])
    em = make_em(inputs, layout, pseudocount=pc)
    for b, ref in enumerate(refs):
        assert (ref["w"] == 0).any() and (ref["theta"].sum(axis=0) == 0).any()       # the zero-weight rule is exercised
        em.resample(2024, b)
        assert np.array_equal(em.weights(), ref["w"].astype(np.float64))
        em.reprepare(pc)
        close(em.allelic_expression, ref["theta0"])
        em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
        assert em.num_iters == ref["n"], (b, em.num_iters, ref["n"])
        np.testing.assert_allclose(em.err_history, ref["hist"], rtol=1e-7)
        close(em.allelic_expression, ref["theta"])
        close(em.expected_read_counts(), ref["counts"])
    em.close()


@functools.lru_cache(maxsize=None)
def models_reference(path):
    from oracle.em_oracle import EMOracle
    g = load_golden(path)
    inputs = fixture_inputs(g)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = inputs
    refs = []
    for b in range(2):
        w = br.weights(2024, b, R, count)
        ptr, idx, cnt = br.restate_input(indptr, indices, w)
        o = EMOracle(R, L, H, ptr, idx, cnt)
        if gtmask is not None:
            o.apply_genotype_mask(gtmask)
        o.prepare(float(g["pseudocount"]), eff_len)
        cpu = ModelsEM(R, L, H, ptr, idx, cnt, eff_len, groups, gtmask)
        old = np.seterr(all="raise", under="ignore")
        try:
            theta, counts, hist = cpu.run(o.theta.copy(), int(g["model"]), float(g["tol"]), int(g["max_iters"]))
        finally:
            np.seterr(**old)
        assert np.isfinite(theta).all()
        refs.append(dict(w=w, theta0=o.theta.copy(), theta=theta, counts=counts, hist=hist))
    return g, inputs, refs


@pytest.mark.parametrize("layout", ["tiles", "csc"])
@pytest.mark.parametrize("path", MODEL_FILES, ids=_id)
def test_models123_replicate_is_the_fit_of_the_restated_file(path, layout):
    g, inputs, refs = models_reference(path)
    model, pc = int(g["model"]), float(g["pseudocount"])
    em = make_em(inputs, layout, pseudocount=pc, grouped_models=True)
    for b, ref in enumerate(refs):
        em.resample(2024, b)
        em.reprepare(pc)
        close(em.allelic_expression, ref["theta0"])
        em.run(model=model, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
        assert em.num_iters == len(ref["hist"]), (b, em.num_iters, len(ref["hist"]))
        np.testing.assert_allclose(em.err_history, ref["hist"], rtol=1e-7)
        close(em.allelic_expression, ref["theta"])
        close(em.expected_read_counts(), ref["counts"])
    em.close()


def long_row_inputs():
    """400 rows x 60 loci x 2 haplotypes; every 50th row aligns to 40 loci - more than a tile row holds, so it goes to
    the long-row kernels - and the rows before 100 carry counts of 0-3."""
    rng = np.random.default_rng(8)
    R, L, H = 400, 60, 2
    dense = np.zeros((H, R, L), dtype=bool)
    for r in range(R):
        loci = rng.choice(L, size=40 if r % 50 == 7 else 1 + r % 3, replace=False)
        for l in loci:
            m = rng.integers(1, 4)
            dense[0, r, l], dense[1, r, l] = m & 1, m >> 1
    indptr, indices = [], []
    for h in range(H):
        rows, cols = np.nonzero(dense[h].T)[::-1]             # column-major: row ids ascending inside a locus
        indptr.append(np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=L)))).astype(np.uint32))
        indices.append(rows.astype(np.uint32))
    count = np.ones(R)
    count[:100] = np.arange(100) % 4
    eff = np.tile(200.0 + 7 * np.arange(L), (H, 1))
    return (R, L, H, indptr, indices, count, eff, [], None)


@pytest.mark.parametrize("layout", ["tiles", "csc", "deterministic"])
def test_long_rows_take_the_drawn_weights(layout):
    from oracle.em_oracle import EMOracle
    inputs = long_row_inputs()
    R, L, H, indptr, indices, count, eff_len = inputs[:7]
    em = make_em(inputs, layout)
    if layout != "csc":
        assert em.info().num_long_rows == 8
    for b in range(3):
        w = br.weights(5, b, R, count)
        assert (w[7::50] == 0).any() and (w[7::50] > 0).any() or b > 0
        ptr, idx, cnt = br.restate_input(indptr, indices, w)
        o = EMOracle(R, L, H, ptr, idx, cnt)
        o.prepare(0.0, eff_len)
        em.resample(5, b)
        em.reprepare(0.0)
        close(em.allelic_expression, o.theta)
        n = o.run(tol=1e-4, max_iters=40)
        em.run(model=4, tol=1e-4, max_iters=40, verbose=False)
        assert em.num_iters == n
        close(em.allelic_expression, o.theta)
        close(em.expected_read_counts(), o.expected_read_counts())
    em.close()


def test_deterministic_replicate_is_bit_identical_twice():
    g, inputs, refs = model4_reference(os.path.join(GOLD, "em_h8_count_len.npz"))
    thetas = []
    for _ in range(2):
        em = make_em(inputs, "deterministic")
        em.resample(2024, 1)
        em.reprepare(0.0)
        em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
        thetas.append((em.allelic_expression.copy(), em.expected_read_counts(), em.num_iters))
        em.close()
    assert thetas[0][2] == thetas[1][2]
    assert np.array_equal(thetas[0][0], thetas[1][0]) and np.array_equal(thetas[0][1], thetas[1][1])


@pytest.mark.parametrize("layout", ["tiles", "csc", "deterministic"])
def test_ordinary_handles_keep_the_zero_denominator_error(layout):
    """Without the flag nothing changes: a count fixture gives the reference's numbers, and a row whose alignments all
    have zero abundance is a float error whatever its count - also when the count is 0."""
    g = load_golden(os.path.join(GOLD, "em_h8_count_len.npz"))
    inputs = list(em_case_inputs(g))
    em = make_em(inputs, layout, resample=False)
    close(em.allelic_expression, g["theta0"])
    em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    close(em.allelic_expression, g["theta_final"])
    close(em.expected_read_counts(), g["expected_counts"])
    em.close()
    # rows over all-zero theta whose count is 0: an error on an ordinary handle, none on a resampling one
    R, L, H, indptr, indices, count = inputs[:6]
    row = int(np.asarray(indices[0])[0])
    hit = np.zeros(L, dtype=bool)
    cols = [np.repeat(np.arange(L), np.diff(np.asarray(indptr[h], dtype=np.int64))) for h in range(H)]
    for h in range(H):
        hit[cols[h][np.asarray(indices[h]) == row]] = True
    outside = np.zeros(R, dtype=bool)                   # rows with an alignment to a locus that keeps its theta
    for h in range(H):
        outside[np.asarray(indices[h], dtype=np.int64)[~hit[cols[h]]]] = True
    count0 = count.copy()
    count0[~outside] = 0.0
    assert not outside[row] and (count0 > 0).any()
    inputs[5] = count0
    for resample, fails in ((False, True), (True, False)):
        em = make_em(inputs, layout, resample=resample)
        theta = em.allelic_expression.copy()
        theta[:, hit] = 0.0
        em.allelic_expression = theta
        if fails:
            with pytest.raises(FloatingPointError):
                em.update_allelic_expression(4)
        else:
            em.update_allelic_expression(4)
            assert np.isfinite(em.allelic_expression).all() and (em.allelic_expression[:, hit] == 0.0).all()
        em.close()


# ---------------------------------------------------------------------------------------------- statistics
def device_sum(theta):
    """Sum of theta in the order of the device's stats_sum_kernel: locus-major elements, thread t adds the elements
    t, t + 1024, ... in order, then a halving tree over the 1024 threads."""
    v = np.ascontiguousarray(theta.T).ravel()
    v = np.concatenate((v, np.zeros(-len(v) % 1024)))
    s = np.zeros(1024)
    for chunk in v.reshape(-1, 1024):
        s = s + chunk
    half = 512
    while half:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0]


def _check_statistics(stats, kept_tpm, kept_cnt):
    B = kept_tpm.shape[0]
    assert stats["num_replicates"] == B
    for key, kept in (("tpm", kept_tpm), ("count", kept_cnt)):
        for suffix, x in (("", kept), ("_total", kept.sum(axis=1))):
            mean, sd = x.mean(axis=0), x.std(axis=0, ddof=1)
            np.testing.assert_allclose(stats[f"{key}{suffix}_mean"], mean, rtol=1e-12, atol=1e-300)
            err = np.abs(stats[f"{key}{suffix}_sd"] - sd)
            assert (err <= 1e-9 * sd + 1e-12 * np.abs(mean)).all(), (key, suffix, err.max())


@pytest.mark.parametrize("name", ["em_h8_len", "emmodel_m3_h8_len"])
def test_bootstrap_statistics(name):
    """em.bootstrap(replicates=8, keep=True): the kept replicates are the single-replicate path, the means and standard
    deviations those of numpy over the kept arrays (a Welford update differs from the two-pass form by about B
    roundings), at isoform level, gene level and for the totals.

    Model 4 runs on the bit-reproducible E-step, so a kept replicate equals a fresh single-replicate run bit for bit.
    Models 1-3 have no bit-reproducible form (GBRS_ERR_UNSUPPORTED with GBRS_EM_DETERMINISTIC: their sums use float
    atomics), so two runs of one replicate may differ in the last bits; there the fresh run is held to the project's
    1e-9, and bit equality is checked where it is defined: the values a replicate is folded in with are, bit for bit,
    the handle's own theta scaled by 1e6 / (its sum in the device's order) and its own expected counts."""
    g = load_golden(os.path.join(GOLD, name + ".npz"))
    model4 = name.startswith("em_")
    inputs = em_case_inputs(g) if model4 else fixture_inputs(g)
    model = 4 if model4 else int(g["model"])
    pc, tol, cap = float(g["pseudocount"]), float(g["tol"]), int(g["max_iters"])
    layout = "deterministic" if model4 else "tiles"
    kw = {} if model4 else dict(grouped_models=True)
    em = make_em(inputs, layout, pseudocount=pc, **kw)
    res = em.bootstrap(model, 8, seed=99, pseudocount=pc, tol=tol, max_iters=cap, keep=True)
    R, L, H = inputs[0], inputs[1], inputs[2]
    G = len(inputs[7])
    assert res["tpm"].shape == res["expected_read_counts"].shape == (8, H, L)
    assert res["gene_tpm"].shape == res["gene_expected_read_counts"].shape == (8, H, G)
    assert res["num_iters"].shape == (8,) and (res["num_iters"] > 0).all()
    count = inputs[5]
    assert np.array_equal(em.weights(), np.ones(R) if count is None else count)      # the base weights are back
    _check_statistics(res["isoforms"], res["tpm"], res["expected_read_counts"])
    _check_statistics(res["genes"], res["gene_tpm"], res["gene_expected_read_counts"])
    em.close()
    # the single-replicate path on a fresh handle
    one = make_em(inputs, layout, pseudocount=pc, **kw)
    gptr, mem = one.probability.group_csr()
    for b in range(8):
        one.resample(99, b)
        one.reprepare(pc)
        one.run(model=model, tol=tol, max_iters=cap, verbose=False)
        one.bootstrap_begin()
        vals = one.bootstrap_add(keep=True)
        theta, counts = one.allelic_expression, one.expected_read_counts()
        # what is folded in is the handle's own result, bit for bit
        assert np.array_equal(vals["tpm"], theta * (1000000.0 / device_sum(theta)))
        assert np.array_equal(vals["expected_read_counts"], counts)
        for key, src in (("gene_tpm", vals["tpm"]), ("gene_expected_read_counts", counts)):
            want = np.zeros((H, G))
            for i in range(G):
                for m in mem[gptr[i]:gptr[i + 1]]:
                    want[:, i] += src[:, m]
            assert np.array_equal(vals[key], want)
        for kept_key, v in (("tpm", vals["tpm"]), ("expected_read_counts", vals["expected_read_counts"]),
                            ("gene_tpm", vals["gene_tpm"]), ("gene_expected_read_counts", vals["gene_expected_read_counts"])):
            if model4:
                assert np.array_equal(res[kept_key][b], v), (kept_key, b)
            else:
                close(res[kept_key][b], v)
        assert one.num_iters == res["num_iters"][b]
    one.close()


# ---------------------------------------------------------------------------------------------- the command
REPORTS = ("isoforms.tpm", "isoforms.expected_read_counts", "genes.tpm", "genes.expected_read_counts")
STAT_KEYS = ("tpm_mean", "tpm_sd", "count_mean", "count_sd")
TOTAL_KEYS = ("tpm_total_mean", "tpm_total_sd", "count_total_mean", "count_total_sd")


def _command_inputs(tmp_path, fmt):
    """em_h8_mask's input as an alignment file with group, length and genotype files that give the fixture's mask."""
    g = load_golden(os.path.join(GOLD, "em_h8_mask.npz"))
    inputs = em_case_inputs(g)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = inputs
    apm = make_apm(inputs[:8] + (None,))
    hn, ln = apm.hname, apm.lname
    aln = tmp_path / f"aln.{fmt}"
    apm.save(str(aln), incidence_only=True)
    # a genotype file can only call genes: the loci in no gene become genes of their own (model 4 looks at no group)
    grouped = {int(m) for mem in groups for m in mem}
    genes = [list(map(int, mem)) for mem in groups] + [[l] for l in range(L) if l not in grouped]
    grp, gt, lens = tmp_path / "g2t.tsv", tmp_path / "gt.tsv", tmp_path / "len.tsv"
    with open(grp, "w") as fh, open(gt, "w") as fg:
        fg.write("#Gene_ID\tDiplotype\n")
        for i, mem in enumerate(genes):
            fh.write(f"G{i:07d}\t" + "\t".join(ln[m] for m in mem) + "\n")
            hs = np.flatnonzero(gtmask[:, mem[0]])
            assert all(np.array_equal(np.flatnonzero(gtmask[:, m]), hs) for m in mem) and len(hs) in (1, 2)
            fg.write(f"G{i:07d}\t" + "".join(hn[h] for h in (hs if len(hs) == 2 else [hs[0], hs[0]])) + "\n")
    with open(lens, "w") as fh:
        for l in range(L):
            for h in hn:
                fh.write(f"{ln[l]}_{h}\t{int(g['raw_length'][l])}\n")
    common = ["quantify", "-i", str(aln), "-g", str(grp), "-L", str(lens), "-t", str(float(g["tol"])),
              "-m", str(int(g["max_iters"]))]
    return g, inputs, genes, common, ["-G", str(gt)]


@pytest.mark.parametrize("masked", [False, True], ids=["multiway", "diploid"])
@pytest.mark.parametrize("fmt", ["npz", "h5"])
def test_quantify_command_bootstrap(tmp_path, monkeypatch, fmt, masked):
    """`gbrs quantify [-G ...] --bootstrap 6 --keep-replicates` end to end, on the bit-reproducible E-step
    (GBRS_EM_DETERMINISTIC=1 for every command of the test): the ordinary reports are byte for byte those of the
    command without the option, the files have the listed keys and shapes, every kept replicate is the library's, and
    the same seed gives the same arrays."""
    from gbrs_amd import cli
    monkeypatch.setenv("GBRS_EM_DETERMINISTIC", "1")
    g, inputs, genes, common, mask_args = _command_inputs(tmp_path, fmt)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = inputs
    if masked:
        common = common + mask_args
    tag = "diploid" if masked else "multiway"
    boot = ["--bootstrap", "6", "--bootstrap-seed", "31", "--keep-replicates"]
    stages = tmp_path / "stages.json"
    monkeypatch.setenv("GBRS_STAGE_TIMES", str(stages))
    assert cli.main(common + ["-o", str(tmp_path / "plain")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "boot")] + boot) == 0
    import json
    assert "bootstrap" in json.load(open(stages)) and "error" not in json.load(open(stages))
    assert cli.main(common + ["-o", str(tmp_path / "again")] + boot) == 0
    for name in REPORTS:
        a = open(tmp_path / f"plain.{tag}.{name}", "rb").read()
        assert len(a) > 0 and a == open(tmp_path / f"boot.{tag}.{name}", "rb").read(), name
    assert not os.path.exists(tmp_path / f"plain.{tag}.isoforms.bootstrap.npz")
    # the library's replicates on the same input
    lib_inputs = inputs[:7] + ([np.asarray(m) for m in genes], gtmask if masked else None)
    em = make_em(lib_inputs, "deterministic")
    res = em.bootstrap(4, 6, seed=31, tol=float(g["tol"]), max_iters=int(g["max_iters"]), keep=True)
    em.close()
    for level, n, tpm_key, cnt_key in (("isoforms", L, "tpm", "expected_read_counts"),
                                       ("genes", len(genes), "gene_tpm", "gene_expected_read_counts")):
        with np.load(tmp_path / f"boot.{tag}.{level}.bootstrap.npz") as z, \
                np.load(tmp_path / f"again.{tag}.{level}.bootstrap.npz") as z2:
            assert set(z.files) == {"names", "haplotypes", "num_replicates", "seed", "multiread_model", "num_iters",
                                    "tpm", "expected_read_counts", *STAT_KEYS, *TOTAL_KEYS}
            assert z["names"].shape == (n,) and z["haplotypes"].tolist() == [chr(65 + h) for h in range(H)]
            assert int(z["num_replicates"]) == 6 and int(z["seed"]) == 31 and int(z["multiread_model"]) == 4
            assert z["num_iters"].shape == (6,) and np.array_equal(z["num_iters"], res["num_iters"])
            for k in STAT_KEYS:
                assert z[k].shape == (H, n)
            for k in TOTAL_KEYS:
                assert z[k].shape == (n,)
            assert z["tpm"].shape == z["expected_read_counts"].shape == (6, H, n)
            assert np.array_equal(z["tpm"], res[tpm_key]) and np.array_equal(z["expected_read_counts"], res[cnt_key])
            for k in z.files:
                assert np.array_equal(z[k], z2[k]), k
            _check_statistics({**{k: z[k] for k in STAT_KEYS + TOTAL_KEYS}, "num_replicates": 6}, z["tpm"],
                              z["expected_read_counts"])
    # without --keep-replicates the replicates stay out of the files
    assert cli.main(common + ["-o", str(tmp_path / "lean"), "--bootstrap", "2"]) == 0
    with np.load(tmp_path / f"lean.{tag}.isoforms.bootstrap.npz") as z:
        assert "tpm" not in z.files and "expected_read_counts" not in z.files and int(z["seed"]) == 0
