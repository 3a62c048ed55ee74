"""The tiny EM cases (tests/em_tiny_cases.py: degenerate and boundary shapes, every haplotype count from 1 to 32) on the
device against the 60-digit EM of tests/em_exact.py, over the create flags and the GBRS_TUNING_* variables that pick a
layout or an E-step form (needs an MI355X).  Bounds as in tests/test_em_tiny_cpu.py: theta and counts rtol 1e-9 with atol
1e-300, the err history rtol 1e-7 with atol 4e-3.  Every run prints its largest deviation before it asserts; as written,
the largest over all cases and layouts is 3.3e-15 relative in theta, counts and posteriors (H = 8 and 24) and 4.8e-10
absolute in an err_sum."""
import numpy as np
import pytest

import em_tiny_cases as tc
from em_models_restate import ModelsEM

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-300
ERR_RTOL, ERR_ATOL = 1e-7, 4e-3
CASES = tc.all_cases()
LIVE = [n for n, c in CASES.items() if not c.no_entries]
EMPTY = [n for n, c in CASES.items() if c.no_entries]
MERGE, CSC, FORCE_INTERLEAVE, NO_STREAMS, DETERMINISTIC, NO_LOCUS_SETS = 1, 2, 8, 16, 32, 512

# (name, create flags, GBRS_TUNING_* variables); the variables each on flags 0
CONFIGS = [
    ("default", 0, {}),
    ("merge", MERGE, {}),
    ("csc", CSC, {}),
    ("no_streams", NO_STREAMS, {}),
    ("interleaved", NO_STREAMS | FORCE_INTERLEAVE, {}),
    ("deterministic", DETERMINISTIC, {}),
    ("deterministic_merge", DETERMINISTIC | MERGE, {}),
    ("no_locus_sets", NO_LOCUS_SETS, {}),
    ("whole_row_sets", 0, dict(LOCUS_SETS=1)),
    ("group_sets", 0, dict(LOCUS_SETS=0, GROUP_SETS=1, SET_MIN_ROWS=1)),
    ("both_folds", 0, dict(RUN_WORDS=2)),
    ("one_word_fold", 0, dict(RUN_WORDS=1)),
    ("no_phase_split", 0, dict(NO_PHASE_SPLIT=1)),
    ("tile_words_64", 0, dict(TILE_WORDS=64)),
    ("persistent", 0, dict(PERSISTENT=1, PERSISTENT_GROUPS=2)),
    ("half_loci", 0, dict(HALF_LOCI=1)),            # 16 haplotypes only
    ("two_launch_mstep", 0, dict(NO_FUSED_MSTEP=1)),
]


def configs_for(case):
    return [c for c in CONFIGS if c[0] != "half_loci" or case.H == 16]


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


def deviation(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


_csc = {}


def arrays_of(case):
    if case.name not in _csc:
        _csc[case.name] = tc.csc_of(case)
    return _csc[case.name]


def create(case, flags, env, monkeypatch, masked_on="device"):
    """A handle of the case under the case's and the configuration's variables (read by the library at create)."""
    from gbrs_amd.engine import EmEngine
    csc = arrays_of(case)
    indptr, indices, allowed = csc.indptr, csc.indices, case.allowed
    if allowed is not None and masked_on == "host":
        (indptr, indices), allowed = tc.masked_csc_of(case), None
    with monkeypatch.context() as mp:
        for k, v in dict(case.env, **env).items():
            mp.setenv("GBRS_TUNING_" + k, str(v))
        return EmEngine.from_host(case.R, case.L, case.H, indptr, indices, case.count, case.eff_len, flags=flags,
                                  allowed=allowed)


def check_run(eng, case, label):
    """prepare at both pseudocounts, a run of three iterations with its err history, the expected counts, and the same
    three steps through set_theta + step; returns the largest relative deviation from em_exact."""
    want = tc.expected_of(case)
    got = {}
    eng.prepare(tc.PSEUDOCOUNT)
    got["theta0_pc"] = (eng.theta(), want.theta0_pc)
    eng.prepare(0.0)
    got["theta0"] = (eng.theta(), want.theta0)
    n, hist = eng.run(model=4, tol=0.0, max_iters=tc.STEPS)
    # tol = 0 stops a run before max_iters exactly when its err_sum is 0.0 (test_em_tiny_cpu.check_history)
    assert 1 <= n == len(hist) <= tc.STEPS, (label, n, hist)
    got["theta_run"] = (eng.theta(), want.theta[n - 1])
    if n == tc.STEPS:
        got["counts"] = (eng.expected_counts(), want.counts)
    eng.set_theta(want.theta0)
    eng.step(tc.STEPS)
    got["theta_step"] = (eng.theta(), want.theta[-1])
    got["counts_step"] = (eng.expected_counts(), want.counts)
    worst = max(deviation(a, b) for a, b in got.values())
    err_dev = float(np.max(np.abs(hist - np.asarray(want.err[:n]))))
    print(f"DEVICE_DEVIATION {case.name} {label} H={case.H} theta={worst:.3e} err_abs={err_dev:.3e} iters={n}")
    for key, (a, b) in got.items():
        assert np.isfinite(a).all(), (label, key)
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=f"{label}: {key}")
    np.testing.assert_allclose(hist, want.err[:n], rtol=ERR_RTOL, atol=ERR_ATOL, err_msg=label)
    if n < tc.STEPS:
        assert hist[-1] == 0.0, (label, hist)
    return worst


def check_facts(eng, case, label):
    inf = eng.info()
    for key, value in case.facts.items():
        assert getattr(inf, key) == value, (label, key, getattr(inf, key), value)


@pytest.mark.parametrize("name", LIVE)
def test_case_on_every_layout(name, monkeypatch):
    from gbrs_amd import _lib
    case = CASES[name]
    for label, flags, env in configs_for(case):
        if case.H > 16 and flags & DETERMINISTIC:
            # the documented answer (gbrs_hip.h, GBRS_EM_DETERMINISTIC): not available above 16 haplotypes
            with pytest.raises(_lib.GbrsHipError) as e:
                create(case, flags, env, monkeypatch)
            assert e.value.status == _lib.GBRS_ERR_UNSUPPORTED, label
            continue
        eng = create(case, flags, env, monkeypatch)
        inf = eng.info()
        assert inf.layout == (0 if case.H > 16 or flags & CSC else 1), label
        assert inf.num_entries == tc.exact_of(case).num_entries, label
        if flags == case.home_flags and not env and inf.layout == 1:
            check_facts(eng, case, label)
        if label == "whole_row_sets" and inf.layout == 1 and case.count is None:
            # unweighted rows: the sets are there whenever a read carries several loci under one mask
            if case.allowed is None:
                shared = [pairs for _, pairs in case.rows if len(pairs) > 1 and len({m for _, m in pairs}) == 1]
                assert (inf.num_locus_sets > 0) == bool(shared), (label, inf.num_locus_sets, len(shared))
        check_run(eng, case, label)
        eng.close()


@pytest.mark.parametrize("name", EMPTY)
def test_no_entries(name, monkeypatch):
    """Create succeeds, the handle says it has no entries, prepare gives zeros, a step or a run is the reference's
    FloatingPointError (the total it scales by is zero) and nothing hands back a NaN."""
    case = CASES[name]
    for label, flags, env in configs_for(case):
        eng = create(case, flags, env, monkeypatch)
        assert eng.info().num_entries == 0 and eng.info().num_rows == case.R, label
        for pc in (0.0, tc.PSEUDOCOUNT):
            eng.prepare(pc)
            theta = eng.theta()
            assert theta.shape == (case.H, case.L) and not theta.any(), (label, pc)
        with pytest.raises(FloatingPointError):
            eng.step(1)
        assert np.isfinite(eng.theta()).all(), label
        eng.prepare(0.0)
        with pytest.raises(FloatingPointError):
            eng.run(model=4, tol=0.0, max_iters=tc.STEPS)
        assert np.isfinite(eng.theta()).all() and np.isfinite(eng.expected_counts()).all(), label
        eng.close()


# ---- one shard of a sharded run: the caller all-reduces acc between the two halves of a pass --------------------------------

# the long rows' sums added by the gather, no tile to launch, the per-locus M-step, the width-16 tiles, the CSC kernels
SINGLE_SHARD = ["row_of_33_words_h8", "only_a_long_row_h8", "sweep_h3", "sweep_h16", "sweep_h24"]


@pytest.mark.parametrize("name", SINGLE_SHARD)
def test_single_shard_partial_sequence(name, monkeypatch):
    """prepare_partial -> finish_prepare, then three times estep_partial -> finish_step with its err_sum, as one shard that
    has nothing to add to its own acc; a step of the handle's own after that gathers all of acc as well."""
    case = CASES[name]
    want = tc.expected_of(case)
    eng = create(case, 0, {}, monkeypatch)
    ptr, n = eng.prepare_partial()
    assert ptr and n == case.H * case.L
    eng.finish_prepare(0.0)
    close(eng.theta(), want.theta0)
    errs = []
    for k in range(tc.STEPS):
        assert eng.estep_partial() == (ptr, n)
        errs.append(eng.finish_step(want_err=True))
        theta = eng.theta()
        print(f"SHARD_DEVIATION {name} step={k} theta={deviation(theta, want.theta[k]):.3e} "
              f"err_abs={abs(errs[k] - want.err[k]):.3e}")
        close(theta, want.theta[k])
    close(eng.expected_counts(), want.counts)
    np.testing.assert_allclose(errs, want.err, rtol=ERR_RTOL, atol=ERR_ATOL)
    if name == "row_of_33_words_h8":
        eng.step(1)
        one_more = tc.dense(tc.exact_of(case).prepare(0.0).step(tc.STEPS + 1).theta, case.H, case.L)
        close(eng.theta(), one_more)
    eng.close()


# ---- device arrays -----------------------------------------------------------------------------------------------------------

FROM_DEVICE = ([n for n in CASES if n.startswith("corners_")] + EMPTY
               + [f"sweep_h{H}{c}" for H in (6, 13, 32) for c in ("", "_counts")])


@pytest.mark.parametrize("name", FROM_DEVICE)
def test_from_device(name):
    import torch
    from gbrs_amd.engine import EmEngine
    case = CASES[name]
    csc = arrays_of(case)

    def dev(a, dtype):
        t = torch.zeros(max(len(a), 1), dtype=dtype, device="cuda")       # (never a null pointer for an empty array)
        t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(dtype)
        return t
    d_ptr = [dev(p, torch.int32) for p in csc.indptr]
    d_idx = [dev(i, torch.int32) for i in csc.indices]
    d_cnt = None if case.count is None else torch.from_numpy(case.count).to("cuda")
    d_len = None if case.eff_len is None else torch.from_numpy(np.ascontiguousarray(case.eff_len, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    for flags in (0, CSC):
        eng = EmEngine.from_device(case.R, case.L, case.H, [t.data_ptr() for t in d_ptr], [t.data_ptr() for t in d_idx],
                                   None if d_cnt is None else d_cnt.data_ptr(), None if d_len is None else d_len.data_ptr(),
                                   flags=flags, allowed=case.allowed)
        assert eng.info().num_entries == tc.exact_of(case).num_entries
        if case.no_entries:
            eng.prepare(0.0)
            assert not eng.theta().any()
            with pytest.raises(FloatingPointError):
                eng.step(1)
        else:
            if flags == case.home_flags and eng.info().layout == 1:
                check_facts(eng, case, "from_device")
            check_run(eng, case, f"from_device_flags{flags}")
        eng.close()


# ---- the `-G` mask carried out by the device and by the host ----------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, CSC, DETERMINISTIC | MERGE])
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.allowed is not None])
def test_masked_create_on_host_and_on_device(name, flags, monkeypatch):
    case = CASES[name]
    res = []
    for where in ("device", "host"):
        eng = create(case, flags, {}, monkeypatch, masked_on=where)
        assert eng.info().num_entries == tc.exact_of(case).num_entries
        if case.no_entries:
            eng.prepare(0.0)
            res.append((eng.theta(), eng.theta()))
            assert not res[-1][0].any()
            with pytest.raises(FloatingPointError):
                eng.step(1)
        else:
            check_run(eng, case, f"mask_on_{where}_flags{flags}")
            res.append((eng.theta(), eng.expected_counts()))
        eng.close()
    if flags & DETERMINISTIC:
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- read-level posterior ---------------------------------------------------------------------------------------------------

def make_apm(case, groups=None):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    csc = arrays_of(case)
    apm = AlignmentPropertyMatrix(shape=(case.L, case.H, case.R), indptr=csc.indptr, indices=csc.indices, count=case.count,
                                  haplotype_names=[f"H{h}" for h in range(case.H)],
                                  locus_names=[f"T{l:07d}" for l in range(case.L)])
    if groups is not None:
        apm.groups = groups
        apm.gname = np.array([f"G{i:07d}" for i in range(len(groups))])
        apm.num_groups = len(groups)
    return apm


POSTERIOR = [f"sweep_h{H}" for H in (1, 6, 11, 16, 32)] + ["sweep_h11_counts", "only_a_long_row_h8", "only_a_long_row_h16",
                                                          "only_a_long_row_h11"]


@pytest.mark.parametrize("name", POSTERIOR)
def test_posterior_of_every_haplotype(name):
    """gbrs_em_posterior after three steps: every stored entry of every haplotype against em_exact."""
    from gbrs_amd.em import EMfactory
    case = CASES[name]
    want = tc.expected_of(case)
    csc = arrays_of(case)
    em = EMfactory(make_apm(case), keep_posterior=True)
    em.target_lengths = case.eff_len
    em.prepare(pseudocount=0.0)
    for _ in range(tc.STEPS):
        em.update_allelic_expression(model=4)
    close(em.allelic_expression, want.theta[-1])
    worst, per_read = 0.0, np.zeros(case.R)
    for h in range(case.H):
        rows = csc.indices[h].astype(np.int64)
        loci = np.repeat(np.arange(case.L), np.diff(csc.indptr[h].astype(np.int64)))
        ref = np.array([want.posterior[(int(r), int(l), h)] for r, l in zip(rows, loci)])
        got = em.posterior(h)
        assert got.shape == ref.shape and got.dtype == np.float64
        if len(ref):
            worst = max(worst, deviation(got, ref))
        close(got, ref)
        np.add.at(per_read, rows, got)
    print(f"POSTERIOR_DEVIATION {name} H={case.H} {worst:.3e}")
    aligned = [r for r, _ in case.rows]
    np.testing.assert_allclose(per_read[aligned], 1.0, rtol=1e-12)
    em.close()


# ---- multiread models 1-3 ---------------------------------------------------------------------------------------------------

SWEEP_GROUPS = [[5], [l for l in range(tc.SWEEP_L) if l not in (5, 20)]]       # locus 20 is in no gene, the third one


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("name", ["sweep_h3", "sweep_h6", "sweep_h13", "sweep_h13_counts"])
def test_models_1_to_3_with_groups(name, model):
    """Genes of one locus, of all the others but one, and a locus in no gene, against tests/em_models_restate.py at the
    tolerances of tests/test_em_models_gpu.py (1e-9 / 1e-300; err history 1e-7)."""
    from gbrs_amd.em import EMfactory
    case = CASES[name]
    csc = arrays_of(case)
    cpu = ModelsEM(case.R, case.L, case.H, csc.indptr, csc.indices, case.count, case.eff_len, SWEEP_GROUPS)
    assert cpu.n_genes == 3
    em = EMfactory(make_apm(case, SWEEP_GROUPS), grouped_models=True)
    em.target_lengths = case.eff_len
    em.prepare(pseudocount=0.0)
    theta = np.array(tc.expected_of(case).theta0)
    close(em.allelic_expression, theta)
    step_theta = theta
    for _ in range(2):
        em.update_allelic_expression(model)
        step_theta, counts = cpu.step(step_theta, model)
        close(em.allelic_expression, step_theta)
        close(em.expected_read_counts(), counts)
    ref_theta, ref_counts, ref_hist = cpu.run(theta, model, 0.0, 3)
    em.prepare(pseudocount=0.0)
    em.run(model=model, tol=0.0, max_iters=3, verbose=False)
    assert em.num_iters == 3
    np.testing.assert_allclose(em.err_history, ref_hist, rtol=1e-7)
    close(em.allelic_expression, ref_theta)
    close(em.expected_read_counts(), ref_counts)
    close(em.get_allelic_expression(at_group_level=True), cpu.group_sums(ref_theta, SWEEP_GROUPS))
    em.close()
