"""Read-level posteriors on the device (GBRS_EM_POSTERIOR, gbrs_em_posterior, `gbrs quantify -w --posterior-values`)
against the posterior_*.npz fixtures made by running the reference, and against the closed form of
tests/posterior_restate.py (needs an MI355X)."""
import os

import numpy as np
import pytest

from conftest import em_case_inputs, em_case_values, golden_files, load_golden
from em_models_restate import ModelsEM, fixture_inputs
from posterior_restate import masked_structure, posterior

pytestmark = pytest.mark.gpu

# the tolerances the project holds the expected counts to (tests/test_em_models_gpu.py:19-20)
RTOL = 1e-9
GOLD = os.path.dirname(golden_files("posterior")[0]) if golden_files("posterior") else ""
CASES = [os.path.basename(p)[len("posterior_"):-4] for p in golden_files("posterior")]
# the device layouts of test_em_gpu.py the EM of a model-4 run may be on; the posterior must not depend on them
LAYOUTS = {"tiles": (dict(), {}), "csc": (dict(csc_layout=True), {}),
           "tiles_locus_sets_forced": (dict(), {"GBRS_TUNING_LOCUS_SETS": "1"}),
           "tiles_deterministic": (dict(deterministic=True), {})}


def close(a, b, rtol=RTOL):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def pack_mask(gtmask):
    H = gtmask.shape[0]
    return ((gtmask != 0).astype(np.uint32) << np.arange(H, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32)


_inputs = {}


def case_inputs(case):
    """The inputs of a posterior_<case>.npz fixture (those of emmodel_m1_<case>.npz) and its values, loaded once."""
    if case not in _inputs:
        _inputs[case] = (load_golden(os.path.join(GOLD, f"emmodel_m1_{case}.npz")),
                         load_golden(os.path.join(GOLD, f"posterior_{case}.npz")))
    return _inputs[case]


def make_apm(inputs, indices=None):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    R, L, H, indptr, idx, count, eff_len, groups, gtmask, values = inputs
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=idx if indices is None else indices,
                                  count=count, haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)], values=values)
    apm.groups = groups
    apm.gname = np.array([f"G{i:07d}" for i in range(len(groups))])
    apm.num_groups = len(groups)
    if gtmask is not None:
        apm.set_haplotype_mask(pack_mask(gtmask))
    return apm


def make_factory(inputs, pseudocount=0.0, indices=None, keep_posterior=True, **kw):
    from gbrs_amd.em import EMfactory
    em = EMfactory(make_apm(inputs, indices), grouped_models=True, keep_posterior=keep_posterior, **kw)
    em.target_lengths = inputs[6]
    em.prepare(pseudocount=pseudocount)
    return em


def restatement(inputs):
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = inputs
    return ModelsEM(R, L, H, indptr, indices, count, eff_len, groups, gtmask)


# ------------------------------------------------------------------------------------------ 1. parity with the reference

@pytest.mark.parametrize("model", [1, 2, 3, 4])
@pytest.mark.parametrize("case", CASES)
def test_posterior_matches_reference_fixture(case, model, monkeypatch):
    g, post = case_inputs(case)
    inputs = fixture_inputs(g)
    H, L = inputs[2], inputs[1]
    m_ptr, m_idx = masked_structure(L, H, inputs[3], inputs[4], inputs[8])
    for name, (kw, env) in LAYOUTS.items():
        if model != 4 and name != "tiles":
            continue                       # models 1-3 step on the grouped layout, whatever model 4 runs on
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            em = make_factory(inputs, float(g["pseudocount"]), **kw)
        em.run(model=model, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
        assert em.num_iters == int(post[f"m{model}_num_iters"]), name
        for h in range(H):
            got = em.posterior(h)
            assert got.dtype == np.float64 and got.shape == (len(m_idx[h]),), (name, h)
            close(got, post[f"m{model}_post{h}"])
        if model == 4:
            close(em.allelic_expression, post["m4_theta_final"])
            close(em.expected_read_counts(), post["m4_expected_counts"])
        em.close()


# ------------------------------------------------------------------------------------------ 2. invariants on the existing goldens

def _check_invariants(em, R, L, H, indptr, indices, count, gtmask, expected_counts):
    m_ptr, m_idx = masked_structure(L, H, indptr, indices, gtmask)
    cnt = np.ones(R) if count is None else np.asarray(count, dtype=np.float64)
    per_read, touched = np.zeros(R), np.zeros(R, dtype=bool)
    got_counts = np.zeros((H, L))
    for h in range(H):
        p = em.posterior(h)
        rows = m_idx[h].astype(np.int64)
        col = np.repeat(np.arange(L), np.diff(m_ptr[h].astype(np.int64)))
        assert p.shape == rows.shape
        np.add.at(got_counts[h], col, cnt[rows] * p)
        np.add.at(per_read, rows, p)
        touched[rows] = True
    close(got_counts, expected_counts)
    close(per_read[touched], np.ones(int(touched.sum())))


@pytest.mark.parametrize("path", golden_files("em"), ids=lambda p: os.path.basename(p)[:-4])
def test_invariants_model4_goldens(path):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.em import EMfactory
    g = load_golden(path)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=[f"H{h}" for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)], values=em_case_values(g))
    if gtmask is not None:
        apm.set_haplotype_mask(pack_mask(gtmask))
    em = EMfactory(apm, keep_posterior=True)
    em.target_lengths = eff_len
    em.prepare(pseudocount=float(g["pseudocount"]))
    em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    _check_invariants(em, R, L, H, indptr, indices, count, gtmask, g["expected_counts"])
    em.close()


@pytest.mark.parametrize("path", golden_files("emmodel"), ids=lambda p: os.path.basename(p)[:-4])
def test_invariants_model_goldens(path):
    g = load_golden(path)
    inputs = fixture_inputs(g)
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = inputs
    em = make_factory(inputs, float(g["pseudocount"]))
    em.run(model=int(g["model"]), tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    _check_invariants(em, R, L, H, indptr, indices, count, gtmask, g["expected_counts"])
    em.close()


# ------------------------------------------------------------------------------------------ 3. step by step

@pytest.mark.parametrize("model", [1, 2, 3, 4])
@pytest.mark.parametrize("case", ["h8_len", "h1_len"])
def test_posterior_step_by_step(case, model):
    g, _ = case_inputs(case)
    inputs = fixture_inputs(g)
    cpu = restatement(inputs)
    for k in (1, 3):
        em = make_factory(inputs, float(g["pseudocount"]))
        for _ in range(k - 1):
            em.update_allelic_expression(model)
        before = em.allelic_expression.copy()              # theta the k-th step starts from
        em.update_allelic_expression(model)
        want = posterior(cpu, before, model)
        for h in range(inputs[2]):
            close(em.posterior(h), want[h])
        em.close()


# ------------------------------------------------------------------------------------------ 4. zero theta

@pytest.mark.parametrize("model", [4, 3])
def test_zero_theta_column_is_exactly_zero(model):
    g, _ = case_inputs("h8_len")
    inputs = fixture_inputs(g)
    R, L, H = inputs[:3]
    cpu = restatement(inputs)
    per_read = np.bincount(cpu.r, minlength=R)
    # a column all of whose reads have another entry (its theta stays positive: prepare leaves no zero on an entry)
    col_min = np.full((H, L), np.iinfo(np.int64).max)
    np.minimum.at(col_min, (cpu.h, cpu.l), per_read[cpu.r])
    width = np.zeros((H, L), dtype=np.int64)
    np.add.at(width, (cpu.h, cpu.l), 1)
    h0, l0 = map(int, np.argwhere((width >= 5) & (col_min >= 2))[0])
    em = make_factory(inputs, float(g["pseudocount"]))
    theta = em.allelic_expression.copy()
    assert (theta[cpu.h, cpu.l] > 0).all()
    theta[h0, l0] = 0.0
    em.allelic_expression = theta
    em.update_allelic_expression(model)
    want = posterior(cpu, theta, model)
    ptr = masked_structure(L, H, inputs[3], inputs[4], inputs[8])[0]
    for h in range(H):
        got = em.posterior(h)
        close(got, want[h])
        if h == h0:
            a, b = int(ptr[h][l0]), int(ptr[h][l0 + 1])
            assert b - a >= 5 and (got[a:b] == 0.0).all() and not np.signbit(got[a:b]).any()
            assert (np.delete(got, np.arange(a, b)) > 0.0).all()
    em.close()


# ------------------------------------------------------------------------------------------ 5. order inside a column

@pytest.mark.parametrize("model", [4, 2])
def test_order_inside_a_column_is_the_callers(model):
    g, post = case_inputs("h8_mask")
    inputs = fixture_inputs(g)
    R, L, H, indptr, indices = inputs[:5]
    rng = np.random.default_rng(5)
    perm, shuffled = [], []
    for h in range(H):
        p = np.arange(len(indices[h]))
        for l in range(L):
            a, b = int(indptr[h][l]), int(indptr[h][l + 1])
            p[a:b] = a + rng.permutation(b - a)
        perm.append(p)
        shuffled.append(np.ascontiguousarray(indices[h][p]))
    assert any((p != np.arange(len(p))).any() for p in perm)
    # positions of the masked arrays: the mask drops whole columns, the order inside the kept ones stays
    keep = []
    for h in range(H):
        width = np.diff(indptr[h].astype(np.int64))
        keep.append(np.repeat(inputs[8][h] != 0, width))
    em = make_factory(inputs, float(g["pseudocount"]), indices=shuffled)
    em.run(model=model, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(post[f"m{model}_num_iters"])
    for h in range(H):
        full = np.full(len(indices[h]), np.nan)
        full[keep[h]] = post[f"m{model}_post{h}"]            # the fixture's values at the unmasked positions
        close(em.posterior(h), full[perm[h]][keep[h]])       # (a column is kept or dropped as a whole)
    em.close()


# ------------------------------------------------------------------------------------------ 6. block and column boundaries

@pytest.fixture(scope="module")
def boundary_case():
    """100,000 reads x 8 haplotypes x 300 loci: one locus carries about half of all entries (each of its columns is far
    longer than a workgroup's 256 entries), 25 loci have no entry at all, 1,500 reads have none, counts given, and a
    `-G`-style mask that drops columns."""
    R, H, L, hot = 100_000, 8, 300, 137
    rng = np.random.default_rng(6)
    with_entries = rng.permutation(R)[:R - 1500]
    empty_loci = rng.choice(np.setdiff1d(np.arange(L), [hot]), size=25, replace=False)
    others = np.setdiff1d(np.arange(L), np.concatenate(([hot], empty_loci)))
    u = rng.random(len(with_entries))
    on_hot = u < 0.8
    on_other = ~on_hot | (rng.random(len(with_entries)) < 0.75)
    rr = np.concatenate((with_entries[on_hot], with_entries[on_other]))
    ll = np.concatenate((np.full(int(on_hot.sum()), hot), rng.choice(others, size=int(on_other.sum()))))
    m = rng.random((len(rr), H)) < 0.6
    m[np.arange(len(rr)), rng.integers(0, H, size=len(rr))] = True
    indptr, indices = [], []
    for h in range(H):
        sel = m[:, h]
        order = np.lexsort((rng.random(int(sel.sum())), ll[sel]))          # rows in no particular order inside a column
        indptr.append(np.searchsorted(ll[sel][order], np.arange(L + 1)).astype(np.uint32))
        indices.append(rr[sel][order].astype(np.uint32))
    nnz = sum(len(i) for i in indices)
    hot_share = sum(int(p[hot + 1]) - int(p[hot]) for p in indptr) / nnz
    assert 0.4 < hot_share < 0.6 and min(int(p[hot + 1]) - int(p[hot]) for p in indptr) > 10_000
    assert sum(int(np.sum(np.diff(p.astype(np.int64)) == 0)) for p in indptr) >= 20
    assert R - len(np.unique(rr)) >= 1000
    count = rng.integers(1, 6, size=R).astype(np.float64)
    eff_len = np.maximum(np.round(rng.lognormal(6.5, 0.5, size=L)) - 99, 1.0)[None, :].repeat(H, 0)
    bounds = np.arange(0, L - 20, 3)                                   # genes of 3 loci, the last 20 loci in none
    groups = [list(range(int(a), int(a) + 3)) for a in bounds[:-1]]
    gtmask = (rng.random((H, L)) < 0.7).astype(np.float64)
    gtmask[:, hot] = 1.0
    gtmask[2, hot] = 0.0                                               # a long column goes too
    inputs = (R, L, H, indptr, indices, count, eff_len, groups, gtmask, None)
    return inputs, restatement(inputs)


@pytest.mark.parametrize("model", [4, 3])
def test_block_and_column_boundaries(boundary_case, model):
    inputs, cpu = boundary_case
    R, L, H = inputs[:3]
    em = make_factory(inputs)
    for _ in range(2):
        em.update_allelic_expression(model)
    before = em.allelic_expression.copy()
    em.update_allelic_expression(model)
    want = posterior(cpu, before, model)
    m_idx = masked_structure(L, H, inputs[3], inputs[4], inputs[8])[1]
    for h in range(H):
        got = em.posterior(h)
        assert got.shape == (len(m_idx[h]),)
        close(got, want[h])
    em.close()


# ------------------------------------------------------------------------------------------ 7. state and argument errors

def test_state_and_argument_errors():
    from gbrs_amd import _lib
    g, _ = case_inputs("h8_len")
    inputs = fixture_inputs(g)
    em = make_factory(inputs, keep_posterior=False)
    em.update_allelic_expression(4)
    with pytest.raises(RuntimeError, match="GBRS_EM_POSTERIOR"):
        em.posterior(0)
    out = np.zeros(len(inputs[4][0]))
    assert _lib.load().gbrs_em_posterior(em._h, 0, _lib.ptr(out), len(out)) == _lib.GBRS_ERR_STATE
    em.close()
    em = make_factory(inputs)
    with pytest.raises(RuntimeError, match="no EM step"):
        em.posterior(0)
    assert _lib.load().gbrs_em_posterior(em._h, 0, _lib.ptr(out), len(out)) == _lib.GBRS_ERR_STATE
    em.update_allelic_expression(4)
    assert em.posterior(0).shape == out.shape
    with pytest.raises(RuntimeError):
        em.posterior(inputs[2])
    lib = _lib.load()
    assert lib.gbrs_em_posterior(em._h, inputs[2], _lib.ptr(out), len(out)) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_em_posterior(em._h, 0, _lib.ptr(out), len(out) - 1) == _lib.GBRS_ERR_INVALID
    assert lib.gbrs_em_posterior(em._h, 0, _lib.ptr(out), len(out)) == 0
    em.prepare()                                            # a new prepare: the posterior of the old run is gone
    with pytest.raises(RuntimeError, match="no EM step"):
        em.posterior(0)
    em.close()


# ------------------------------------------------------------------------------------------ 8. the flag changes nothing else

def test_flag_leaves_the_em_alone():
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.em import EMfactory
    g = load_golden(os.path.join(os.path.dirname(golden_files("em")[0]), "em_h8_count_len.npz"))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    res = []
    for keep in (False, True):
        apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                      haplotype_names=[chr(65 + h) for h in range(H)],
                                      locus_names=[f"T{l:07d}" for l in range(L)], values=em_case_values(g))
        if gtmask is not None:
            apm.set_haplotype_mask(pack_mask(gtmask))
        em = EMfactory(apm, deterministic=True, keep_posterior=keep)
        em.target_lengths = eff_len
        em.prepare(pseudocount=float(g["pseudocount"]))
        em.run(model=4, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
        res.append((em.num_iters, em.allelic_expression.copy(), em.expected_read_counts(), list(em.err_history)))
        em.close()
    assert res[0][0] == res[1][0] == int(g["num_iters"])
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3]


# ------------------------------------------------------------------------------------------ 9. the command

def _h5_has_data(path):
    """(incidence_only attribute, whether /h0/data exists) of an EMASE .h5 file."""
    from gbrs_amd import emase_h5 as e
    lib = e._load()
    f = lib.H5Fopen(os.fsencode(path), e.H5F_ACC_RDONLY, e.H5P_DEFAULT)
    assert f >= 0
    try:
        root = lib.H5Gopen2(f, b'/', e.H5P_DEFAULT)
        inc = e._as_bool(e._read_attr(root, 'incidence_only'))
        g0 = lib.H5Gopen2(f, b'/h0', e.H5P_DEFAULT)
        has = lib.H5Lexists(g0, b'data', e.H5P_DEFAULT) > 0
        lib.H5Gclose(g0)
        lib.H5Gclose(root)
        return inc, has
    finally:
        lib.H5Fclose(f)


def _command_inputs(tmp_path):
    """h8_mask's input as an .h5 with group, length and genotype files that give the fixture's mask; returns the
    argv shared by the test's commands and what the outputs are compared with."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    g, post = case_inputs("h8_mask")
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    hn = [chr(65 + h) for h in range(H)]
    ln = [f"T{l:07d}" for l in range(L)]
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=hn, locus_names=ln)
    aln = tmp_path / "aln.h5"
    apm.save(str(aln), incidence_only=True)
    # the fixture's mask calls a pair for every gene and for every locus in no gene: a genotype file can only call
    # genes, so the group file of this command lists those loci as genes of their own (model 4 looks at no group)
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
    common = ["quantify", "-i", str(aln), "-g", str(grp), "-L", str(lens), "-G", str(gt),
              "-t", str(float(g["tol"])), "-m", str(int(g["max_iters"]))]
    m_ptr, m_idx = masked_structure(L, H, indptr, indices, gtmask)
    return common, (L, H, R), m_ptr, m_idx, post


REPORTS = ("isoforms.tpm", "isoforms.expected_read_counts", "genes.tpm", "genes.expected_read_counts")


def _same_tables(a, b):
    """Two report files: the same lines, names and notes, every number within the project's 1e-9."""
    la, lb = a.decode().split("\n"), b.decode().split("\n")
    assert len(la) == len(lb) and la[0] == lb[0]
    for x, y in zip(la[1:], lb[1:]):
        fx, fy = x.split("\t"), y.split("\t")
        assert len(fx) == len(fy)
        for u, v in zip(fx, fy):
            try:
                u, v = float(u), float(v)
            except ValueError:
                assert u == v
            else:
                close(u, v)


def test_quantify_command_writes_posterior_values(tmp_path, monkeypatch):
    """`gbrs quantify -G ... -w --posterior-values` end to end.

    The reports are compared byte for byte with those of the same command without the option on the bit-reproducible
    E-step (GBRS_EM_DETERMINISTIC, which the test switches on for both commands).  On the default layout the command
    is not byte-reproducible against itself - the tiles add with LDS float atomics, whose order differs from run to
    run: five runs of the unchanged `-w` command on this input left five different sets of report files, differing in
    the last printed digit - so there the two commands' reports are held to the 1e-9 every other report test uses."""
    from gbrs_amd import cli, quantify as quantify_module
    from gbrs_amd.alignment import load_alignment
    from gbrs_amd.em import EMfactory
    common, (L, H, R), m_ptr, m_idx, post = _command_inputs(tmp_path)
    assert cli.main(common + ["-o", str(tmp_path / "val"), "-w", "--posterior-values"]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "inc"), "-w"]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "imp"), "--posterior-values"]) == 0      # the option implies -w
    with monkeypatch.context() as mp:
        mp.setattr(quantify_module, "EMfactory", lambda *a, **kw: EMfactory(*a, deterministic=True, **kw))
        assert cli.main(common + ["-o", str(tmp_path / "detval"), "-w", "--posterior-values"]) == 0
        assert cli.main(common + ["-o", str(tmp_path / "detinc"), "-w"]) == 0
    for base in ("val", "imp", "detval"):
        path = str(tmp_path / f"{base}.diploid.posterior.h5")
        assert _h5_has_data(path) == (False, True)
        got = load_alignment(path)
        assert got.shape == (L, H, R) and got.values is not None
        for h in range(H):
            assert np.array_equal(got.indptr[h], m_ptr[h]) and np.array_equal(got.indices[h], m_idx[h])
            close(got.values[h], post[f"m4_post{h}"])
    # -w alone: the structure, as before
    for base in ("inc", "detinc"):
        inc_path = str(tmp_path / f"{base}.diploid.posterior.h5")
        assert _h5_has_data(inc_path) == (True, False)
        inc = load_alignment(inc_path)
        assert inc.values is None
        for h in range(H):
            assert np.array_equal(inc.indptr[h], m_ptr[h]) and np.array_equal(inc.indices[h], m_idx[h])
    # the reports do not know about the option
    for name in REPORTS:
        a = open(tmp_path / f"detval.diploid.{name}", "rb").read()
        assert len(a) > 0 and a == open(tmp_path / f"detinc.diploid.{name}", "rb").read(), name
        _same_tables(open(tmp_path / f"val.diploid.{name}", "rb").read(),
                     open(tmp_path / f"inc.diploid.{name}", "rb").read())
