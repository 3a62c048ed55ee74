"""Multiread models 1-3 on the device (gbrs_em_set_groups / gbrs_em_step_model / gbrs_em_run) against the emmodel_*.npz
fixtures made by running the reference, and against the closed-form restatement (needs an MI355X)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_files, load_golden
from em_models_restate import ModelsEM, fixture_inputs

pytestmark = pytest.mark.gpu

RTOL = 1e-9
FIXTURES = golden_files("emmodel")
IDS = [p.split("/")[-1][:-4] for p in FIXTURES]
LAYOUTS = {"tiles": dict(), "csc": dict(csc_layout=True), "tiles_merged": dict(merge_identical_rows=True)}


def close(a, b, rtol=RTOL):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)


def pack_mask(gtmask):
    H = gtmask.shape[0]
    return ((gtmask != 0).astype(np.uint32) << np.arange(H, dtype=np.uint32)[:, None]).sum(axis=0).astype(np.uint32)


def make_apm(g, with_groups=True):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=[chr(65 + h) for h in range(H)],
                                  locus_names=[f"T{l:07d}" for l in range(L)], values=values)
    if with_groups:
        apm.groups = groups
        apm.gname = np.array([f"G{i:07d}" for i in range(len(groups))])
        apm.num_groups = len(groups)
    if gtmask is not None:
        apm.set_haplotype_mask(pack_mask(gtmask))
    return apm


def make_factory(g, layout="tiles", grouped=True, **kw):
    from gbrs_amd.em import EMfactory
    em = EMfactory(make_apm(g), grouped_models=grouped, **LAYOUTS[layout], **kw)
    em.target_lengths = fixture_inputs(g)[6]
    em.prepare(pseudocount=float(g["pseudocount"]))
    return em


def restatement(g):
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    return ModelsEM(R, L, H, indptr, indices, count, eff_len, groups, gtmask)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_models_match_reference_fixture(path, layout):
    g = load_golden(path)
    model = int(g["model"])
    em = make_factory(g, layout)
    close(em.allelic_expression, g["theta0"])
    # single steps through update_allelic_expression
    for k in range(1, 6):
        em.update_allelic_expression(model)
        if f"theta_iter{k}" in g:
            close(em.allelic_expression, g[f"theta_iter{k}"])
    # the device loop with the stopping rule, from a fresh prepare
    em.prepare(pseudocount=float(g["pseudocount"]))
    em.run(model=model, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    np.testing.assert_allclose(em.err_history, g["err_history"], rtol=1e-7)
    close(em.allelic_expression, g["theta_final"])
    close(em.expected_read_counts(), g["expected_counts"])
    close(em.get_allelic_expression(at_group_level=True), g["gene_theta"])
    close(em._group_sums(1), g["gene_counts"])
    em.close()


@pytest.mark.parametrize("path", [p for p in FIXTURES if "h8_len" in p], ids=lambda p: p.split("/")[-1][:-4])
def test_rebuild_route(path):
    """A handle built without GBRS_EM_GROUPED_MODELS is rebuilt once at the first model 1-3 call, theta carried over."""
    from gbrs_amd import _lib
    g = load_golden(path)
    model = int(g["model"])
    em = make_factory(g, grouped=False)
    assert not em.flags & _lib.GBRS_EM_GROUPED_MODELS
    em.update_allelic_expression(model)
    assert em.flags & _lib.GBRS_EM_GROUPED_MODELS
    close(em.allelic_expression, g["theta_iter1"])
    em.prepare(pseudocount=float(g["pseudocount"]))
    em.run(model=model, tol=float(g["tol"]), max_iters=int(g["max_iters"]), verbose=False)
    assert em.num_iters == int(g["num_iters"])
    close(em.allelic_expression, g["theta_final"])
    em.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_mixed_models_on_one_handle(layout):
    g = load_golden([p for p in FIXTURES if p.endswith("emmodel_m1_h8_len.npz")][0])
    cpu = restatement(g)
    em = make_factory(g, layout)
    theta = g["theta0"].copy()
    for model in (1, 4, 2, 3, 4, 1, 3, 2, 4):
        em.update_allelic_expression(model)
        theta, counts = cpu.step(theta, model)
        close(em.allelic_expression, theta)
        close(em.expected_read_counts(), counts)
    em.close()


@pytest.mark.parametrize("model", [1, 2, 3])
def test_zero_theta_column_is_not_an_error(model):
    """An entry whose theta is exactly 0 takes no part (the reference eliminates zeros first); no FloatingPointError."""
    g = load_golden([p for p in FIXTURES if p.endswith("emmodel_m1_h8_len.npz")][0])
    cpu = restatement(g)
    em = make_factory(g)
    theta = g["theta0"].copy()
    busiest = np.bincount(cpu.l, minlength=cpu.L).argmax()
    theta[:, busiest] = 0.0                 # a whole locus
    theta[3, np.bincount(cpu.l[cpu.h == 3], minlength=cpu.L).argmax()] = 0.0     # and one (h, l) column
    em.allelic_expression = theta
    for _ in range(3):
        em.update_allelic_expression(model)
        theta, counts = cpu.step(theta, model)
        close(em.allelic_expression, theta)
    assert (em.allelic_expression[:, busiest] == 0.0).all()
    em.close()


def _raw_handle(g, flags):
    from gbrs_amd import _lib
    lib = _lib.load()
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    h = C.c_void_p()
    _lib.check(lib.gbrs_em_create(R, L, H, _lib.ptr_table(indptr), _lib.ptr_table(indices), _lib.ptr(count),
                                  _lib.ptr(None if eff_len is None else np.ascontiguousarray(eff_len)), 0, flags,
                                  C.byref(h)))
    _lib.check(lib.gbrs_em_prepare(h, 0.0))
    return lib, h, groups


def _groups_csr(groups):
    ptr = np.concatenate(([0], np.cumsum([len(m) for m in groups]))).astype(np.int64)
    mem = np.concatenate([np.asarray(m, dtype=np.int64) for m in groups])
    return ptr, mem


def test_abi_errors():
    from gbrs_amd import _lib
    g = load_golden([p for p in FIXTURES if p.endswith("emmodel_m2_h8_len.npz")][0])
    n = C.c_int(0)
    # plain handle: models 1-3 unsupported, set_groups refused
    lib, h, groups = _raw_handle(g, 0)
    ptr, mem = _groups_csr(groups)
    assert lib.gbrs_em_run(h, 2, 0.0, 3, C.byref(n), None, 0, None) == _lib.GBRS_ERR_UNSUPPORTED
    assert lib.gbrs_em_step_model(h, 3, 1, None) == _lib.GBRS_ERR_UNSUPPORTED
    assert lib.gbrs_em_set_groups(h, len(groups), _lib.ptr(ptr), _lib.ptr(mem)) == _lib.GBRS_ERR_STATE
    assert lib.gbrs_em_step_model(h, 5, 1, None) == _lib.GBRS_ERR_INVALID
    lib.gbrs_em_destroy(h)
    # flag given, no groups yet
    lib, h, groups = _raw_handle(g, _lib.GBRS_EM_GROUPED_MODELS)
    assert lib.gbrs_em_run(h, 2, 0.0, 3, C.byref(n), None, 0, None) == _lib.GBRS_ERR_UNSUPPORTED
    assert lib.gbrs_em_step_model(h, 1, 1, None) == _lib.GBRS_ERR_UNSUPPORTED
    # overlapping groups: the message names the locus
    bad_mem = mem.copy()
    bad_mem[-1] = groups[0][0]
    assert lib.gbrs_em_set_groups(h, len(groups), _lib.ptr(ptr), _lib.ptr(bad_mem)) == _lib.GBRS_ERR_INVALID
    assert f"locus {groups[0][0]} " in lib.gbrs_last_error().decode()
    assert lib.gbrs_em_set_groups(h, len(groups), _lib.ptr(ptr), _lib.ptr(mem)) == 0
    assert lib.gbrs_em_run(h, 2, 0.0, 3, C.byref(n), None, 0, None) == 0 and n.value == 3
    lib.gbrs_em_destroy(h)
    # deterministic mode has no models 1-3
    lib, h, groups = _raw_handle(g, _lib.GBRS_EM_GROUPED_MODELS | _lib.GBRS_EM_DETERMINISTIC)
    assert lib.gbrs_em_set_groups(h, len(groups), _lib.ptr(ptr), _lib.ptr(mem)) == 0
    assert lib.gbrs_em_step_model(h, 2, 1, None) == _lib.GBRS_ERR_UNSUPPORTED
    assert lib.gbrs_em_run(h, 1, 0.0, 3, C.byref(n), None, 0, None) == _lib.GBRS_ERR_UNSUPPORTED
    assert lib.gbrs_em_step_model(h, 4, 1, None) == 0
    lib.gbrs_em_destroy(h)


def test_no_groups_error():
    from gbrs_amd.em import EMfactory
    g = load_golden(FIXTURES[0])
    em = EMfactory(make_apm(g, with_groups=False), grouped_models=True)
    em.prepare()
    for model in (1, 2, 3):
        with pytest.raises(RuntimeError, match="Group information matrix is missing.*not implemented"):
            em.run(model=model, verbose=False)
    em.close()


@pytest.mark.parametrize("layout", list(LAYOUTS) + ["tiles_deterministic"])
def test_model4_unchanged_by_groups(layout):
    """Groups on a handle leave Model 4 alone: bit-identical in the deterministic mode (the other layouts add with float
    atomics, whose order differs from run to run), the same iterations and 1e-12 elsewhere."""
    g = load_golden([p for p in FIXTURES if p.endswith("emmodel_m3_h8_mask.npz")][0])
    kw = dict(deterministic=True) if layout == "tiles_deterministic" else {}
    lay = "tiles" if layout == "tiles_deterministic" else layout
    a = make_factory(g, lay, grouped=True, **kw)
    b = make_factory(g, lay, grouped=False, **kw)
    a.run(model=4, tol=1e-4, max_iters=50, verbose=False)
    b.run(model=4, tol=1e-4, max_iters=50, verbose=False)
    assert a.num_iters == b.num_iters
    if kw:
        assert a.err_history == b.err_history
        assert np.array_equal(a.allelic_expression, b.allelic_expression)
        assert np.array_equal(a.expected_read_counts(), b.expected_read_counts())
    else:
        np.testing.assert_allclose(a.err_history, b.err_history, rtol=1e-9)
        close(a.allelic_expression, b.allelic_expression, 1e-12)
        close(a.expected_read_counts(), b.expected_read_counts(), 1e-12)
    a.close()
    b.close()


def _parse_tsv(text):
    lines = [l.split("\t") for l in text.strip().split("\n")]
    return lines[0], {l[0]: l[1:] for l in lines[1:]}


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("case,fmt", [("h8_len", "npz"), ("h8_len", "h5"), ("h8_called", "npz"), ("h8_called", "h5")])
def test_quantify_cli_models(tmp_path, model, case, fmt):
    """`gbrs quantify -M 1|2|3` end to end: the four report files match the reference's texts to 1e-9.  The h8_called
    fixture carries a called diplotype per gene (its loci in no group keep nothing, as under a genotype file): it runs
    with `-G`, i.e. genotype file -> haplotype mask -> masked create -> groups."""
    from gbrs_amd import cli
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    g = load_golden([p for p in FIXTURES if p.endswith(f"emmodel_m{model}_{case}.npz")][0])
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    hn = [chr(65 + h) for h in range(H)]
    ln = [f"T{l:07d}" for l in range(L)]
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=hn, locus_names=ln)
    aln = tmp_path / f"aln.{fmt}"
    if fmt == "h5":
        apm.save(str(aln), incidence_only=True)
    else:
        apm.save_npz(str(aln))
    grp = tmp_path / "g2t.tsv"
    with open(grp, "w") as fh:
        for i, mem in enumerate(groups):
            fh.write(f"G{i:07d}\t" + "\t".join(ln[m] for m in mem) + "\n")
    lens = tmp_path / "len.tsv"
    with open(lens, "w") as fh:
        for l in range(L):
            for h in hn:
                fh.write(f"{ln[l]}_{h}\t{int(g['raw_length'][l])}\n")
    argv = ["quantify", "-i", str(aln), "-g", str(grp), "-L", str(lens), "-o", str(tmp_path / "out"),
            "-M", str(model), "-t", str(float(g["tol"])), "-m", str(int(g["max_iters"]))]
    suffix = "multiway"
    if gtmask is not None:
        gt = tmp_path / "gt.tsv"
        with open(gt, "w") as fh:
            fh.write("#Gene_ID\tDiplotype\n")
            for i, mem in enumerate(groups):
                hs = np.flatnonzero(gtmask[:, mem[0]])
                fh.write(f"G{i:07d}\t" + "".join(hn[h] for h in (hs if len(hs) == 2 else [hs[0], hs[0]])) + "\n")
        argv += ["-G", str(gt)]
        suffix = "diploid"
    assert cli.main(argv) == 0
    for key, fname in (("text_isoforms_tpm", "isoforms.tpm"), ("text_isoforms_counts", "isoforms.expected_read_counts"),
                       ("text_genes_tpm", "genes.tpm"), ("text_genes_counts", "genes.expected_read_counts")):
        got_h, got = _parse_tsv(open(tmp_path / f"out.{suffix}.{fname}").read())
        exp_h, exp = _parse_tsv(str(g[key]))
        assert got_h[:len(exp_h)] == exp_h and list(got) == list(exp)
        if gtmask is not None:
            assert got_h[-1] == "notes"
        for k in exp:
            np.testing.assert_allclose([float(x) for x in got[k][:len(exp[k])]], [float(x) for x in exp[k]],
                                       rtol=1e-9, atol=1e-300)


# ---------------------------------------------------------------------------------------------------- at full size

@pytest.fixture(scope="module")
def c2_multi_isoform():
    """BASELINE configs[1] (40M reads x 8 haplotypes x 120k isoforms) with multi-isoform reads of up to 12 loci and
    masks that differ from locus to locus, built in HBM by the bench generator."""
    import torch
    from gbrs_amd import synth, synth_torch
    prob = synth_torch.make_em_problem_device(40_000_000, 8, 120_000, synth.SEED_BASE_EM + 1, "cuda:0",
                                              variant="multi_isoform")
    yield prob
    del prob
    torch.cuda.empty_cache()


def _shifted_groups(L, starts):
    """The test's genes: the generator's genes moved up by one locus, so that a read over a generator gene's first
    locus and another of its loci crosses genes here; every 7th left out, so that its loci are genes of their own."""
    bounds = np.minimum(np.concatenate((np.asarray(starts) + 1, [L])), L)
    spans = [(int(a), int(b)) for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])) if i % 7 != 3 and b > a]
    ptr = np.concatenate(([0], np.cumsum([b - a for a, b in spans]))).astype(np.int64)
    mem = np.concatenate([np.arange(a, b) for a, b in spans]).astype(np.int64)
    return ptr, mem


class _TorchModels:
    """The E-step of models 1-3 restated with torch segment sums over the stored entries (every theta stays > 0 on
    this sample, which the step asserts, so the segments are fixed once)."""

    def __init__(self, prob, gptr, gmem):
        import torch
        R, L, H = prob["R"], prob["L"], prob["H"]
        dev = prob["eff_len"].device
        self.R, self.L, self.H, self.eff_len = R, L, H, prob["eff_len"]
        rs, hs, ls = [], [], []
        for h in range(H):
            ip = prob["indptr"][h].long()
            ls.append(torch.repeat_interleave(torch.arange(L, device=dev), ip[1:] - ip[:-1]))
            rs.append(prob["indices"][h].long())
            hs.append(torch.full_like(rs[-1], h))
        self.r, self.h, self.l = torch.cat(rs), torch.cat(hs), torch.cat(ls)
        del rs, hs, ls
        gene = np.full(L, -1, dtype=np.int64)
        gene[gmem] = np.repeat(np.arange(len(gptr) - 1), np.diff(gptr))
        free = np.flatnonzero(gene < 0)
        gene[free] = len(gptr) - 1 + np.arange(len(free))
        Gx = self.n_genes = len(gptr) - 1 + len(free)
        self.gene = torch.from_numpy(gene).to(dev)
        self.g = self.gene[self.l]
        self.hl = self.h * L + self.l
        self.u_rg, self.i_rg = torch.unique(self.r * Gx + self.g, return_inverse=True)
        self.seg_r, self.seg_g = self.u_rg // Gx, self.u_rg % Gx
        u_rl, self.i_rl = torch.unique(self.r * L + self.l, return_inverse=True)
        self.n_rl = u_rl.numel()
        self.rl_l = u_rl % L
        self.rl_seg = torch.searchsorted(self.u_rg, (u_rl // L) * Gx + self.gene[self.rl_l])
        del u_rl
        u_rgh, self.i_rgh = torch.unique((self.r * Gx + self.g) * H + self.h, return_inverse=True)
        self.n_rgh = u_rgh.numel()
        self.rgh_seg = torch.searchsorted(self.u_rg, u_rgh // H)
        self.rgh_g, self.rgh_h = (u_rgh // H) % Gx, u_rgh % H
        del u_rgh

    def step(self, theta, model):
        import torch
        H, L, dev = self.H, self.L, theta.device
        f64 = dict(dtype=torch.float64, device=dev)
        t = theta.reshape(-1)[self.hl]
        assert bool((t > 0).all())
        Y = torch.zeros(self.n_genes, H, **f64).index_add_(0, self.gene, theta.T.contiguous())
        T, U = Y.sum(dim=1), theta.sum(dim=0)
        D = torch.zeros(self.R, **f64).index_add_(0, self.seg_r, T[self.seg_g])
        nseg = self.u_rg.numel()
        if model == 3:
            S = torch.zeros(nseg, **f64).index_add_(0, self.i_rg, t)
            f = T[self.g] / S[self.i_rg]
        elif model == 2:
            V = torch.zeros(self.n_rl, **f64).index_add_(0, self.i_rl, t)
            W = torch.zeros(nseg, **f64).index_add_(0, self.rl_seg, U[self.rl_l])
            f = U[self.l] * T[self.g] / (V[self.i_rl] * W[self.i_rg])
        else:
            X = torch.zeros(self.n_rgh, **f64).index_add_(0, self.i_rgh, t)
            Z = torch.zeros(nseg, **f64).index_add_(0, self.rgh_seg, Y[self.rgh_g, self.rgh_h])
            f = Y[self.g, self.h] * T[self.g] / (X[self.i_rgh] * Z[self.i_rg])
        A = torch.zeros(H * L, **f64).index_add_(0, self.hl, f / D[self.r]).reshape(H, L)
        counts = theta * A
        return counts / self.eff_len, counts


def test_models_full_size(c2_multi_isoform):
    """configs[1] with multi-isoform reads (581M entries): each of models 1-3 after 3 steps on the device against the
    torch restatement to 1e-9, and the expected counts add up to the number of reads."""
    import torch
    from gbrs_amd import _lib
    prob = c2_multi_isoform
    lib = _lib.load()
    R, L, H = prob["R"], prob["L"], prob["H"]
    gptr, gmem = _shifted_groups(L, prob["gene_starts"])
    h = C.c_void_p()
    _lib.check(lib.gbrs_em_create_device(R, L, H, _lib.raw_table([t.data_ptr() for t in prob["indptr"]]),
                                         _lib.raw_table([t.data_ptr() for t in prob["indices"]]), None,
                                         C.c_void_p(prob["eff_len"].data_ptr()), 0, _lib.GBRS_EM_GROUPED_MODELS,
                                         C.byref(h)))
    try:
        _lib.check(lib.gbrs_em_prepare(h, 0.0))
        _lib.check(lib.gbrs_em_set_groups(h, len(gptr) - 1, _lib.ptr(gptr), _lib.ptr(gmem)))
        theta0 = np.empty((H, L))
        _lib.check(lib.gbrs_em_get(h, _lib.ptr(theta0), None))
        ref = _TorchModels(prob, gptr, gmem)
        # the sample has what the layout must handle: rows of many entries, reads across genes, loci in no group
        rows_with_entries = int(torch.unique(ref.r).numel())
        assert ref.r.numel() > 5 * R and ref.u_rg.numel() > rows_with_entries * 1.01, (ref.r.numel(), ref.u_rg.numel())
        assert ref.n_genes > len(gptr) - 1
        for model in (1, 2, 3):
            _lib.check(lib.gbrs_em_set_theta(h, _lib.ptr(theta0)))
            _lib.check(lib.gbrs_em_step_model(h, model, 3, None))
            got, got_counts = np.empty((H, L)), np.empty((H, L))
            _lib.check(lib.gbrs_em_get(h, _lib.ptr(got), _lib.ptr(got_counts)))
            theta = torch.from_numpy(theta0).to(prob["eff_len"].device)
            for _ in range(3):
                theta, counts = ref.step(theta, model)
            close(got, theta.cpu().numpy())
            close(got_counts, counts.cpu().numpy())
            assert abs(got_counts.sum() - R) <= 1e-9 * R, (model, got_counts.sum())
            del theta, counts
        del ref
    finally:
        lib.gbrs_em_destroy(h)
        torch.cuda.empty_cache()
