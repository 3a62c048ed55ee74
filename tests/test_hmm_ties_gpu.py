"""Viterbi calls on exact ties and on decisions inside the rounding of delta, on every route of the HIP HMM (needs an
MI355X).

Tier A hands the device the reference's (or the oracle's) emissions, so that it does nothing but max(delta + T) + e and
the argmax rules: the calls must be the reference's, ties included.  Tier B lets the device compute the emissions: a
decision that the reference takes inside the rounding of its own emission may then fall on another of the tied
candidates, and on no other state.  Tier C compares the blocked scan with the unblocked chain at size."""
import functools
import os

import numpy as np
import pytest

import hmm_ties
from conftest import golden_files, hmm_case_inputs, load_golden

pytestmark = pytest.mark.gpu

TIE_FILES = golden_files("hmmtie")
H8_FILES = [p for p in TIE_FILES if "_h8_" in p]
fid = lambda p: "class_constant" if p == "cc" else p.split("/")[-1][:-4]      # noqa: E731
WANT = ("gamma", "states", "calls", "alpha", "beta", "delta", "scaler")

# one-sample routes of the 36-state pass, selected as tests/test_hmm_gpu.py selects them.  The unblocked chain is adds and
# max in the reference's order: its delta is the reference's bit for bit.  The blocked routes store "true delta minus one
# constant per block" and add the constants back - another association, not bit-exact by design: 1e-9.
BLK = "GBRS_TUNING_HMM_"
ROUTES = {"unblocked": {BLK + "BLOCKED": "0"}, "defaults": {}}
for _bg in ("5", "9"):
    _on = {BLK + "BLOCKED": "2", BLK + "BLOCK_GENES": _bg}
    ROUTES["rank-" + _bg] = dict(_on)
    ROUTES["operators-" + _bg] = dict(_on, **{BLK + "DELTA_SPEC": "0"})
    ROUTES["fallback-" + _bg] = dict(_on, **{BLK + "DELTA_TOL": "-1"})
PLAIN_CHAINS = {"unblocked"}
# batches: MFMA sweeps from 16 samples, the samples-on-lanes delta chain from 16, the samples-on-lanes backpointers from 5.
# Their delta chains (one wave per sample below 16 samples, samples on lanes from there) are plain chains.
BATCH = {BLK + "MFMA": "16", BLK + "DLANES": "16", BLK + "BPLANES": "5"}
# and with the library's defaults, 25 and 40 samples (mfma_ng = 0 in the batch tests' rows): the two-samples-per-wave chains
# (tests/hmm_batched_cases.py), the same template as the one-sample-per-wave chain and as plain.  The tie samples sit in a
# wave's first slot (0, 16), in its second slot (15, 39) and alone in the last wave (24).
BATCH_ROWS = [(5, 1), (21, 1), (21, 2), (37, 1), (37, 2), pytest.param(25, 0, id="25-defaults"), pytest.param(40, 0, id="40-defaults")]


def set_route(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def set_batch_route(monkeypatch, mfma_ng):
    if mfma_ng:
        set_route(monkeypatch, dict(BATCH, **{BLK + "MFMA_NG": str(mfma_ng)}))
        return
    for k in list(os.environ):
        if k.startswith((BLK, "GBRS_DIAG_HMM_")):
            monkeypatch.delenv(k, raising=False)


def oracle_sample(H, tables, eprobs):
    """Per chromosome, everything the reference computes from log emissions [n, S]."""
    from oracle import hmm_oracle as o
    iv = o.init_vector(H)
    out = []
    for T, E in zip(tables, eprobs):
        alpha, scaler = o.forward(T, E, iv)
        beta = o.backward(T, E, scaler)
        delta, states, calls = o.viterbi(T, E, iv)
        out.append(dict(eprob=E, alpha=alpha, scaler=scaler, beta=beta, gamma=o.posterior(alpha, beta), delta=delta,
                        states=states, calls=calls))
    return out


def fixture_sample(g, chroms):
    return [{k: g[f"{k}_{ch}"] for k in ("eprob",) + WANT} for ch in chroms]


def make_hmm(H, tables, n_genes):
    from gbrs_amd.hmm import DiplotypeHMM
    return DiplotypeHMM(H, [f"c{k}" for k in range(len(tables))], n_genes, tables)


def check_numbers(r, ref, exact_delta, msg):
    for k in ("alpha", "beta", "scaler"):
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-9, atol=1e-9, err_msg=f"{k} {msg}")
    if exact_delta:
        np.testing.assert_array_equal(r["delta"], ref["delta"], err_msg=f"delta {msg}")
    else:
        np.testing.assert_allclose(r["delta"], ref["delta"], rtol=1e-9, atol=1e-9, err_msg=f"delta {msg}")
    np.testing.assert_allclose(r["gamma"], ref["gamma"], rtol=1e-8, atol=1e-300, err_msg=f"gamma {msg}")


def check_exact(hmm, sample, expected, exact_delta, msg):
    """Tier A: path and calls are the reference's, ties included."""
    for ci, ref in enumerate(expected):
        r = hmm.get(ci, sample=sample, want=WANT)
        np.testing.assert_array_equal(r["states"], ref["states"], err_msg=f"states {msg} chromosome {ci}")
        np.testing.assert_array_equal(r["calls"], ref["calls"], err_msg=f"calls {msg} chromosome {ci}")
        check_numbers(r, ref, exact_delta, f"{msg} chromosome {ci}")


def check_eps_optimal(hmm, sample, tables, expected, msg, outright=False):
    """Tier B: the device's own emissions.  Every step of its path is a best candidate of the reference's delta to
    within the slack, at most 5 % of a chromosome's steps use it, and a chromosome all of whose margins are wide - or
    every chromosome, when `outright` - has the reference's path and calls."""
    for ci, (T, ref) in enumerate(zip(tables, expected)):
        at = f"{msg} chromosome {ci}"
        r = hmm.get(ci, sample=sample, want=WANT + ("eprob",))
        np.testing.assert_allclose(r["eprob"], ref["eprob"], rtol=1e-10, atol=1e-10, err_msg=at)
        check_numbers(r, ref, False, at)                       # device emissions: delta at 1e-9 on every route
        used = hmm_ties.assert_path_eps_optimal(T, ref["delta"], r["states"], at)
        margins, slacks = hmm_ties.decision_table(T, ref["delta"], ref["states"])
        assert used <= 0.05 * len(margins), f"{at}: {used} of {len(margins)} steps used the slack"
        m = min(len(T), ref["delta"].shape[1])
        want_calls = np.full(ref["delta"].shape[1], -1, dtype=np.int32)
        want_calls[:m] = r["states"][:m]
        np.testing.assert_array_equal(r["calls"], want_calls, err_msg=f"calls are not the path's, {at}")
        if outright or (margins > slacks).all():
            np.testing.assert_array_equal(r["states"], ref["states"], err_msg=f"states {at}")
            np.testing.assert_array_equal(r["calls"], ref["calls"], err_msg=f"calls {at}")


# ------------------------------------------------------------------------------------------------ inputs

CC_LENS = [1, 2, 3, 64, 65, 200]
CC_KINDS = ["prior", "one", "two"]


@functools.lru_cache(maxsize=None)
def cc_problem(H, minus_one=False, lens=tuple(CC_LENS)):
    """Class-constant tables and one sample per kind of symmetric emission; the expected values are the oracle's, from
    the same tables and emissions on this machine."""
    tables = [hmm_ties.class_constant_tables(H, n, seed=100 * H + k) for k, n in enumerate(lens)]
    if minus_one:
        tables = [T[:n - 1] for T, n in zip(tables, lens)]
    samples = [[hmm_ties.symmetric_emissions(H, n, kind, seed=1000 * H + 10 * k + j) for k, n in enumerate(lens)]
               for j, kind in enumerate(CC_KINDS)]
    return tables, samples, [oracle_sample(H, tables, E) for E in samples]


@functools.lru_cache(maxsize=None)
def fixture_problem(path):
    g = load_golden(path)
    c = hmm_case_inputs(g)
    chroms = c["chroms"]
    tables = [c["tprob"][ch] for ch in chroms]
    return g, c, tables, fixture_sample(g, chroms)


@functools.lru_cache(maxsize=None)
def ordinary_sample(key, s):
    """Sample s of a batch, drawn as in test_hmm_sample_batches_and_short_chromosomes (seed 1234 + s), on the tables - and,
    for a fixture, the specificity entries - of the tie input `key`: (expression rows, oracle results) per chromosome."""
    from gbrs_amd import synth
    from oracle import hmm_oracle as o
    if key == "cc":
        H, tables, lens = 8, cc_problem(8)[0], CC_LENS
        avec = [[None] * n for n in lens]
    else:
        g, c, tables, _ = fixture_problem(key)
        H, lens = c["H"], [len(c["genes"][ch]) for ch in c["chroms"]]
        avec = [[c["avecs"][ch][i] if c["has_avec"][ch][i] else None for i in range(n)] for ch, n in zip(c["chroms"], lens)]
    p = synth.make_hmm_problem(H=H, genes_per_chrom=lens, seed=1234 + s)
    expr = [np.array([p.expr[x] for x in p.gene_ids[ch]]) for ch in p.chroms]
    iv = o.init_vector(H)
    E = [np.array([o.emission(e[i], a[i], iv, 1.5, 0.12) for i in range(len(e))]) for e, a in zip(expr, avec)]
    return expr, oracle_sample(H, tables, E)


def tie_slots(n_samples):
    return sorted({0, 15, 16, n_samples - 1} & set(range(n_samples)))


# ------------------------------------------------------------------------------------------------ tier A

@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("path", H8_FILES, ids=fid)
def test_tier_a_fixtures_one_sample_routes(path, route, monkeypatch):
    """The reference's emissions on every one-sample route of the 36-state pass."""
    set_route(monkeypatch, ROUTES[route])
    g, c, tables, expected = fixture_problem(path)
    hmm = make_hmm(8, tables, [len(c["genes"][ch]) for ch in c["chroms"]])
    hmm.set_eprob([ref["eprob"] for ref in expected])
    hmm.run()
    check_exact(hmm, 0, expected, route in PLAIN_CHAINS, f"{fid(path)} {route}")
    inf = hmm.info()
    if route.startswith("fallback"):
        bg = int(route.split("-")[1])
        assert inf.last_delta_fallbacks == sum(1 for n in hmm.n_genes if min(64, int(n) // bg) >= 2)
    hmm.close()


@pytest.mark.parametrize("minus_one", [False, True], ids=["tprob_n", "tprob_n_minus_1"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_tier_a_class_constant_one_sample_routes(route, minus_one, monkeypatch):
    """Prior, one-founder and two-founder emissions on class-constant tables at lengths 1, 2, 3, 64, 65 and 200: ties in
    the recursion, at the final argmax and inside the backtrace (tests/test_hmm_ties_cpu.py counts them)."""
    set_route(monkeypatch, ROUTES[route])
    tables, samples, expected = cc_problem(8, minus_one)
    for j, kind in enumerate(CC_KINDS):
        hmm = make_hmm(8, tables, CC_LENS)
        hmm.set_eprob(samples[j])
        hmm.run()
        check_exact(hmm, 0, expected[j], route in PLAIN_CHAINS, f"class-constant {kind} {route}")
        hmm.close()


def test_tier_a_library_defaults_cut_a_long_chromosome():
    """No switch, one sample, 400 genes: the default block length cuts the chromosome."""
    for j, kind in enumerate(CC_KINDS):
        tables, samples, expected = cc_problem(8, False, (400,))
        hmm = make_hmm(8, tables, [400])
        hmm.set_eprob(samples[j])
        hmm.run()
        inf = hmm.info()
        assert inf.last_delta_blocks + inf.last_delta_fallbacks > 0       # the blocked scan ran and did cut it
        check_exact(hmm, 0, expected[j], False, f"class-constant {kind}, 400 genes, defaults")
        hmm.close()


def run_batch(key, n_samples, tier):
    """A batch with the tie samples of input `key` at sample 0, 15, 16 and the last slot among ordinary samples.  Returns
    (hmm, tables, [(sample, expected, is_tie)])."""
    if key == "cc":
        tables, tie_E, tie_expected = cc_problem(8)
        lens, c = CC_LENS, None
    else:
        g, c, tables, ref = fixture_problem(key)
        lens = [len(c["genes"][ch]) for ch in c["chroms"]]
        tie_E, tie_expected = [[r["eprob"] for r in ref]], [ref]
    slots = tie_slots(n_samples)
    members = []
    for s in range(n_samples):
        if s in slots:
            k = slots.index(s) % len(tie_E)
            expr = None if c is None else [c["expr"][ch] for ch in c["chroms"]]
            members.append((tie_E[k], expr, tie_expected[k], True))
        else:
            expr, expected = ordinary_sample(key, s)
            members.append(([r["eprob"] for r in expected], expr, expected, False))
    hmm = make_hmm(8, tables, lens)
    if tier == "A":
        hmm.set_eprob([np.stack([m[0][ci] for m in members]) for ci in range(len(lens))])
    else:
        hmm.set_expression([np.stack([m[1][ci] for m in members]) for ci in range(len(lens))],
                           [c["avecs"][ch] for ch in c["chroms"]], [c["has_avec"][ch] for ch in c["chroms"]], 1.5, 0.12)
    hmm.run()
    return hmm, tables, [(s, m[2], m[3]) for s, m in enumerate(members)]


BATCH_KEYS_A = ["cc"] + H8_FILES              # tier A: the class-constant problem and every 8-founder fixture
BATCH_KEYS_B = H8_FILES                       # tier B: the fixtures (the class-constant problem has no expression)


@pytest.mark.parametrize("n_samples,mfma_ng", BATCH_ROWS)
@pytest.mark.parametrize("key", BATCH_KEYS_A, ids=fid)
def test_tier_a_batches(key, n_samples, mfma_ng, monkeypatch):
    set_batch_route(monkeypatch, mfma_ng)
    hmm, _, members = run_batch(key, n_samples, "A")
    assert sum(1 for m in members if m[2]) == len(tie_slots(n_samples))
    for s, expected, _ in members:
        check_exact(hmm, s, expected, True, f"{fid(key)} sample {s} of {n_samples}")
    hmm.close()


@pytest.mark.parametrize("key", BATCH_KEYS_A, ids=fid)
def test_tier_a_batch_of_70_library_defaults(key):
    hmm, _, members = run_batch(key, 70, "A")
    for s, expected, _ in members:
        check_exact(hmm, s, expected, True, f"{fid(key)} sample {s} of 70")
    hmm.close()


@pytest.mark.parametrize("n_samples", [1, 3])
def test_tier_a_sixteen_founders(n_samples):
    """136 states, the 4-lanes-per-state chains (quad_argmax): the H = 16 fixture and a class-constant problem."""
    path = [p for p in TIE_FILES if p.endswith("hmmtie_h16_silent_weak.npz")][0]
    g, c, tables, expected = fixture_problem(path)
    hmm = make_hmm(16, tables, [len(c["genes"][ch]) for ch in c["chroms"]])
    hmm.set_eprob([np.repeat(ref["eprob"][None], n_samples, axis=0) for ref in expected])
    hmm.run()
    for s in range(n_samples):
        check_exact(hmm, s, expected, True, f"hmmtie_h16 sample {s}")
    hmm.close()
    lens = (1, 2, 3, 33, 70)
    tables, samples, expected = cc_problem(16, False, lens)
    order = [k % 3 for k in range(n_samples)]
    hmm = make_hmm(16, tables, list(lens))
    hmm.set_eprob([np.stack([samples[j][ci] for j in order]) for ci in range(len(lens))])
    hmm.run()
    for s, j in enumerate(order):
        check_exact(hmm, s, expected[j], True, f"class-constant H=16 {CC_KINDS[j]} sample {s}")
    hmm.close()


@pytest.mark.parametrize("H", [2, 3, 4, 5, 7, 9])
def test_tier_a_other_founder_counts(H):
    """3, 4 and 7 founders on the single-wave chain kernels, 2, 5 and 9 on the generic multi-wave kernels; one sample per
    kind of emission in one launch, then each alone; odd founder counts with tprob of length n - 1."""
    lens = (1, 2, 3, 6, 65, 130)
    tables, samples, expected = cc_problem(H, bool(H % 2), lens)
    hmm = make_hmm(H, tables, list(lens))
    hmm.set_eprob([np.stack([samples[j][ci] for j in range(3)]) for ci in range(len(lens))])
    hmm.run()
    for j in range(3):
        check_exact(hmm, j, expected[j], True, f"class-constant H={H} {CC_KINDS[j]} in a batch of 3")
    for j in range(3):
        hmm.set_eprob(samples[j])
        hmm.run()
        check_exact(hmm, 0, expected[j], True, f"class-constant H={H} {CC_KINDS[j]} alone")
    hmm.close()


def test_tier_a_four_founder_fixture():
    path = [p for p in TIE_FILES if p.endswith("hmmtie_h4_silent_weak.npz")][0]
    g, c, tables, expected = fixture_problem(path)
    for n_samples in (1, 5):
        hmm = make_hmm(4, tables, [len(c["genes"][ch]) for ch in c["chroms"]])
        hmm.set_eprob([np.repeat(ref["eprob"][None], n_samples, axis=0) for ref in expected])
        hmm.run()
        for s in range(n_samples):
            check_exact(hmm, s, expected, True, f"hmmtie_h4 sample {s} of {n_samples}")
        hmm.close()


# ------------------------------------------------------------------------------------------------ tier B

def set_fixture_expression(hmm, g, c, n_samples=1):
    chroms = c["chroms"]
    ex = [c["expr"][ch] if n_samples == 1 else np.repeat(c["expr"][ch][None], n_samples, axis=0) for ch in chroms]
    hmm.set_expression(ex, [c["avecs"][ch] for ch in chroms], [c["has_avec"][ch] for ch in chroms],
                       float(g["expr_threshold"]), float(g["sigma"]))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("path", H8_FILES, ids=fid)
def test_tier_b_fixtures_one_sample_routes(path, route, monkeypatch):
    set_route(monkeypatch, ROUTES[route])
    g, c, tables, expected = fixture_problem(path)
    hmm = make_hmm(8, tables, [len(c["genes"][ch]) for ch in c["chroms"]])
    set_fixture_expression(hmm, g, c)
    hmm.run()
    check_eps_optimal(hmm, 0, tables, expected, f"{fid(path)} {route}", outright=path.endswith("h8_silent_only.npz"))
    hmm.close()


@pytest.mark.parametrize("n_samples,mfma_ng", BATCH_ROWS)
@pytest.mark.parametrize("key", BATCH_KEYS_B, ids=fid)
def test_tier_b_batches(key, n_samples, mfma_ng, monkeypatch):
    set_batch_route(monkeypatch, mfma_ng)
    hmm, tables, members = run_batch(key, n_samples, "B")
    for s, expected, is_tie in members:
        check_eps_optimal(hmm, s, tables, expected, f"{fid(key)} sample {s} of {n_samples}",
                          outright=is_tie and key.endswith("h8_silent_only.npz"))
    hmm.close()


@pytest.mark.parametrize("key", BATCH_KEYS_B, ids=fid)
def test_tier_b_batch_of_70_library_defaults(key):
    hmm, tables, members = run_batch(key, 70, "B")
    for s, expected, is_tie in members:
        check_eps_optimal(hmm, s, tables, expected, f"{fid(key)} sample {s} of 70",
                          outright=is_tie and key.endswith("h8_silent_only.npz"))
    hmm.close()


@pytest.mark.parametrize("path", [p for p in TIE_FILES if "_h8_" not in p], ids=fid)
def test_tier_b_four_and_sixteen_founders(path):
    g, c, tables, expected = fixture_problem(path)
    for n_samples in (1, 3):
        hmm = make_hmm(c["H"], tables, [len(c["genes"][ch]) for ch in c["chroms"]])
        set_fixture_expression(hmm, g, c, n_samples)
        hmm.run()
        for s in range(n_samples):
            check_eps_optimal(hmm, s, tables, expected, f"{fid(path)} sample {s} of {n_samples}")
        hmm.close()


@pytest.mark.parametrize("route", ["defaults", "unblocked", "rank-9"])
def test_tier_b_reconstruct_files_silent_only(route, tmp_path, monkeypatch):
    """`gbrs reconstruct` on files, as test_reconstruct_files: genotypes.tsv of the silent-only fixture character for
    character, the exact ties of its silent chromosomes included."""
    from gbrs_amd import hmm as H
    from gbrs_amd.synth import diplotype_names
    set_route(monkeypatch, ROUTES[route])
    g, c, _, _ = fixture_problem([p for p in TIE_FILES if p.endswith("hmmtie_h8_silent_only.npz")][0])
    chroms = c["chroms"]
    hn = [chr(65 + h) for h in range(c["H"])]
    (tmp_path / "ref.fa.fai").write_text("".join(f"{ch}\t1000\t0\t60\t61\n" for ch in chroms) + "MT\t16299\t0\t60\t61\n")
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    with open(tmp_path / "genes.tpm", "w") as fh:
        fh.write("locus\t" + "\t".join(hn) + "\ttotal\n")
        for ch in chroms:
            for gid, v in zip(c["genes"][ch], c["expr"][ch]):
                fh.write(str(gid) + "\t" + "\t".join(repr(float(x)) for x in v) + "\t" + repr(float(v.sum())) + "\n")
    np.savez(tmp_path / "tprob.npz", **{ch: c["tprob"][ch] for ch in chroms})
    av, gp = {}, {}
    for ch in chroms:
        for gid, has, a in zip(c["genes"][ch], c["has_avec"][ch], c["avecs"][ch]):
            if has:
                av[str(gid)] = a
        arr = np.zeros(len(c["genes"][ch]), dtype=[("f0", "U24"), ("f1", "i8")])
        arr["f0"] = c["genes"][ch]
        gp[ch] = arr
    np.savez(tmp_path / "avecs.npz", **av)
    np.savez(tmp_path / "gpos.npz", **gp)
    out = str(tmp_path / "out")
    H.reconstruct(str(tmp_path / "genes.tpm"), str(tmp_path / "tprob.npz"), str(tmp_path / "avecs.npz"),
                  str(tmp_path / "gpos.npz"), 1.5, 0.12, out)
    assert open(out + ".genotypes.tsv").read() == str(g["tsv_text"])
    st = np.load(out + ".genotypes.npz")
    names = diplotype_names(hn)
    for ch in chroms:
        assert list(st[ch]) == [names[s] for s in g[f"states_{ch}"]]


# ------------------------------------------------------------------------------------------------ tier C

def test_tier_c_blocked_scan_equals_the_unblocked_chain_on_ties_at_size(monkeypatch):
    """Three long chromosomes on jitter-free DO tables with a tenth of the haplotypes expressed, one with a silent run of
    400 genes (longer than a block), one silent throughout: with the emissions the device itself computed the blocked
    scan's path and calls are the unblocked chain's, both are eps-optimal against the oracle, and the chromosomes
    without information take the fallback chain."""
    from gbrs_amd import synth
    from gbrs_amd.hmm import DiplotypeHMM
    from oracle import hmm_oracle
    prob = synth.make_hmm_problem(H=8, genes_per_chrom=[2600, 1700, 1100], style="do", jitter=0, expressed_fraction=0.1)
    chroms = prob.chroms
    ex = [np.array([prob.expr[g] for g in prob.gene_ids[c]]) for c in chroms]
    ex[0][300:700] = 0.0
    ex[2][:] = 0.0
    ha = [np.array([g in prob.avecs for g in prob.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([prob.avecs.get(g, np.zeros((8, 8))) for g in prob.gene_ids[c]]) for c in chroms]
    res, fallbacks, tie_fallbacks = {}, None, None
    for mode in ("0", "2"):
        monkeypatch.setenv("GBRS_TUNING_HMM_BLOCKED", mode)
        hmm = DiplotypeHMM(8, chroms, [len(prob.gene_ids[c]) for c in chroms], [prob.tprob[c] for c in chroms])
        hmm.set_expression(ex, av, ha, 1.5, 0.12)
        hmm.run()
        res[mode] = [hmm.get(ci, want=("states", "calls", "delta")) for ci in range(3)]
        if mode == "2":
            fallbacks, tie_fallbacks = hmm.info().last_delta_fallbacks, hmm.info().last_delta_tie_fallbacks
        hmm.close()
    print(f"last_delta_fallbacks = {fallbacks}, of them for a close decision alone = {tie_fallbacks}")
    iv = hmm_oracle.init_vector(8)
    for ci, (a, b) in enumerate(zip(res["0"], res["2"])):
        np.testing.assert_array_equal(a["states"], b["states"], err_msg=f"chromosome {ci}")
        np.testing.assert_array_equal(a["calls"], b["calls"], err_msg=f"chromosome {ci}")
        np.testing.assert_allclose(b["delta"], a["delta"], rtol=1e-10, atol=1e-9)
        ids = prob.gene_ids[chroms[ci]]
        E = np.array([hmm_oracle.emission(ex[ci][k], prob.avecs.get(g), iv) for k, g in enumerate(ids)])
        T = prob.tprob[chroms[ci]]
        d_ref, st_ref, _ = hmm_oracle.viterbi(T, E, iv)
        np.testing.assert_allclose(b["delta"], d_ref, rtol=1e-10, atol=1e-9)
        margins, slacks = hmm_ties.decision_table(T, d_ref, st_ref)
        print(f"chromosome {ci}: {int((margins == 0).sum())} exact ties, {int(((margins > 0) & (margins <= slacks)).sum())} "
              f"decisions inside the slack, of {len(margins)}")
        for mode in ("0", "2"):
            hmm_ties.assert_path_eps_optimal(T, d_ref, res[mode][ci]["states"], f"BLOCKED={mode} chromosome {ci}")
    # the silent chromosome and the one with the 400-gene silent run.  The run is longer than a block, so blocks inside it
    # cannot meet the values chained from the informative genes before it: the fix-up itself gives that chromosome up.  The
    # blocks of the silent chromosome do converge (both chains settle behind the first cheap recombination interval); it is
    # the tie among the heterozygotes at its last gene that sends it to the sequential chain.
    assert fallbacks >= 2
    assert fallbacks - tie_fallbacks >= 1 and tie_fallbacks >= 1
