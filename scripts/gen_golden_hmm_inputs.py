#!/usr/bin/env python3
"""Generate tests/golden/tranprob_<case>.npz and tests/golden/alnspec_<case>.npz by running the imported reference's
get_transition_prob and get_alignment_spec (gbrs/gbrs_utils.py:208-294, :297-379).

Build container only (the reference's sources are not on the GPU machines); no test, smoke() or bench.py calls it:

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_hmm_inputs.py

get_transition_prob runs unmodified.  get_alignment_spec does not run under Python 3 as written (`dtype='string'` at
gbrs_utils.py:322 is rejected, a `map` object is assigned into an array row at :350), so it runs with two names patched
in the reference module's namespace, and nothing else changed:

  * the module's `np` is a proxy of numpy whose loadtxt maps dtype='string' to str;
  * the module-level name `map` is a map that returns a list.

Every file holds the input texts as strings (the marker file; or the gene list, the sample list and the report files,
with @DIR@ for the directory the reports lie in) and the reference's output arrays with the key list `<name>_keys` beside them:
tprob / gpos under `<name>_<key>` members, the equally shaped per-gene blocks axes / ases / avecs stacked in key order
under `<name>` (one zip member per gene would put either alnspec file above 200 KB).  Before a file is written the outputs are
asserted to agree with tests/hmm_inputs_restate.py: exactly for the tables, the gene positions, axes and ases, to 1e-15
for avecs.
"""
import contextlib
import io
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.environ.get("GBRS_REFERENCE_SRC", "/root/reference/src")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF_SRC)

import numpy as np  # noqa: E402

WORK = tempfile.mkdtemp(prefix="gbrs_golden_hmm_inputs_")
os.environ["GBRS_DATA"] = WORK            # read at import time by gbrs_utils (gbrs_utils.py:20)

from gbrs.gbrs import gbrs_utils as ref  # noqa: E402

import hmm_inputs_restate as hr  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MAX_BYTES = 200_000


class _NumpyWithStringDtype:
    """numpy, except that loadtxt(dtype='string') reads str (the Python-2 spelling at gbrs_utils.py:322)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def loadtxt(*args, **kw):
        if kw.get("dtype") == "string":
            kw["dtype"] = str
        return np.loadtxt(*args, **kw)


def _list_map(fn, *iterables):
    return list(map(fn, *iterables))


def patch_for_alignment_spec():
    ref.np = _NumpyWithStringDtype()
    ref.map = _list_map


def load_npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def keyed_members(name, arrays, stacked=False):
    """A dict of arrays as fixture members: the key list `<name>_keys` and one member `<name>_<key>` per array, or -
    stacked, for the hundreds of equally shaped per-gene blocks, which as members of their own would cost more zip
    directory than data - one member `<name>` that holds them in key order."""
    out = {f"{name}_keys": np.array(list(arrays), dtype=str)}
    if stacked:
        out[name] = np.stack(list(arrays.values()))
        return out
    for k, a in arrays.items():
        out[f"{name}_{k}"] = a
    return out


def save(name, members):
    path = os.path.join(GOLD, f"{name}.npz")
    np.savez_compressed(path, **members)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    return size


# ---- get-transition-prob ---------------------------------------------------------------------------------------------
def marker_lines(rng, chrom, n, specials=()):
    """n markers of one chromosome: cM steps of 0.001 - 2.5, `specials` = (index, step) overrides"""
    steps = np.round(rng.uniform(0.001, 2.5, size=n), 4)
    for k, s in specials:
        steps[k] = s
    cm, bp, out = 0.0, 3_000_000, []
    for k in range(n):
        cm = float(np.round(cm + steps[k], 7)) if k else float(np.round(rng.uniform(0.0, 3.0), 4))
        bp += int(rng.integers(1_000, 900_000))
        out.append(f"ENSG{chrom}_{k:04d}\t{chrom}\t{bp}\t{cm!r}\n")
    return out


def case_tranprob_main():
    rng = np.random.default_rng(301)
    one = marker_lines(rng, "1", 70, [(10, 0.0), (20, -0.37), (30, 4e-7), (40, 50.0)])
    two = marker_lines(rng, "2", 301, [(150, 0.0), (299, 50.0), (300, -2.0)])
    ex = marker_lines(rng, "X", 5, [(1, 0.0), (3, 50.0), (4, 3e-7)])
    low = marker_lines(rng, "x", 3)
    why = marker_lines(rng, "Y", 2)
    mt = marker_lines(rng, "MT", 1)
    # the markers of `1` are split by a block of `X` lines: chromosomes are grouped, not file-contiguous
    lines = one[:33] + ex[:2] + one[33:] + two + ex[2:] + low + why + mt
    return dict(marker_text="".join(lines), haplotypes="A,B", mating_scheme="RI", gamma_scale=0.01, epsilon=0.000001)


def case_tranprob_params():
    rng = np.random.default_rng(302)
    lines = marker_lines(rng, "3", 12, [(4, 5e-4), (7, 0.0)]) + marker_lines(rng, "X", 9, [(2, 9e-4), (5, -1.0)])
    return dict(marker_text="".join(lines), haplotypes="A,B", mating_scheme="RI", gamma_scale=0.25, epsilon=1e-3)


def write_tranprob(name, c):
    work = tempfile.mkdtemp(dir=WORK)
    marker_file = os.path.join(work, "markers.tsv")
    with open(marker_file, "w") as fh:
        fh.write(c["marker_text"])
    out_file = os.path.join(work, "tranprob.npz")                 # absolute: os.path.join(DATA_DIR, ...) keeps it
    ref.get_transition_prob(marker_file, haplotypes=c["haplotypes"], mating_scheme=c["mating_scheme"],
                            gamma_scale=c["gamma_scale"], epsilon=c["epsilon"], output_file=out_file)
    tprob = load_npz(out_file)
    gpos = {k: v.astype(str) for k, v in load_npz(os.path.join(WORK, "ref.gene_pos.ordered.npz")).items()}
    tables, positions = hr.transition_prob(c["marker_text"], c["gamma_scale"], c["epsilon"])
    assert list(tprob) == list(tables) == list(gpos) == list(positions), (name, list(tprob), list(tables))
    for k in tprob:
        assert tprob[k].shape == tables[k].shape and tprob[k].dtype == np.float64, (name, k, tprob[k].shape)
        assert np.array_equal(tprob[k], tables[k]), (name, k, "tables differ from the restatement")
        assert np.isfinite(tprob[k]).all(), (name, k)
        assert np.array_equal(gpos[k], positions[k]), (name, k, "gene positions differ from the restatement")
    g = dict(marker_text=np.array(c["marker_text"]), haplotypes=np.array(c["haplotypes"]),
             mating_scheme=np.array(c["mating_scheme"]), gamma_scale=np.float64(c["gamma_scale"]),
             epsilon=np.float64(c["epsilon"]))
    g.update(keyed_members("tprob", tprob))
    g.update(keyed_members("gpos", gpos))
    size = save(f"tranprob_{name}", g)
    print(f"tranprob_{name}: chromosomes {[(k, len(v)) for k, v in tprob.items()]} size={size} B")


# ---- get-alignment-spec ----------------------------------------------------------------------------------------------
def report_text(strains, rows):
    """rows: [(gene, values)] -> a genes.tpm report (locus, one column per strain, total)"""
    out = ["locus\t" + "\t".join(strains) + "\ttotal\n"]
    for gene, v in rows:
        out.append(gene + "\t" + "\t".join(repr(float(x)) for x in v) + "\t" + repr(float(np.sum(v))) + "\n")
    return "".join(out)


def alnspec_case(seed, strains, n_genes, files_per_strain, missing, min_expr=2.0):
    """files_per_strain[i] report files for strain i (strain 0 has one, so that its rows are a file's own numbers);
    missing: (strain, file) pairs that are listed and do not exist."""
    rng = np.random.default_rng(seed)
    S = len(strains)
    assert files_per_strain[0] == 1 and S >= 2
    genes = [f"ENSMUSG{k:05d}" for k in range(n_genes)]
    gene_text = "".join(g + "".join(f"\tENSMUST{k:05d}_{t}" for t in range(1 + k % 3)) + "\n" for k, g in enumerate(genes))
    ABSENT, TWICE, NOFILE, LOW, ONE, ZERO, TINY, EXACT = 3, 5, 7, 11, 13, 17, 19, 23
    sample_lines, paths, texts, missing_paths = [], [], [], []
    for i, st in enumerate(strains):
        for f in range(files_per_strain[i]):
            path = f"{hr.DIR_TOKEN}/{st}_{f}.genes.tpm"
            sample_lines.append(f"{st}\t{path}\n")
            if (i, f) in missing:
                missing_paths.append(path)
                continue
            rows = []
            for k, gene in enumerate(genes):
                v = np.round(rng.lognormal(0.0, 1.5, size=S) * (rng.random(S) < 0.8), 3)
                v[i] = np.round(v[i] + rng.lognormal(2.0, 1.0), 3)           # a strain's reads prefer its own haplotype
                if k == NOFILE or (k == ABSENT and f == files_per_strain[i] - 1 and i == S - 1):
                    continue
                if k == LOW:                                                # below min_expr in every strain
                    v = np.round(rng.uniform(0.0, min_expr / (S + 1), size=S), 3)
                if k == ONE and i != 1:                                     # expressed in strain 1 only
                    v = np.round(rng.uniform(0.0, min_expr / (S + 1), size=S), 3)
                if k in (ONE, ZERO, TINY) and i == 1:                       # surely above min_expr there
                    v[i] = np.round(v[i] + 5.0, 3)
                if k == ZERO and i == 0:                                    # an all-zero row next to expressed ones
                    v = np.zeros(S)
                if k == TINY and i == 0:                                    # 0 < sum <= 1e-6: left unscaled
                    v = np.zeros(S)
                    v[0], v[1] = 3e-7, 2e-7
                if k == EXACT:                                              # the largest row sum is min_expr itself
                    v = np.zeros(S)
                    if i == 0:
                        v[0], v[1] = 1.5, min_expr - 1.5
                    else:
                        v[i] = 0.25
                if k == TWICE and f == 0:
                    rows.append((gene, np.round(v + 1.0, 3)))               # overwritten by the line below
                rows.append((gene, v))
                if k == 29 and f == 0:
                    rows.append(("ENSMUSG_NOT_LISTED", np.round(v * 2.0, 3)))
            paths.append(path)
            texts.append(report_text(strains, rows))
    return dict(gene_text=gene_text, sample_text="".join(sample_lines), report_paths=paths, report_texts=texts,
                missing_paths=missing_paths, strains=strains, min_expr=min_expr,
                special=dict(absent=genes[ABSENT], twice=genes[TWICE], nofile=genes[NOFILE], low=genes[LOW], one=genes[ONE],
                             zero=genes[ZERO], tiny=genes[TINY], exact=genes[EXACT]))


def case_alnspec_s2():
    return alnspec_case(311, ["A", "B"], 300, [1, 3], {(1, 1)})


def case_alnspec_s8():
    return alnspec_case(312, list("ABCDEFGH"), 130, [1, 2, 3, 1, 2, 3, 2, 1], set())


def write_alnspec(name, c):
    work = tempfile.mkdtemp(dir=WORK)
    g = dict(gene_text=np.array(c["gene_text"]), sample_text=np.array(c["sample_text"]),
             report_paths=np.array(c["report_paths"], dtype=str), report_texts=np.array(c["report_texts"], dtype=str),
             missing_paths=np.array(c["missing_paths"], dtype=str), strains=np.array(c["strains"], dtype=str),
             min_expr=np.float64(c["min_expr"]),
             special_names=np.array(list(c["special"]), dtype=str), special_genes=np.array(list(c["special"].values()), dtype=str))
    sample_file, strains, min_expr, missing = hr.alnspec_write_inputs(g, work)
    os.replace(os.path.join(work, "ref.gene2transcripts.tsv"), os.path.join(WORK, "ref.gene2transcripts.tsv"))
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        ref.get_alignment_spec(sample_file, strains, min_expr=min_expr)
    assert said.getvalue() == "".join(f"File {p} does not exist.\n" for p in missing), said.getvalue()
    axes, ases, avecs = (load_npz(os.path.join(WORK, f"{k}.npz")) for k in ("axes", "ases", "avecs"))
    r_axes, r_ases, r_avecs, r_missing = hr.alignment_spec(c["gene_text"], c["sample_text"].replace(hr.DIR_TOKEN, work),
                                                           hr.alnspec_reports(g, work), strains, min_expr)
    assert r_missing == missing
    assert list(axes) == list(r_axes) and list(ases) == list(r_ases) and list(avecs) == list(r_avecs), name
    worst = 0.0
    for k in axes:
        assert axes[k].shape == r_axes[k].shape and np.array_equal(axes[k], r_axes[k]), (name, k, "axes")
        assert ases[k].shape == r_ases[k].shape == (1, len(strains)) and np.array_equal(ases[k], r_ases[k]), (name, k, "ases")
    for k in avecs:
        assert avecs[k].shape == r_avecs[k].shape
        worst = max(worst, hr.max_rel(r_avecs[k], avecs[k]))
    assert worst <= 1e-15, (name, worst)
    # the cases the kernels can get wrong are really there
    sp = c["special"]
    assert sp["low"] not in avecs and sp["nofile"] not in avecs and sp["exact"] not in avecs
    assert ases[sp["exact"]].max() == min_expr and not axes[sp["nofile"]].any()
    assert sp["one"] in avecs and (ases[sp["one"]][0] > min_expr).tolist() == [False, True] + [False] * (len(strains) - 2)
    assert sp["zero"] in avecs and not axes[sp["zero"]][0].any() and not avecs[sp["zero"]][0].any()
    assert sp["tiny"] in avecs and 0 < ases[sp["tiny"]][0, 0] <= 1e-6
    assert np.array_equal(avecs[sp["tiny"]][0], axes[sp["tiny"]][0])
    g.update(keyed_members("axes", axes, stacked=True))
    g.update(keyed_members("ases", ases, stacked=True))
    g.update(keyed_members("avecs", avecs, stacked=True))
    size = save(f"alnspec_{name}", g)
    print(f"alnspec_{name}: strains={len(strains)} genes={len(axes)} with avecs={len(avecs)} files={len(c['report_paths'])} "
          f"missing={len(missing)} worst rel diff of avecs vs restatement={worst:.1e} size={size} B")


TRANPROB = dict(main=case_tranprob_main, params=case_tranprob_params)
ALNSPEC = dict(s2=case_alnspec_s2, s8=case_alnspec_s8)


def main():
    os.makedirs(GOLD, exist_ok=True)
    for name, make in TRANPROB.items():
        write_tranprob(name, make())
    patch_for_alignment_spec()
    for name, make in ALNSPEC.items():
        write_alnspec(name, make())


if __name__ == "__main__":
    main()
