"""numpy restatement of `gbrs get-transition-prob` (gbrs/gbrs_utils.py:101-187, :208-294) and of
`gbrs get-alignment-spec` (:297-379) on texts instead of files, and the readers of the tranprob_*.npz / alnspec_*.npz
fixtures (made by running the reference, scripts/gen_golden_hmm_inputs.py, which asserts that it agrees with this
file: exactly for the tables, the gene positions, axes and ases, to 1e-15 for avecs).  It shares no code with
gbrs_amd.hmm_inputs."""
import io
import os
from collections import OrderedDict

import numpy as np

DIR_TOKEN = "@DIR@"          # stands for the directory of the report files inside a fixture's sample list


# ---- get-transition-prob ---------------------------------------------------------------------------------------------
def parse_markers(marker_text):
    """chromosome -> (ids, positions, cM), chromosomes in order of first appearance, markers in file order"""
    by_chrom = OrderedDict()
    for line in io.StringIO(marker_text):
        item = line.rstrip().split("\t")
        ids, pos, cm = by_chrom.setdefault(item[1], ([], [], []))
        ids.append(item[0])
        pos.append(int(item[2]))
        cm.append(float(item[3]))
    return by_chrom


def ri_table(cm, is_x, gamma_scale, epsilon, scalar_logs=True):
    """(n - 1, 3, 3) log transition table of one chromosome, ris_step's forward direction in its operation order.
    scalar_logs: one np.log call per number, as the reference makes them (the fixtures are equal to that bit for bit);
    without it the same expressions on whole arrays, for chromosomes of a million markers - numpy's array loops may
    round a logarithm differently from its scalar path, by an ulp."""
    d = np.diff(np.array(cm, dtype=np.float64))
    d[d < epsilon] = epsilon
    out = np.empty((len(d), 3, 3))
    for i, r in enumerate(d if scalar_logs else [d]):
        if is_x:
            R = (2 * r) / (1.0 + 4.0 * r)
        else:
            R = 4.0 * r / (1 + 6.0 * r)
        g = R * gamma_scale
        z = np.log(1 + g)
        last = [np.log(2.0 * R) - z, np.log(g) - z, np.log(1.0 - 2.0 * R) - z] if is_x else \
            [np.log(R) - z, np.log(g) - z, np.log(1.0 - R) - z]
        first = [np.log(1.0 - R) - z, np.log(g) - z, np.log(R) - z]
        where = i if scalar_logs else slice(None)
        for e in range(3):
            out[where, 0, e] = first[e]
            out[where, 1, e] = np.log(1 / 3.0)
            out[where, 2, e] = last[e]
    return out


def transition_prob(marker_text, gamma_scale=0.01, epsilon=0.000001):
    """(chromosome -> table, chromosome -> (n, 2) string array [id, str(position)]), both in file order"""
    tables, gpos = OrderedDict(), OrderedDict()
    for c, (ids, pos, cm) in parse_markers(marker_text).items():
        tables[c] = ri_table(cm, c == "X", gamma_scale, epsilon)
        gpos[c] = np.array([[i, str(p)] for i, p in zip(ids, pos)], dtype=str).reshape(len(ids), 2)
    return tables, gpos


# ---- get-alignment-spec ----------------------------------------------------------------------------------------------
def unit_vector(v):
    if sum(v) > 1e-6:
        return v / np.sqrt(np.dot(v, v))
    return v


def spec_from_tables(tables, divisors, min_expr=2.0):
    """tables[i]: the (G x S) tables of strain i's existing files, in file order; divisors[i]: the files it lists.
    Returns axes (G, S, S), ases (G, S), avecs (G, S, S; rows of genes without a block are 0) and has_avec (G)."""
    S = len(divisors)
    G = next(t[0].shape[0] for t in tables if len(t))          # (at least one table)
    dset = []
    for i in range(S):
        total = np.zeros((G, S))
        for one in tables[i]:
            total += one
        dset.append(total / divisors[i])
    axes, ases, avecs = np.zeros((G, S, S)), np.zeros((G, S)), np.zeros((G, S, S))
    has = np.zeros(G, dtype=bool)
    for g in range(G):
        for i in range(S):
            axes[g, i, :] = dset[i][g, :]
            ases[g, i] = sum(axes[g, i, :])
        has[g] = any(s > min_expr for s in ases[g])
        if has[g]:
            for i in range(S):
                avecs[g, i, :] = unit_vector(axes[g, i, :])
    return axes, ases, avecs, has


def alignment_spec(gene_text, sample_text, reports, strains, min_expr=2.0):
    """reports: path -> text of the report files that exist.  Returns (axes, ases, avecs, missing paths)."""
    S = len(strains)
    gname = np.loadtxt(io.StringIO(gene_text), usecols=(0,), dtype=str).tolist()
    G = len(gname)
    gid = dict(zip(gname, range(G)))
    flist = OrderedDict()
    for line in io.StringIO(sample_text):
        item = line.rstrip().split("\t")
        flist.setdefault(item[0], []).append(item[1])
    tables, missing = [], []
    for st in strains:
        mine = []
        for path in flist[st]:
            if path not in reports:
                missing.append(path)
                continue
            one = np.zeros((G, S))
            for line in list(io.StringIO(reports[path]))[1:]:
                item = line.rstrip().split("\t")
                if item[0] in gid:
                    one[gid[item[0]], :] = [float(x) for x in item[1:S + 1]]
            mine.append(one)
        tables.append(mine)
    if not any(len(t) for t in tables):
        tables[0] = [np.zeros((G, S))]           # no file at all: adding a table of zeros changes nothing
    a, s, v, has = spec_from_tables(tables, [len(flist[st]) for st in strains], min_expr)
    axes = OrderedDict((g, a[gid[g]]) for g in gname)
    ases = OrderedDict((g, s[gid[g]][None, :]) for g in gname)
    avecs = OrderedDict((g, v[gid[g]]) for g in gname if has[gid[g]])
    return axes, ases, avecs, missing


# ---- fixtures --------------------------------------------------------------------------------------------------------
def keyed(g, name):
    """the arrays of the key list `<name>_keys`, in its order: stored as `<name>_<key>` members, or stacked as `<name>`"""
    if name in g:
        return OrderedDict((str(k), a) for k, a in zip(g[f"{name}_keys"], g[name]))
    return OrderedDict((str(k), g[f"{name}_{k}"]) for k in g[f"{name}_keys"])


def tranprob_params(g):
    return dict(haplotypes=str(g["haplotypes"]), mating_scheme=str(g["mating_scheme"]),
                gamma_scale=float(g["gamma_scale"]), epsilon=float(g["epsilon"]))


def alnspec_reports(g, directory=DIR_TOKEN):
    """path -> text of the fixture's existing report files, the paths under `directory`"""
    return {str(p).replace(DIR_TOKEN, directory): str(t) for p, t in zip(g["report_paths"], g["report_texts"])}


def alnspec_write_inputs(g, directory):
    """Writes the gene list (ref.gene2transcripts.tsv), the sample list and the report files of an alnspec fixture under
    `directory`; returns (sample file, strains, min_expr, the listed paths that do not exist)."""
    directory = str(directory)
    with open(os.path.join(directory, "ref.gene2transcripts.tsv"), "w") as fh:
        fh.write(str(g["gene_text"]))
    sample_file = os.path.join(directory, "samples.tsv")
    with open(sample_file, "w") as fh:
        fh.write(str(g["sample_text"]).replace(DIR_TOKEN, directory))
    for path, text in alnspec_reports(g, directory).items():
        with open(path, "w") as fh:
            fh.write(text)
    missing = [str(p).replace(DIR_TOKEN, directory) for p in g["missing_paths"]]
    return sample_file, [str(s) for s in g["strains"]], float(g["min_expr"]), missing


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r[a == b] = 0.0
    return float(r.max())
