"""Input files of `gbrs quantify` from an em_*.npz golden (alignment, group, length and genotype files), for the tests
of the sharded command (`--gpus N`)."""
import numpy as np

from conftest import em_case_inputs, em_case_values, golden_files, load_golden


def golden_path(name):
    return [p for p in golden_files("em") if p.endswith(f"em_{name}.npz")][0]


def write_case(tmp_path, name, fmt="npz", use_mask=False):
    """(quantify argv without -o, report suffix, golden dict, gene calls or None)."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    g = load_golden(golden_path(name))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask = em_case_inputs(g)
    hn = [chr(65 + h) for h in range(H)]
    ln = [f"T{l:07d}" for l in range(L)]
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                  haplotype_names=hn, locus_names=ln, values=em_case_values(g))
    aln = tmp_path / f"aln.{fmt}"
    if fmt == "h5":
        apm.save(str(aln), incidence_only=apm.values is None)
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
    argv = ["quantify", "-i", str(aln), "-g", str(grp), "-L", str(lens), "-p", str(float(g["pseudocount"]))]
    calls = None
    if use_mask:
        gt = tmp_path / "gt.tsv"
        calls = []
        with open(gt, "w") as fh:
            fh.write("#Gene_ID\tDiplotype\n")
            for i, mem in enumerate(groups):
                hs = np.flatnonzero(gtmask[:, mem[0]])
                calls.append("".join(hn[h] for h in (hs if len(hs) == 2 else [hs[0], hs[0]])))
                fh.write(f"G{i:07d}\t{calls[-1]}\n")
        argv += ["-G", str(gt)]
    return argv, ("diploid" if use_mask else "multiway"), g, calls


REPORTS = (("text_isoforms_tpm", "isoforms.tpm"), ("text_isoforms_counts", "isoforms.expected_read_counts"),
           ("text_genes_tpm", "genes.tpm"), ("text_genes_counts", "genes.expected_read_counts"))


def parse_tsv(text):
    lines = [l.split("\t") for l in text.strip().split("\n")]
    return lines[0], {l[0]: l[1:] for l in lines[1:]}


def check_reports_against_golden(out_prefix, g):
    """The four EM reports under `out_prefix` hold the golden's rows, within 1e-9 of its numbers."""
    for key, fname in REPORTS:
        got_h, got = parse_tsv(open(f"{out_prefix}.{fname}").read())
        exp_h, exp = parse_tsv(str(g[key]))
        assert got_h[:len(exp_h)] == exp_h and list(got) == list(exp), fname
        for k in exp:
            np.testing.assert_allclose([float(x) for x in got[k][:len(exp[k])]], [float(x) for x in exp[k]],
                                       rtol=1e-9, atol=1e-300, err_msg=f"{fname} {k}")


def check_reports_close(prefix_a, prefix_b, names, rtol=1e-9):
    """Two runs' reports: the same rows and header, numbers within rtol."""
    for fname in names:
        ha, a = parse_tsv(open(f"{prefix_a}.{fname}").read())
        hb, b = parse_tsv(open(f"{prefix_b}.{fname}").read())
        assert ha == hb and list(a) == list(b), fname
        for k in a:
            va, vb = a[k], b[k]
            num = [i for i, x in enumerate(va) if x not in ("None",) and not x.isalpha()]
            np.testing.assert_allclose([float(va[i]) for i in num], [float(vb[i]) for i in num], rtol=rtol, atol=1e-300,
                                       err_msg=f"{fname} {k}")
            assert [va[i] for i in range(len(va)) if i not in num] == [vb[i] for i in range(len(vb)) if i not in num]
