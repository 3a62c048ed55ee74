"""Shapes and candidate table sets of the log-likelihood pass (gbrs_hmm_loglik, gbrs_hmm_loglik_tables,
`gbrs reconstruct --loglik / --alt-tprob-file`): plain numpy, no GPU.

The problems are grid_cases': chromosomes of 1, 2, 3, 65 and 200 genes, H in HS, styles "benign" and "do"."""
import functools

import numpy as np

import grid_cases

HS = (1, 2, 3, 8, 16)
STYLES = ("benign", "do")
CANDIDATES = ("other", "x_only", "minus_inf", "short")


def other(style):
    return "benign" if style == "do" else "do"


def tables_of(p):
    return [p.tprob[c] for c in p.chroms]


@functools.lru_cache(maxsize=None)
def candidate(H, style, name):
    """A candidate table set for the problem (H, style), per chromosome in handle order, read-only:
    "base"       the problem's own tables;
    "other"      the other style's tables of the same H;
    "x_only"     the base with the blocks of "X" re-drawn with another seed (the other chromosomes are the base's arrays);
    "minus_inf"  the base with -inf in every transition INTO the last state on "4" (every block);
    "short"      the tprob_len_minus_one variant: n - 1 blocks per chromosome, none for the one-gene chromosome."""
    from gbrs_amd import synth
    p0 = grid_cases.problem(H, style)
    base = tables_of(p0)
    if name == "base":
        out = base
    elif name == "other":
        out = tables_of(grid_cases.problem(H, other(style)))
    elif name == "x_only":
        with np.errstate(divide="ignore"):
            q = synth.make_hmm_problem(H=H, genes_per_chrom=list(grid_cases.LENS), chroms=list(grid_cases.CHROMS),
                                       seed=grid_cases.SEED + H + 77, style=style)
        out = base[:-1] + [q.tprob["X"]]
    elif name == "minus_inf":
        t = base[3].copy()
        t[:, -1, :] = -np.inf
        out = base[:3] + [t] + base[4:]
    elif name == "short":
        with np.errstate(divide="ignore"):
            q = synth.make_hmm_problem(H=H, genes_per_chrom=list(grid_cases.LENS), chroms=list(grid_cases.CHROMS),
                                       seed=grid_cases.SEED + H, style=style, tprob_len_minus_one=True)
        out = tables_of(q)
    else:
        raise KeyError(name)
    for t in out:
        t.setflags(write=False)
    return tuple(out)


def write_candidate(path, H, style, name):
    """The candidate as a table file (.npz, one member per chromosome)."""
    np.savez(path, **dict(zip(grid_cases.CHROMS, candidate(H, style, name))))
    return str(path)


# The fixtures of the command tests (base style, alternatives, samples); tests/test_loglik_cpu.py asserts that the oracle
# decides each of them by more than 1e-6, or ties exactly.  COMMAND: some of the five samples stay with the base and some
# move to "x_only".  SINGLE: the "do" tables against the "benign" ones, which explain the sample better by thousands.
# TIE_H: one founder, every table is log(1) = 0, the totals tie exactly and the first listed candidate wins.
COMMAND_H, COMMAND_STYLE, COMMAND_ALTS, COMMAND_SAMPLES = 8, "benign", ("other", "x_only"), 5
SINGLE_H, SINGLE_STYLE, SINGLE_ALTS = 8, "do", ("other", "x_only")
TIE_H = 1
