"""The data log-likelihood restated on the oracle: per chromosome -forward(T, E, init)[1].sum(), the reference's
alpha_scaler (gbrs_utils.py:500-526) added up.  Imports the oracle; computed once per argument set, read-only."""
import functools

import numpy as np

import grid_cases
import loglik_cases as cases


def loglik(T, E, init_vec):
    from oracle import hmm_oracle
    with np.errstate(divide="ignore"):
        return -float(hmm_oracle.forward(T, E, init_vec)[1].sum())


@functools.lru_cache(maxsize=None)
def per_chromosome(H, style, sample, name="base"):
    """float64 (n_chrom,): the sample's log-likelihood under candidate `name` of problem (H, style), on the oracle's own
    emissions."""
    from oracle import hmm_oracle
    res, _ = grid_cases.oracle_arrays(H, style, sample)
    iv = hmm_oracle.init_vector(H)
    out = np.array([loglik(T, res[c]["eprob"], iv) for c, T in zip(grid_cases.CHROMS, cases.candidate(H, style, name))])
    out.setflags(write=False)
    return out


def totals(H, style, samples, names):
    """float64 (K, n): per candidate and sample the chromosomes' values added in handle order."""
    out = np.zeros((len(names), len(samples)))
    for k, name in enumerate(names):
        for j, s in enumerate(samples):
            for v in per_chromosome(H, style, s, name):
                out[k, j] = out[k, j] + v
    return out


def choose(total):
    """choose_tables restated with plain loops: (first index of the largest total, best minus second best); NaN never
    wins, all -inf selects 0 with margin 0.0, one candidate gives margin inf."""
    total = np.asarray(total, dtype=np.float64)
    picks, margins = [], []
    for col in total.T:
        vals = [(-np.inf if np.isnan(v) else float(v)) for v in col]
        best = 0
        for k, v in enumerate(vals):
            if v > vals[best]:
                best = k
        rest = [v for k, v in enumerate(vals) if k != best]
        if not rest:
            margin = np.inf
        elif vals[best] == -np.inf:
            margin = 0.0
        else:
            margin = vals[best] - max(rest)
        picks.append(best)
        margins.append(margin)
    return np.array(picks), np.array(margins)
