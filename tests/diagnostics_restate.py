"""numpy restatement of `gbrs reconstruct --diagnostics` (gbrs_hmm_diagnostics, gbrs_hmm_pair_posterior).

One (sample, chromosome) with n genes and S states; alpha, beta, gamma are (S x n), E is the (n x S) log emission,
T[i][to][from] the log table that leads from gene i to gene i + 1 (only T[0 .. n-2] are read), iv the prior, ch the
founder-change table.  An entry of -inf carries weight 0.

    interval i -> i + 1, k the state at gene i, j at gene i + 1:
        lx[k][j] = alpha[k][i] + T[i][j][k] + E[i+1][j] + beta[j][i+1]
        m = max lx,  x = exp(lx - m),  xi_i[k][j] = x[k][j] / sum x
        xo[i] = sum x * ch / sum x,  pswitch[i] = sum_{k != j} x / sum x   (the off-diagonal terms added, not 1 - diagonal)
    gene i:
        lse(v) = max v + log sum exp(v - max v)
        errlod[i] = (lse(iv + E[i]) - (lse(alpha[:,i] + beta[:,i]) - lse(alpha[:,i] - E[i] + beta[:,i]))) / ln 10
        maxmarg[i] = the first index of the largest gamma[:, i],  maxprob[i] = that value
"""
import numpy as np

from sim_geno_restate import change_table      # noqa: F401  (S x S) by brute force on multisets


def init_vec(H):
    """The reference's init_vec: log(1 / H^2) for a homozygous diplotype, log(2 / H^2) for a heterozygous one."""
    return np.log(np.array([(1.0 if a == b else 2.0) / (H * H) for a in range(H) for b in range(a, H)]))


def founders(S):
    return int(round((np.sqrt(8 * S + 1) - 1) / 2))


def weights(lx):
    """(x, sum x) of one array of log terms: x = exp(lx - max lx), 0 where lx is -inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(np.isneginf(lx), 0.0, np.exp(lx - lx.max()))
    return x, x.sum()


def lse(v, axis=0):
    """max v + log sum exp(v - max v) along `axis`, -inf entries carrying weight 0."""
    v = np.asarray(v, dtype=np.float64)
    m = v.max(axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(np.isneginf(v), 0.0, np.exp(v - m))
        return (m + np.log(x.sum(axis=axis, keepdims=True))).squeeze(axis=axis)


def pair_terms(alpha, beta, E, T, i):
    """lx[k][j] of the interval i -> i + 1."""
    with np.errstate(invalid="ignore"):
        return alpha[:, i][:, None] + T[i].T + E[i + 1][None, :] + beta[:, i + 1][None, :]


def pairs(alpha, beta, E, T, ch=None):
    """(xi (n-1 x S x S), xo (n-1), pswitch (n-1)) in one pass over the intervals."""
    S, n = alpha.shape
    ch = change_table(founders(S)) if ch is None else ch
    off = ~np.eye(S, dtype=bool)
    m = max(n - 1, 0)
    xi, xo, pswitch = np.zeros((m, S, S)), np.zeros(m), np.zeros(m)
    for i in range(n - 1):
        x, total = weights(pair_terms(alpha, beta, E, T, i))
        with np.errstate(invalid="ignore", divide="ignore"):
            xi[i] = x / total
            xo[i] = (x * ch).sum() / total
            pswitch[i] = x[off].sum() / total
    return xi, xo, pswitch


def pair_posterior(alpha, beta, E, T):
    """xi (n-1 x S x S)."""
    return pairs(alpha, beta, E, T)[0]


def crossovers(alpha, beta, E, T, ch=None):
    """(xo, pswitch), each (n-1)."""
    return pairs(alpha, beta, E, T, ch)[1:]


def error_lod(alpha, beta, E, iv=None):
    """errlod (n)."""
    S, n = alpha.shape
    iv = init_vec(founders(S)) if iv is None else iv
    with np.errstate(invalid="ignore"):
        without = np.where(np.isneginf(alpha), -np.inf, alpha - E.T + beta)
    return (lse(iv[:, None] + E.T) - (lse(alpha + beta) - lse(without))) / np.log(10.0)


def most_likely(gamma):
    """(maxmarg int32 (n), maxprob (n))."""
    at = gamma.argmax(axis=0)
    return at.astype(np.int32), gamma[at, np.arange(gamma.shape[1])]


def expressed(rows, expr_threshold=1.5):
    """The emission's own test on (n x H) TPM rows: the founders' TPMs added left to right are not below the threshold."""
    return np.array([not (sum(r) < expr_threshold) for r in np.asarray(rows, dtype=np.float64)], dtype=bool)


def all_of(res_c, T, ch=None, iv=None):
    """Every quantity, `xi` included, from one chromosome's dict of arrays (alpha, beta, eprob, gamma)."""
    xi, xo, pswitch = pairs(res_c["alpha"], res_c["beta"], res_c["eprob"], T, ch)
    maxmarg, maxprob = most_likely(res_c["gamma"])
    return dict(xi=xi, xo=xo, pswitch=pswitch, errlod=error_lod(res_c["alpha"], res_c["beta"], res_c["eprob"], iv),
                maxmarg=maxmarg, maxprob=maxprob)
