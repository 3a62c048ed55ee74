"""numpy restatement of the diplotype path draw of `gbrs reconstruct --sim-geno` (gbrs_hmm_sample_paths).

Sample with stream id `stream`, chromosome index c with n genes, draw d, genes i = n-1 .. 0; T[i][to][from] leads from
gene i to gene i+1:

    l_k = alpha[k][n-1] at the last gene, alpha[k][i] + T[i][z_{i+1}][k] below it, k = 0 .. S-1
    w_k = exp(l_k),  c_k = w_0 + .. + w_k,  t = u * c_{S-1}
    z_i = the smallest k with c_k > t;  no such k by rounding: the largest k with w_k > 0;
          c_{S-1} zero or not finite: the first argmax of l_k, counted as degenerate
    u   = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53, a and b the words 2 (i & 1) and 2 (i & 1) + 1 of Philox4x32-10 on the
          counter (i >> 1, c, d, stream) and the key (seed & 0xFFFFFFFF, seed >> 32)

The founder changes of a draw: 2 - |{a,b} n {c,d}| (multisets) summed over neighbouring genes.  The margin of a decision is
min_k |c_k - t| / c_{S-1}: how far, relative to the total, the threshold is from the nearest cumulative sum - a device that
adds the w_k in another association, or forms w_k as exp(alpha) * exp(T), may decide otherwise only where it is tiny.
"""
import collections
import itertools

import numpy as np

from bootstrap_restate import MASK32, philox4x32_10


def u_from_words(a, b):
    """The uniform of two 32-bit words: 53 bits, in [0, 1)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    top = ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64)   # < 2^53: exact
    return top * 2.0 ** -53


def uniforms(seed, stream, chrom, n_genes, n_draws):
    """float64 (n_draws x n_genes): u of every (draw, gene) of one (sample stream, chromosome)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(n_genes, dtype=np.int64)[None, :]
    d = np.arange(n_draws, dtype=np.int64)[:, None]
    shape = (n_draws, n_genes)
    words = philox4x32_10((np.broadcast_to(i >> 1, shape), np.full(shape, int(chrom)), np.broadcast_to(d, shape),
                           np.full(shape, int(stream) & MASK32)), (seed & MASK32, seed >> 32))
    odd = np.broadcast_to((i & 1) == 1, shape)
    return u_from_words(np.where(odd, words[2], words[0]), np.where(odd, words[3], words[1]))


def pick(logw, u):
    """One decision per row of logw (K x S) with the uniforms u (K): (states, margins, degenerate flags)."""
    logw = np.asarray(logw, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = np.exp(logw)
        c = np.cumsum(w, axis=1)                       # c_k in state order, one addition after the other
        total = c[:, -1]
        t = u * total
        above = c > t[:, None]
        z = above.argmax(axis=1)
        none = ~above.any(axis=1)
        last_positive = w.shape[1] - 1 - (w[:, ::-1] > 0).argmax(axis=1)
        z = np.where(none, last_positive, z)
        degenerate = ~((total > 0) & np.isfinite(total))
        z = np.where(degenerate, logw.argmax(axis=1), z)
        margin = np.abs(c - t[:, None]).min(axis=1) / total
    return z.astype(np.int64), margin, degenerate


def change_table(H):
    """(S x S) founder changes between diplotypes by brute force on multisets."""
    states = [collections.Counter(p) for p in itertools.combinations_with_replacement(range(H), 2)]
    return np.array([[2 - sum((p & q).values()) for q in states] for p in states], dtype=np.int64)


def sample_paths(alpha, T, seed, stream, chrom, n_draws, table=None):
    """alpha (S x n) log forward values of one (sample, chromosome), T (n_t x S x S) log tables with n_t >= n - 1.
    Returns (paths uint8 (K x n), changes int64 (K), margins float64 (K x n), number of degenerate decisions)."""
    alpha = np.asarray(alpha, dtype=np.float64)
    S, n = alpha.shape
    K = int(n_draws)
    paths = np.zeros((K, n), dtype=np.uint8)
    margins = np.full((K, n), np.inf)
    changes = np.zeros(K, dtype=np.int64)
    if n == 0:
        return paths, changes, margins, 0
    if table is None:
        table = change_table(int(round((np.sqrt(8 * S + 1) - 1) / 2)))
    u = uniforms(seed, stream, chrom, n, K)
    degenerate = 0
    z_next = None
    for i in range(n - 1, -1, -1):
        if i == n - 1:
            logw = np.broadcast_to(alpha[:, i], (K, S))
        else:
            logw = alpha[:, i][None, :] + T[i][z_next, :]
        z, m, bad = pick(logw, u[:, i])
        paths[:, i], margins[:, i] = z, m
        degenerate += int(bad.sum())
        if z_next is not None:
            changes += table[z_next, z]
        z_next = z
    return paths, changes, margins, degenerate


def comparable(margins, floor=1e-12):
    """(bool (K x n), bool (K)): which states of a draw a device must reproduce exactly, and which draws as a whole.  A
    decision with a margin below `floor` may come out otherwise on the device, and everything the draw decides from there
    downwards then follows another path: the draw's genes above its first (highest) close decision stay comparable, the
    rest of it and its change count do not."""
    close = np.asarray(margins) < floor
    K, n = close.shape
    first = np.where(close.any(axis=1), n - 1 - close[:, ::-1].argmax(axis=1), -1)
    return np.arange(n)[None, :] > first[:, None], first < 0
