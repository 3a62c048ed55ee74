"""numpy restatement of the bootstrap draw of `gbrs quantify --bootstrap`, bit for bit:

    w(b, r) = sum over k = 0 .. c_r - 1 of P(u(b, r, k))

c_r = count[r] (1 without a count vector); u(b, r, k) = word k mod 4 of Philox4x32-10 with counter
(r & 0xFFFFFFFF, r >> 32, k div 4, b) and key (seed & 0xFFFFFFFF, seed >> 32); P(u) = the number of j with u >= T[j],
T[j] = floor(2^32 * sum_{i <= j} e^-1 / i!) for j = 0 .. 12 - a Poisson(1) deviate by inversion on integers.

A replicate IS the quantification of the file in which row r occurs w(b, r) times: restate_input() drops the entries of
every row with w = 0 and sets count = w.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key bumps
MASK32 = 0xFFFFFFFF

THRESHOLDS = np.array([1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
                       4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295], dtype=np.uint64)


def thresholds_from_formula(digits=60):
    """T[0..12] from the formula, evaluated with `digits`-digit decimals."""
    from decimal import Decimal, getcontext
    getcontext().prec = digits
    e_inv = Decimal(-1).exp()
    out, cum, fact = [], Decimal(0), Decimal(1)
    for j in range(13):
        if j > 0:
            fact *= j
        cum += e_inv / fact
        out.append(int((cum * (1 << 32)).to_integral_value(rounding="ROUND_FLOOR")))
    return out


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape; key: two scalars.  Returns four uint64 arrays < 2^32."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)            # < 2^64: exact in uint64
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def poisson1(u):
    """P(u): the number of thresholds u reaches."""
    return np.searchsorted(THRESHOLDS, np.asarray(u, dtype=np.uint64), side="right").astype(np.int64)


def weights(seed, b, num_rows, count=None):
    """int64[R]: w(b, r) for every row of the file."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & MASK32, seed >> 32)
    R = int(num_rows)
    c = np.ones(R, dtype=np.int64) if count is None else np.asarray(count).astype(np.int64)
    assert c.shape == (R,) and (c >= 0).all()
    n_blocks = (c + 3) // 4
    row = np.repeat(np.arange(R, dtype=np.int64), n_blocks)
    first = np.concatenate(([0], np.cumsum(n_blocks)))[:-1]
    k4 = np.arange(len(row), dtype=np.int64) - np.repeat(first, n_blocks)
    words = philox4x32_10((row & MASK32, row >> 32, k4, np.full(len(row), int(b) & MASK32, dtype=np.int64)), key)
    left = c[row] - 4 * k4                    # draws of this block that count: 1 .. 4, or more
    w = np.zeros(R, dtype=np.int64)
    for j in range(4):
        np.add.at(w, row, np.where(left > j, poisson1(words[j]), 0))
    return w


def restate_input(indptr, indices, w):
    """The file in which row r occurs w[r] times: (indptr, indices, count) with the entries of every zero-weight row
    dropped and count = w."""
    w = np.asarray(w)
    new_ptr, new_idx = [], []
    for ptr, idx in zip(indptr, indices):
        ptr = np.asarray(ptr, dtype=np.int64)
        idx = np.asarray(idx, dtype=np.int64)
        keep = w[idx] > 0
        col = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        kept = np.bincount(col[keep], minlength=len(ptr) - 1)
        new_ptr.append(np.concatenate(([0], np.cumsum(kept))).astype(np.uint32))
        new_idx.append(idx[keep].astype(np.uint32))
    return new_ptr, new_idx, w.astype(np.float64)
