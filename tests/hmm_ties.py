"""Helpers of the Viterbi tie tests (tests/test_hmm_ties_cpu.py, tests/test_hmm_ties_gpu.py, oracle/gen_golden.py).

A genotype call is an argmax over `delta[:, i] + T[i][next state]` (gbrs_utils.py:586-596).  Where two candidates are
bit-identical - transition tables that are exactly symmetric under founder relabelling, genes under the expression
threshold whose emission is the prior - np.argmax's first-index rule decides the call, and where they differ by less
than the error of the values they are taken from, rounding decides it.  The helpers here classify the decisions of a
path and accept, for a device path, every candidate of such a decision and nothing else."""
from itertools import combinations_with_replacement

import numpy as np

from conftest import viterbi_decision_margins  # noqa: F401  (re-exported: the tests compare decision_table with it)


def slack(v):
    """What two candidates of one decision may be off by, together: the suite's own delta tolerance (rtol=1e-9,
    atol=1e-9 throughout tests/test_hmm_gpu.py) applied to each of the two."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.abs(v[np.isfinite(v)])
    return 2.0 * (1e-9 + 1e-9 * (fin.max() if fin.size else 0.0))


def decisions(T, delta, states):
    """The candidate vectors of every argmax along `states` (the ordered path as the reference stores it: one entry
    per backtrace step plus the final state), last column first: [(chosen state, v), ...]."""
    S, n = delta.shape
    m = min(n, len(T))
    states = np.asarray(states)
    assert len(states) == m + 1, (len(states), m)
    out = [(int(states[m]), delta[:, n - 1])]
    for i in reversed(range(m)):
        out.append((int(states[i]), delta[:, i] + T[i][int(states[i + 1])]))
    return out


def decision_table(T, delta, states):
    """(margin, slack) arrays over the decisions of `states`: best minus second-best candidate, and slack(v)."""
    margins, slacks = [], []
    for _, v in decisions(T, delta, states):
        top = np.sort(v)[::-1]
        margins.append(top[0] - top[1] if len(v) > 1 else np.inf)
        slacks.append(slack(v))
    return np.asarray(margins), np.asarray(slacks)


def assert_path_eps_optimal(T, delta_ref, states_dev, err_msg=""):
    """Every step of the device's path takes a candidate that is within slack(v) of the best one, where v is formed
    from the REFERENCE's delta and the DEVICE's successor state.  Where the reference's margin exceeds the slack this is
    equality with the reference's decision; where it does not, any of the tied candidates passes and nothing else.
    Returns the number of steps at which the chosen candidate was not the first maximum (steps that used the slack)."""
    S, n = delta_ref.shape
    states_dev = np.asarray(states_dev)
    assert states_dev.min() >= 0 and states_dev.max() < S, f"{err_msg}: state out of range"
    used = 0
    for step, (s, v) in enumerate(decisions(T, delta_ref, states_dev)):
        best = v.max()
        assert v[s] >= best - slack(v), \
            f"{err_msg}: backtrace step {step} takes state {s} at {v[s]!r}, best is {int(v.argmax())} at {best!r}"
        used += int(s != int(v.argmax()))
    return used


def follow_argmax(T, delta, states, upto):
    """`states` with the entries below index `upto` replaced by the first-index argmax walk from states[upto]."""
    out = np.array(states)
    for i in reversed(range(upto)):
        out[i] = int((delta[:, i] + T[i][int(out[i + 1])]).argmax())
    return out


def founder_changes(H):
    """[S, S] number of founder changes (0, 1 or 2) between unordered pairs, best matching of the two chromosomes."""
    pairs = list(combinations_with_replacement(range(H), 2))
    S = len(pairs)
    change = np.zeros((S, S), dtype=np.int64)
    for j, (a, b) in enumerate(pairs):
        for k, (c, d) in enumerate(pairs):
            change[j, k] = min((a != c) + (b != d), (a != d) + (b != c))
    return change


def class_constant_tables(H, nt, seed, structural_zeros=True, unlinked_every=6):
    """Log transition tables [nt, S, S] whose entries are one of three numbers per interval - for 0, 1 or 2 founder
    changes - with no column normalisation, so that candidates which are symmetric in the model are bit-identical in
    floating point (the Viterbi recursion does not need stochastic columns).  Every fourth interval forbids double
    changes outright (-inf) when `structural_zeros`.  Every `unlinked_every`-th interval is between unlinked genes
    (recombination (H - 1) / H: the three numbers coincide at log(1 / H^2)), so that the backtrace meets a fresh argmax
    over symmetric states there and not at the last gene only."""
    rng = np.random.default_rng(seed)
    change = founder_changes(H)
    r = 10.0 ** rng.uniform(-15.0, -2.0, size=nt)
    T = np.empty((nt,) + change.shape)
    for i in range(nt):
        q = r[i] / max(H - 1, 1)
        two = -np.inf if structural_zeros and i % 4 == 1 else np.log(q * q)
        T[i] = np.where(change == 0, np.log((1.0 - r[i]) ** 2), np.where(change == 1, np.log(q * (1.0 - r[i])), two))
        if unlinked_every and i % unlinked_every == unlinked_every - 2:
            T[i] = np.log(1.0 / (H * H))
    return T


def symmetric_emissions(H, n, kind, seed):
    """Log emission rows [n, S] that are the prior ("prior"), symmetric in all founders but one ("one": one
    weight per number of copies of founder f, times the prior's weight of the state) or symmetric in all but two ("two":
    one weight per pair of copy numbers); about half the rows stay the prior, the distinguished founders change every
    five genes."""
    from oracle import hmm_oracle
    rng = np.random.default_rng(seed)
    iv = hmm_oracle.init_vector(H)
    pairs = list(combinations_with_replacement(range(H), 2))
    E = np.tile(iv, (n, 1))
    if kind == "prior":
        return E
    f = rng.integers(0, H, size=2)
    for i in range(n):
        if i % 5 == 0:
            f = rng.integers(0, H, size=2)
        if rng.random() < 0.5:
            continue                                            # the prior
        w = rng.uniform(-6.0, 0.0, size=(3, 3))                 # one log weight per (copies of f0, copies of f1)
        f0, f1 = int(f[0]), int(f[1]) if kind == "two" else -1
        E[i] = np.array([iv[k] + w[(a == f0) + (b == f0), (a == f1) + (b == f1)] for k, (a, b) in enumerate(pairs)])
    return E
