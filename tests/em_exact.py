"""The EMASE Model-4 EM in exact or 60-digit arithmetic, standard library only: the reference that oracle/em_oracle.py
(float64) and the device are both held to on the small inputs of tests/em_tiny_cases.py.

Input is a list of (row, [(locus, mask), ...]): bit h of `mask` = the read aligns to haplotype h of the locus.  Storage is
a dict per read, theta a dict of its non-zero elements, so R or L of 65,537 with four entries costs four entries.  The
arithmetic knows nothing about float64: `number` is decimal.Decimal (under a 60-digit context) or fractions.Fraction (no
rounding at all), both through the same code; floats enter by exact conversion and leave through float().

What it restates (oracle/em_oracle.py names the reference's lines):
    prepare     every stored value 1, normalised per read, summed per (haplotype, locus) with the read's count, divided by
                the effective length; a pseudocount is added to every haplotype of a locus that has any non-zero value,
                then the whole is scaled back to the total it had before
    step        value = theta, normalised per read (the posterior), summed as above (the expected counts), divided by the
                effective length
    err_sum     sum over the loci of |curr - prev|, both the per-locus totals of theta scaled to a sum of 1e6
"""
from decimal import Context, Decimal, localcontext
from fractions import Fraction

DIGITS = 60
_CTX = Context(prec=DIGITS)


class ZeroAbundance(ArithmeticError):
    """A read whose alignments all have zero abundance, or a theta without any: where numpy raises FloatingPointError."""


class ExactEM:
    def __init__(self, R, L, H, rows, count=None, eff_len=None, allowed=None, number=Decimal):
        """count: per-row sequence or None; eff_len: indexable [h][l] or None; allowed: per-locus haplotype bits or None
        (the `-G` mask: a masked entry is dropped from the structure)."""
        assert number in (Decimal, Fraction)
        self.R, self.L, self.H, self.num = int(R), int(L), int(H), number
        self.eff_len = eff_len
        self.count = {}
        self.reads = {}                     # row -> sorted [(locus, hap)]
        for r, pairs in rows:
            r = int(r)
            assert 0 <= r < self.R and r not in self.reads
            ent = []
            for l, m in sorted((int(l), int(m)) for l, m in pairs):
                assert 0 <= l < self.L and 0 < m < (1 << self.H)
                if allowed is not None:
                    m &= int(allowed[l])
                ent += [(l, h) for h in range(self.H) if (m >> h) & 1]
            assert len(set(ent)) == len(ent), "repeated (row, locus) pair"
            if ent:
                self.reads[r] = ent
                self.count[r] = number(1) if count is None else self._exact(count[r])
        self.values = {}                    # row -> [value per entry], in the order of self.reads[row]
        self.theta = {}                     # (hap, locus) -> non-zero value
        self.err_history = []

    # ---- number handling ------------------------------------------------------------------------------------------------
    def _exact(self, x):
        if isinstance(x, (Decimal, Fraction)):
            return self.num(x)
        x = float(x)
        return self.num(int(x)) if x == int(x) else self.num(x)       # Decimal(float) / Fraction(float) are exact

    def _len(self, h, l):
        return self._exact(self.eff_len[h][l])

    @property
    def num_entries(self):
        return sum(len(e) for e in self.reads.values())

    # ---- the three primitives ---------------------------------------------------------------------------------------------
    def _normalize_rows(self):
        for r, vals in self.values.items():
            den = sum(vals, self.num(0))
            if den == 0:
                raise ZeroAbundance(f"row {r}: every alignment has zero abundance")
            self.values[r] = [v / den for v in vals]

    def _column_totals(self):
        tot = {}
        for r, ent in self.reads.items():
            c = self.count[r]
            for (l, h), v in zip(ent, self.values[r]):
                tot[(h, l)] = tot.get((h, l), self.num(0)) + c * v
        return tot

    def _theta_from_values(self):
        tot = self._column_totals()
        if self.eff_len is not None:
            tot = {(h, l): v / self._len(h, l) for (h, l), v in tot.items()}
        self.theta = {k: v for k, v in tot.items() if v != 0}

    def _locus_totals_1e6(self):
        per_locus = {}
        for (h, l), v in self.theta.items():
            per_locus[l] = per_locus.get(l, self.num(0)) + v
        total = sum(per_locus.values(), self.num(0))
        if total == 0:
            raise ZeroAbundance("theta has no non-zero element")
        scale = self.num(1000000) / total
        return {l: v * scale for l, v in per_locus.items()}

    # ---- the EM -----------------------------------------------------------------------------------------------------------
    def prepare(self, pseudocount=0.0):
        with localcontext(_CTX):
            self.values = {r: [self.num(1)] * len(ent) for r, ent in self.reads.items()}
            self._normalize_rows()
            self._theta_from_values()
            pc = self._exact(pseudocount)
            if pc > 0 and self.theta:
                before = sum(self.theta.values(), self.num(0))
                for l in {l for _, l in self.theta}:
                    for h in range(self.H):
                        self.theta[(h, l)] = self.theta.get((h, l), self.num(0)) + pc
                scale = before / sum(self.theta.values(), self.num(0))
                self.theta = {k: v * scale for k, v in self.theta.items()}
            self.err_history = []
        return self

    def set_theta(self, theta):
        """theta: dict (hap, locus) -> number, as self.theta."""
        self.theta = {k: self.num(v) for k, v in theta.items() if v != 0}

    def step(self, n=1):
        with localcontext(_CTX):
            for _ in range(n):
                zero = self.num(0)
                self.values = {r: [self.theta.get((h, l), zero) for l, h in ent] for r, ent in self.reads.items()}
                self._normalize_rows()
                self._theta_from_values()
        return self

    def run(self, max_iters):
        """max_iters steps with the stopping-rule sum of each (tol = 0: the rule never stops a run early)."""
        with localcontext(_CTX):
            self.err_history = []
            for _ in range(max_iters):
                prev = self._locus_totals_1e6()
                self.step()
                curr = self._locus_totals_1e6()
                zero = self.num(0)
                self.err_history.append(sum((abs(curr.get(l, zero) - prev.get(l, zero)) for l in set(prev) | set(curr)),
                                            zero))
        return self

    def expected_counts(self):
        """dict (hap, locus) -> expected read count of the last E-step (of prepare's uniform split before any step)."""
        with localcontext(_CTX):
            return {k: v for k, v in self._column_totals().items() if v != 0}

    def posterior(self):
        """dict (row, locus, hap) -> posterior of the entry in the last E-step."""
        return {(r, l, h): v for r, ent in self.reads.items() for (l, h), v in zip(ent, self.values[r])}


def max_relative_difference(a, b):
    """Largest |a - b| / |b| over the keys of two dicts of numbers (a key only one has counts as 0 there), as a float;
    0 where both are zero, infinite where only b is."""
    worst = 0.0
    for k in set(a) | set(b):
        x, y = Fraction(a.get(k, 0)), Fraction(b.get(k, 0))      # exact for a Decimal too
        if x == y:
            continue
        if y == 0:
            return float("inf")
        worst = max(worst, float(abs((x - y) / y)))
    return worst
