"""The likelihood path restated in 50-digit arithmetic (mpmath) -- TEST INFRASTRUCTURE ONLY.

The oracle (``oracle/oracle.py``) is an fp64 restatement of the formulas the kernels use, so a
device-versus-oracle test shows how far the two are from each other, not how far both are from
the number they are meant to compute.  This module computes that number:

* ``q_matrix``: Q assembled in mpmath from the model's exchangeabilities and frequencies, read
  as exact binary64 values, rows summing to zero and scaled to one expected substitution per unit
  time (the rule of ``substitution_models.compute_q_matrix``).  The fp64 eigen-system is not used:
  its rounding is part of what is measured.
* ``Exact.p(tau, order)``: P = expm(Q tau), P' = Q P, P'' = Q^2 P.
* ``Exact.prune``: Felsenstein pruning over an explicit schedule -- the ``ops``, lengths and root
  edge that the tests hand to ``oracle.tree_lnl`` -- with no rescaling.
* ``Exact.edge``: lnL(t), dlnL/dt and d2lnL/dt2 at any edge and any t, from the two directed
  partials of the edge with P, P' and P''.

The rate categories (rates, weights) are inputs and are taken as exact binary64 values; an
invariable category is a category of rate 0 (``rate_models.py``), for which P = I.

Only this module, tests/golden/make_golden_hp.py and tests/test_hp_reference.py import mpmath.
"""
import numpy as np
from mpmath import mp, mpf

from hp_cases import reroot

mp.dps = 50


def q_matrix(exch, freqs):
    """Q [K][K] as an mp.matrix: q_ij = exch_ij pi_j, q_ii = -sum_j q_ij, divided by
    -sum_i pi_i q_ii.  `exch` symmetric [K][K], `freqs` [K]: binary64 values, read exactly."""
    K = len(freqs)
    pi = [mpf(float(x)) for x in freqs]
    q = mp.zeros(K, K)
    for i in range(K):
        for j in range(K):
            if i != j:
                q[i, j] = mpf(float(exch[i][j])) * pi[j]
    for i in range(K):
        q[i, i] = -sum(q[i, j] for j in range(K) if j != i)
    scale = -sum(pi[i] * q[i, i] for i in range(K))
    return q / scale


def to_float(x):
    """Nearest binary64 of an mpf, a list or an mp.matrix of them (nested lists -> ndarray)."""
    if isinstance(x, mp.matrix):
        return np.array([[float(x[i, j]) for j in range(x.cols)] for i in range(x.rows)])
    if isinstance(x, (list, tuple)):
        return np.array([to_float(v) for v in x])
    return float(x)


class Exact(object):
    """One substitution model in exact arithmetic: Q, the frequencies and a memo of P(tau)."""

    def __init__(self, exch, freqs):
        self.K = len(freqs)
        self.pi = [mpf(float(x)) for x in freqs]
        self.Q = q_matrix(exch, freqs)
        self.Q2 = self.Q * self.Q
        self._memo = {}
        self._tipmemo = {}

    @classmethod
    def of_model(cls, model):
        """From a reversible ``substitution_models`` model: its symmetric exchangeabilities
        (``model.rates``) and its frequencies."""
        return cls(np.asarray(model.rates, dtype=np.float64),
                   np.asarray(model.freqs, dtype=np.float64))

    def p(self, tau, order=0):
        """d^order/dtau^order expm(Q tau) as an mp.matrix; `tau` a binary64 value or an mpf."""
        key = (mpf(tau), order)
        if key not in self._memo:
            if order == 0:
                t = mpf(tau)
                self._memo[key] = mp.eye(self.K) if t == 0 else mp.expm(self.Q * t)
            else:
                self._memo[key] = (self.Q if order == 1 else self.Q2) * self.p(tau, 0)
        return self._memo[key]

    def p_cats(self, t, rates, order=0):
        """[C] matrices d^order/dt^order P(t r_c) = r_c^order P^(order)(t r_c); `t` a binary64
        value or an mpf."""
        t = t if isinstance(t, mpf) else mpf(float(t))
        out = []
        for r in rates:
            r = mpf(float(r))
            out.append(self.p(t * r, order) * r ** order)
        return out

    # ------------------------------------------------------------------ pruning
    def _apply(self, M, v):
        K = self.K
        nz = [j for j in range(K) if v[j] != 0]
        return [sum(M[i, j] * v[j] for j in nz) for i in range(K)]

    def _apply_tip(self, tau, v):
        """P(tau) v for a tip vector of zeros and ones, remembered per (tau, v)."""
        key = (tau, tuple(int(x) for x in v))
        if key not in self._tipmemo:
            self._tipmemo[key] = self._apply(self.p(tau), [mpf(int(x)) for x in v])
        return self._tipmemo[key]

    def partials(self, tips, ops, lens, rates):
        """{node: [S][C][K]} of every internal node of the schedule; tips {node: [S][K]} of
        zeros and ones."""
        rates = [mpf(float(r)) for r in rates]
        S = len(next(iter(tips.values())))
        C, K = len(rates), self.K
        part = {}

        def side(node, length, s, c):
            tau = mpf(float(length)) * rates[c]
            if node in tips:
                return self._apply_tip(tau, tips[node][s])
            return self._apply(self.p(tau), part[node][s][c])

        for (p, c1, c2), (l1, l2) in zip(np.asarray(ops).tolist(), np.asarray(lens).tolist()):
            rows = []
            for s in range(S):
                cats = []
                for c in range(C):
                    x, y = side(c1, l1, s, c), side(c2, l2, s, c)
                    cats.append([x[i] * y[i] for i in range(K)])
                rows.append(cats)
            part[p] = rows
        return part

    def _end(self, node, tips, part, s, c):
        if node in tips:
            return [mpf(int(x)) for x in tips[node][s]]
        return part[node][s][c]

    def prune(self, tips, ops, lens, root_edge, root_len, rates, weights, site_weights=None):
        """dict(f [S][C] the likelihood of pattern s in category c, site [S] = log sum_c w_c f_c
        (-inf where the sum is exactly 0), lnl = sum_s site_weights_s site_s over the patterns of
        non-zero weight), all mpf."""
        return self.edge(tips, ops, lens, root_edge, root_len, root_edge, root_len, rates,
                         weights, site_weights, rerooted=True)

    def edge(self, tips, ops, lens, root_edge, root_len, edge, t, rates, weights,
             site_weights=None, rerooted=False, part=None):
        """The tree's likelihood as a function of the length t of `edge` = (a, b): dict(f, site,
        lnl, d1, d2) -- lnl(t), dlnl/dt, d2lnl/dt2 summed over the weighted patterns -- from the
        directed partials of a (away from b) and of b (away from a) with P, P' and P''.  `part`:
        the result of ``partials`` on the schedule rooted on `edge`, to evaluate several t."""
        if not rerooted:
            ops, lens, _ = reroot(ops, lens, root_edge, root_len, edge)
        a, b = (int(v) for v in edge)
        if part is None:
            part = self.partials(tips, ops, lens, rates)
        S = len(next(iter(tips.values())))
        C, K = len(rates), self.K
        w = [mpf(float(x)) for x in weights]
        sw = [mpf(1)] * S if site_weights is None else [mpf(float(x)) for x in site_weights]
        M = [self.p_cats(t, rates, k) for k in range(3)]
        f, site = [], []
        lnl = d1 = d2 = mpf(0)
        for s in range(S):
            fk = [[mpf(0)] * C for _ in range(3)]
            for c in range(C):
                va, vb = self._end(a, tips, part, s, c), self._end(b, tips, part, s, c)
                for k in range(3):
                    y = self._apply(M[k][c], vb)
                    fk[k][c] = sum(self.pi[i] * va[i] * y[i] for i in range(K))
            F = [sum(w[c] * fk[k][c] for c in range(C)) for k in range(3)]
            f.append(fk[0])
            site.append(mp.log(F[0]) if F[0] > 0 else mpf("-inf"))
            if sw[s] != 0:
                lnl += sw[s] * site[-1]
                if F[0] > 0:
                    d1 += sw[s] * F[1] / F[0]
                    d2 += sw[s] * (F[2] * F[0] - F[1] * F[1]) / (F[0] * F[0])
        return dict(f=f, site=site, lnl=lnl, d1=d1, d2=d2)
