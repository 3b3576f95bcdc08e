"""DESIGN 4.30 (likelihood mapping) in plain Python and numpy on top of the oracle: the
four-taxon likelihood out of ``oracle.pmatrix`` / ``oracle.pmatrix_deriv`` matrices, the optimiser
as rounds of ``oracle.newton_edge`` (the yardstick of the Newton rule, not a copy of it), the
quartet draws on tests/sim_reference.py's Philox, and the float64 finish.

The rule.  Topology tau of quartet (a, b, c, d) has tips (p, q | r, s) = (a, b | c, d), (a, c | b,
d), (a, d | b, c); lengths (l_p, l_q, l_r, l_s, l_i);
    L_s = sum_c q_c sum_i pi_i (P_c(l_p) x_p)_i (P_c(l_q) x_q)_i
                    sum_j P_c(l_i)[i][j] (P_c(l_r) x_r)_j (P_c(l_s) x_s)_j,  lnL = sum_s w_s log L_s.
One evaluation at the start; a round takes p, q, r, s, i by the Newton rule from the current
length; stop after round max_rounds or, with min_gain >= 0, when the round gained <= min_gain.
"""
import itertools
import math

import numpy as np

import sim_reference as SR
from oracle import oracle as O

TIPS = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2))  # positions of (p, q, r, s) in (a, b, c, d)
ATTRACTORS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (.5, .5, 0), (.5, 0, .5), (0, .5, .5),
              (1 / 3., 1 / 3., 1 / 3.))


class TwoState(object):
    """A reversible two-state model, Q normalised to one expected change per unit time."""
    reversible = True
    name = "TwoState"

    def __init__(self, pi0=0.3):
        pi = np.array([pi0, 1.0 - pi0])
        self.freqs = pi
        q = np.array([[-pi[1], pi[1]], [pi[0], -pi[0]]]) / (2.0 * pi[0] * pi[1])
        s = np.sqrt(pi)
        lam, u = np.linalg.eigh(s[:, None] * q / s[None, :])
        self._eig = (np.ascontiguousarray(u / s[:, None]), np.ascontiguousarray(lam),
                     np.ascontiguousarray(u.T * s[None, :]))

    def engine_eigen(self):
        return self._eig


class Model(object):
    """The eigen-system, frequencies and categories a call is given."""

    def __init__(self, substitution_model, rates, cat_weights):
        self.ev, self.el, self.iv = (np.asarray(x, dtype=np.float64)
                                     for x in substitution_model.engine_eigen())
        self.pi = np.asarray(substitution_model.freqs, dtype=np.float64)
        self.rates = np.asarray(rates, dtype=np.float64)
        self.cw = np.asarray(cat_weights, dtype=np.float64)

    def p(self, t, order=0):
        return O.pmatrix_deriv(self.ev, self.el, self.iv, t, self.rates, order)


def tip_vectors(codes, table, quartet, tau):
    """[4][S][K]: the tip vectors of (p, q, r, s)."""
    table = np.asarray(table, dtype=np.float64)
    return [table[np.asarray(codes)[quartet[k]]] for k in TIPS[tau]]


def site_terms(m, x, lens, h=None):
    """(L, L', L'') [S] each of the four-taxon tree; the derivatives in the length of edge h
    (0..4 = p, q, r, s, i; None: zeros)."""
    out = []
    for order in ((0, 1, 2) if h is not None else (0,)):
        P = [m.p(lens[e], order if e == h else 0) for e in range(5)]
        A, B, Cv, D = (np.einsum("cij,sj->sci", P[e], x[e]) for e in range(4))
        inner = np.einsum("cij,scj->sci", P[4], Cv * D)
        Lc = (m.pi[None, None, :] * A * B * inner).sum(axis=2)
        out.append(Lc.dot(m.cw))
    while len(out) < 3:
        out.append(np.zeros_like(out[0]))
    return out


def evaluate(m, x, w, lens, h=None):
    """(lnL, lnL', lnL'') in the length of edge h."""
    L, L1, L2 = site_terms(m, x, lens, h)
    w = np.ones(len(L)) if w is None else np.asarray(w, dtype=np.float64)
    live = w != 0
    if np.any(~(L[live] > 0)):
        return -np.inf, np.nan, np.nan
    L, L1, L2, w = L[live], L1[live], L2[live], w[live]
    return (float(np.dot(w, np.log(L))), float(np.dot(w, L1 / L)),
            float(np.dot(w, (L2 * L - L1 * L1) / (L * L))))


def optimise(m, x, w, t0=None, tol=1e-8, max_iter=50, max_rounds=10, min_gain=1e-6,
             with_derivs=False):
    """(row [8] = lnL, five lengths, rounds, evaluations; derivs [5][2] or None)."""
    lens = [min(max(0.1 if t0 is None else float(t0[h]), O.MIN_LEN), O.MAX_LEN) for h in range(5)]
    count = [1]
    cur = evaluate(m, x, w, lens, 0)[0]
    rounds = 0
    for r in range(1, max_rounds + 1):
        if not np.isfinite(cur):
            break
        before = cur
        for h in range(5):
            if not np.isfinite(cur):
                break

            def ev(t, h=h):
                count[0] += 1
                trial = list(lens)
                trial[h] = t
                return evaluate(m, x, w, trial, h)

            lens[h], cur, _ = O.newton_edge(ev, lens[h], tol, max_iter)
        rounds = r
        if min_gain >= 0 and cur - before <= min_gain:
            break
    row = np.array([cur] + lens + [rounds, count[0]], dtype=np.float64)
    der = None
    if with_derivs:
        der = np.full((5, 2), np.nan)
        if np.isfinite(cur):
            for h in range(5):
                der[h] = evaluate(m, x, w, lens, h)[1:]
    return row, der


def scores(codes, table, m, w, quartets, with_derivs=False, **kw):
    """out [Q][3][8] and derivs [Q][3][5][2] (or None) of a call."""
    quartets = np.asarray(quartets).reshape(-1, 4)
    out = np.zeros((len(quartets), 3, 8))
    der = np.zeros((len(quartets), 3, 5, 2)) if with_derivs else None
    for q, quartet in enumerate(quartets):
        for tau in range(3):
            row, d = optimise(m, tip_vectors(codes, table, quartet, tau), w,
                              with_derivs=with_derivs, **kw)
            out[q, tau] = row
            if with_derivs:
                der[q, tau] = d
    return out, der


def four_taxon_oracle(m, x, w, lens):
    """lnL of the explicit tree ((p, q), (r, s)) through oracle.tree_lnl: nodes 4 and 5 join the
    pairs, the root edge (4, 5) carries l_i."""
    tips = {k: x[k] for k in range(4)}
    ops = np.array([[4, 0, 1], [5, 2, 3]], dtype=np.int32)
    brlens = np.array([[lens[0], lens[1]], [lens[2], lens[3]]])
    lnl, _ = O.tree_lnl(tips, ops, brlens, (4, 5), lens[4], m.ev, m.el, m.iv, m.pi, m.rates,
                        m.cw, site_weights=w, n_nodes=6)
    return lnl


def edge_partials(m, x, lens, h):
    """(pa, pb) [S][C][K] on the two ends of edge h, for oracle.edge_derivs (P(0) on a, P(t) on
    b): b is the tip for a tip edge, the (r, s) node for the internal edge."""
    C = len(m.rates)
    P = [m.p(lens[e]) for e in range(5)]
    T = [np.einsum("cij,sj->sci", P[e], x[e]) for e in range(4)]
    if h == 4:
        return T[0] * T[1], T[2] * T[3]
    tip = np.repeat(x[h][:, None, :], C, axis=1)
    if h < 2:
        inner = np.einsum("cij,scj->sci", P[4], T[2] * T[3])
        return T[1 - h] * inner, tip
    inner = np.einsum("cji,scj->sci", P[4], T[0] * T[1] * m.pi[None, None, :]) / m.pi[None, None, :]
    return T[5 - h] * inner, tip


def edge_derivs_oracle(m, x, w, lens, h):
    pa, pb = edge_partials(m, x, lens, h)
    z = np.zeros(pa.shape[:2])
    return O.edge_derivs(pa, z, pb, z, m.ev, m.el, m.iv, lens[h], m.rates, m.cw, m.pi,
                         site_weights=w)


# ---- quartets -----------------------------------------------------------------------------------

def philox_u(seed, g, c2):
    """u of counter (g lo, g hi, c2, 3) under the 64-bit seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(g, dtype=np.uint64)
    g, c2 = np.broadcast_arrays(g, np.asarray(c2, dtype=np.uint64))
    x = SR.philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), c2, np.uint64(3)),
                         (seed & 0xFFFFFFFF, seed >> 32))
    m = ((x[1] >> np.uint64(5)) << np.uint64(26)) | (x[0] >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def draw_quartets(n, Q, seed, cluster=None):
    """int32 [min(m, Q)][4]."""
    if cluster is None:
        m = math.comb(n, 4)
        if m <= Q:
            return np.array(list(itertools.combinations(range(n), 4)), dtype=np.int32)
        u = philox_u(seed, np.arange(Q)[:, None], np.arange(4)[None, :])
        out = np.zeros((Q, 4), dtype=np.int32)
        for g in range(Q):
            chosen = []
            for k in range(4):
                v = min(int(math.floor(u[g, k] * (n - k))), n - k - 1)
                for c in sorted(chosen):
                    if c <= v:
                        v += 1
                chosen.append(v)
            out[g] = chosen
        return out
    cluster = np.asarray(cluster)
    members = [np.flatnonzero(cluster == k) for k in range(4)]
    size = [len(x) for x in members]
    m = size[0] * size[1] * size[2] * size[3]
    if m <= Q:
        return np.array(list(itertools.product(*members)), dtype=np.int32)
    u = philox_u(seed, np.arange(Q)[:, None], 4 + np.arange(4)[None, :])
    return np.array([[members[k][min(int(math.floor(u[g, k] * size[k])), size[k] - 1)]
                      for k in range(4)] for g in range(Q)], dtype=np.int32)


# ---- finish -------------------------------------------------------------------------------------

def weights(lnl3):
    """p [3] of three finite lnL."""
    M = max(lnl3)
    e = [math.exp(v - M) for v in lnl3]
    s = e[0] + e[1] + e[2]
    return [v / s for v in e]


def region7(p):
    best, arg = None, -1
    for k, a in enumerate(ATTRACTORS):
        d = sum((p[i] - a[i]) ** 2 for i in range(3))
        if best is None or d < best:
            best, arg = d, k
    return arg


def region3(p):
    return max(range(3), key=lambda i: (p[i], -i))


def boundary_margin(p):
    """The Euclidean distance from p to the nearest boundary of its region, of the seven (the
    bisector planes between its attractor and the others) and of the three (p_i = p_j)."""
    d = [sum((p[i] - a[i]) ** 2 for i in range(3)) for a in ATTRACTORS]
    k = region7(p)
    out = min((d[j] - d[k]) / (2.0 * math.sqrt(sum((ATTRACTORS[j][i] - ATTRACTORS[k][i]) ** 2
                                                   for i in range(3))))
              for j in range(7) if j != k)
    s = sorted(p)
    return min(out, (s[2] - s[1]) / math.sqrt(2.0))
