"""The two-state (binary character) model, its closed form and binary test problems.

A helper module of the two-state tests (tests/test_twostate_reference.py on the CPU,
tests/test_gpu_twostate.py and tests/test_gpu_categories.py on the device).

* ``TwoState(pi0)``: a ``substitution_models.Model`` like every other -- Q through
  ``compute_q_matrix``, the eigen-system through ``get_eigen`` -- so it has ``p``,
  ``p_derivative`` and ``engine_eigen``.
* The closed form, independent of any eigen code.  With pi = (pi0, pi1) and Q scaled to one
  expected change per unit time, mu = 1 / (2 pi0 pi1) and

      P_ij(t) = pi_j + (delta_ij - pi_j) e^{-mu t} = delta_ij + (delta_ij - pi_j) expm1(-mu t)

  (the second form keeps the off-diagonal entries of a very short branch to full relative
  precision), P' = -mu (delta_ij - pi_j) e^{-mu t} and P'' = mu^2 (delta_ij - pi_j) e^{-mu t}.
* ``binary_problem``: a tree and a simulated alignment coded through
  ``alignment.code_table(BINARY)``, with gaps.
"""
import numpy as np

from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.synthetic import make_problem


class TwoState(SM.Model):
    """Reversible two-state model with frequencies (pi0, 1 - pi0)."""
    _name = "TwoState"
    _size = 2
    _states = ["0", "1"]

    def __init__(self, pi0=0.3):
        SM.Model.__init__(self)
        self._freqs = SM.check_frequencies([pi0, 1.0 - pi0], 2)
        self._rates = np.ones((2, 2)) - np.eye(2)
        self._q_mtx = SM.compute_q_matrix(self._rates, self._freqs)
        self.eigen = SM.Eigen(*SM.get_eigen(self._q_mtx, self._freqs))


# ---------------------------------------------------------------- closed form
def closed_mu(pi0):
    return 1.0 / (2.0 * pi0 * (1.0 - pi0))


def closed_p(pi0, t, rates=(1.0,), order=0):
    """d^order/dt^order P(t r) for every rate r -> [C][2][2] (order 0, 1, 2)."""
    pi = np.array([pi0, 1.0 - pi0])
    d = np.eye(2) - pi[None, :]  # delta_ij - pi_j
    mu = closed_mu(pi0)
    out = []
    for r in np.asarray(rates, dtype=np.float64):
        x = -mu * r * t
        if order == 0:
            out.append(np.eye(2) + d * np.expm1(x))
        elif order == 1:
            out.append(-mu * r * d * np.exp(x))
        elif order == 2:
            out.append((mu * r) ** 2 * d * np.exp(x))
        else:
            raise ValueError("order must be 0, 1 or 2")
    return np.stack(out)


def closed_site_derivs(pi0, x, y, t, rates=(1.0,), weights=(1.0,)):
    """Two taxa joined by a path of length t, tip vectors x, y [S][2]: per site
    (L, dL/dt, d2L/dt2) of L = sum_c w_c sum_i pi_i x_i sum_j P_ij(t r_c) y_j -> [3][S]."""
    pi = np.array([pi0, 1.0 - pi0])
    w = np.asarray(weights, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    return np.stack([np.einsum("c,i,si,cij,sj->s", w, pi, x, closed_p(pi0, t, rates, k), y)
                     for k in range(3)])


def closed_two_taxon_site_lnl(pi0, x, y, ta, tb, rates=(1.0,), weights=(1.0,)):
    """Sitewise lnL of (a:ta,b:tb); -- reversibility makes it a function of ta + tb."""
    return np.log(closed_site_derivs(pi0, x, y, ta + tb, rates, weights)[0])


def closed_two_taxon_derivs(pi0, x, y, t, rates=(1.0,), weights=(1.0,), site_weights=None):
    """(lnL, dlnL/dt, d2lnL/dt2) summed over sites, of the two-taxon tree at path length t."""
    f0, f1, f2 = closed_site_derivs(pi0, x, y, t, rates, weights)
    sw = np.ones(len(f0)) if site_weights is None else np.asarray(site_weights, dtype=np.float64)
    return (float(np.dot(sw, np.log(f0))), float(np.dot(sw, f1 / f0)),
            float(np.dot(sw, (f2 * f0 - f1 * f1) / (f0 * f0))))


# ---------------------------------------------------------------- problems
BIN_TABLE, BIN_LUT = A.code_table(A.BINARY)
GAP = int(np.where(BIN_TABLE.all(axis=1))[0][0])
# code of state k's one-hot vector
STATE_CODE = np.array([int(np.where((BIN_TABLE == np.eye(2)[k]).all(axis=1))[0][0])
                       for k in range(2)], dtype=np.uint8)


def binary_problem(n_taxa, n_sites, pi0=0.3, rates=(1.0,), seed=0, ambiguous=True, lo=0.01,
                   hi=0.3, gap_taxon=True):
    """(tree, names, codes uint8 [n_taxa][S], table [n_codes][2], tip_vectors {name: [S][2]}):
    synthetic.make_problem under TwoState(pi0), the states re-coded through
    code_table(BINARY).  ambiguous: about 10 % of the cells become the gap code, column S // 2
    is all gaps (S > 1) and so is taxon 1 (more than two taxa; gap_taxon=False leaves it
    out for the optimisers, to which the length of that taxon's branch is arbitrary)."""
    tree, names, states = make_problem(n_taxa, n_sites, TwoState(pi0), rates, seed=seed, lo=lo,
                                       hi=hi)
    codes = STATE_CODE[states]
    if ambiguous:
        rng = np.random.default_rng(seed + 7919)
        codes[rng.random(codes.shape) < 0.1] = GAP
        if n_sites > 1:
            codes[:, n_sites // 2] = GAP
        if n_taxa > 2 and gap_taxon:
            codes[1] = GAP
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    table = BIN_TABLE.copy()
    return tree, names, codes, table, {n: table[codes[i]] for i, n in enumerate(names)}


def all_gap_columns(codes):
    return (np.asarray(codes) == GAP).all(axis=0)
