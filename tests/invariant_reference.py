"""The exact yardstick for rate models with an invariable class (+I, +I+G), for the tests.

Every kernel, and the oracle, builds P_c(t) = U diag(e^{lambda t r_c}) U^-1; at r_0 = 0 that is
the identity plus rounding (+-5e-16 off the diagonal, either sign), so at a variable pattern the
invariable category's vectors are noise, rescaled again and again, and F_0 takes either sign.
The device's noise and the oracle's differ and neither is the truth.  The truth is P_0 = I:

    A_0(i) = prod over the tips below of table[code][i]      (likewise every directed vector)

with every scaler 0; F_0 is then exactly 0 at a variable pattern and the masked mix (only
categories with F_c > 0 set m and take a weight: k_edge's rule) drops the category there.

``Exact(orc)`` is the oracle module with that one change: ``pmatrix`` returns the identity itself
where t r_c = 0, and the functions that call ``pmatrix`` inside the oracle (``tree_lnl``,
``edge_derivs``, ``edge_lnl``, ``pmatrix_deriv``) are restated on it.  Categories >= 1 go through
the oracle's own arithmetic untouched.  Handed to the existing restatements (nni_, support_,
ancestral_, counts_, place_ and spr_reference) in place of the oracle it yields the yardstick of
every resident-partials kernel.  ``closed_form`` is the product formula itself, which
tests/test_invariant.py holds ``Exact`` against."""
import numpy as np

import ancestral_reference as AR
import place_reference as PR
from nni_reference import eigen, state  # noqa: F401

from phylo_utils_amd import alignment as A
from phylo_utils_amd import place as PL
from phylo_utils_amd.tree import Traversal, prepare_tree


class Exact(object):
    """The oracle with P_c(t) = I exactly where t r_c = 0."""

    def __init__(self, orc):
        self._orc = orc

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def pmatrix(self, evecs, evals, ivecs, t, rates):
        P = self._orc.pmatrix(evecs, evals, ivecs, t, rates)
        for c, r in enumerate(rates):
            if t * r == 0.0:
                P[c] = np.eye(P.shape[1])
        return P

    def pmatrix_deriv(self, evecs, evals, ivecs, t, rates, order):
        if order == 0:
            return self.pmatrix(evecs, evals, ivecs, t, rates)
        return self._orc.pmatrix_deriv(evecs, evals, ivecs, t, rates, order)  # exactly 0 at r = 0

    def tree_lnl(self, tips, ops, brlens_ops, root_edge, root_len, evecs, evals, ivecs, freqs,
                 rates, weights, site_weights=None, n_nodes=None, nthreads=1, return_all=False):
        pm = lambda t: self.pmatrix(evecs, evals, ivecs, t, rates)
        P = np.array([[pm(brlens_ops[o][0]), pm(brlens_ops[o][1])] for o in range(len(ops))])
        Proot = np.stack([pm(0.0), pm(root_len)])
        return self._orc.tree_lnl_p(tips, ops, P, Proot, root_edge, freqs, weights, site_weights,
                                    n_nodes, nthreads, return_all)

    def edge_derivs(self, pa, sa, pb, sb, evecs, evals, ivecs, t, rates, weights, freqs,
                    site_weights=None):
        S, C, K = pa.shape
        sw = np.ones(S) if site_weights is None else site_weights
        mats = [np.ascontiguousarray(self.pmatrix_deriv(evecs, evals, ivecs, t, rates, k))
                for k in range(3)]
        return self._edge_derivs(pa, sa, pb, sb, mats, weights, freqs, sw)

    def _edge_derivs(self, pa, sa, pb, sb, mats, weights, freqs, sw):
        """or_edge_derivs's sums (pruning_oracle.c) in numpy, P(0) = I on the a side."""
        y = [np.einsum("cij,scj->sci", m, pb) for m in mats]
        f = [np.einsum("i,sci,sci->sc", np.asarray(freqs), pa, v) for v in y]
        live = f[0] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            lc = np.where(live, np.log(np.where(live, f[0], 1.0)) + sa + sb +
                          np.log(np.asarray(weights))[None, :], -np.inf)
            mx = lc.max(axis=1)
            e = np.where(live, np.exp(lc - mx[:, None]), 0.0)
            L = e.sum(axis=1)
            g1 = np.where(live, f[1] / np.where(live, f[0], 1.0), 0.0)
            g2 = np.where(live, f[2] / np.where(live, f[0], 1.0), 0.0)
            d1 = (e * g1).sum(axis=1) / L
            d2 = (e * g2).sum(axis=1) / L - d1 * d1
            sl = mx + np.log(L)
        sw = np.asarray(sw, dtype=np.float64)
        ok = L > 0
        if (~ok & (sw != 0)).any():
            t0 = -np.inf
        else:
            t0 = float(np.dot(sw[ok], sl[ok]))
        return np.array([t0, np.dot(sw[ok], d1[ok]), np.dot(sw[ok], d2[ok])])

    def edge_lnl(self, pa, sa, pb, sb, evecs, evals, ivecs, t, rates, weights, freqs):
        o = self._orc
        cml = np.zeros(sa.shape)
        root = o.clv(self.pmatrix(evecs, evals, ivecs, 0.0, rates),
                     self.pmatrix(evecs, evals, ivecs, t, rates), pa, pb, sa, sb, cml)
        return o.logsumexp_cats(o.lnl_node(freqs, root, cml), weights)


def closed_form(tips, tr):
    """{node: [S][K]} the product formula on the post-order orientation: a tip's table row, an
    internal node's the product of the rows of the tips below it."""
    out = {int(n): np.asarray(v, dtype=np.float64) for n, v in tips.items()}
    for p, a, b in tr.postorder_traversal:
        out[int(p)] = out[int(a)] * out[int(b)]
    return out


def invariant_site_likelihood(tips, tr, freqs):
    """[S] sum_i pi_i prod_tips table[code][i]: the invariable category's site likelihood, > 0
    exactly at the constant patterns (those that one state explains at every tip)."""
    cf = closed_form(tips, tr)
    a, b = (int(v) for v in tr.root_edge)
    return (cf[a] * cf[b]).dot(np.asarray(freqs))


# ---------------------------------------------------------------- cases
# name: (builder case of ancestral_reference, rate model).  The shapes of k_ancestral's cases
# (several tiles, a tile of one lane, an odd and an even category count, the three alphabets,
# scalers that differ between the categories on 297 edges), each with a rate-0 category
def _rm(which, alpha=0.5):
    from phylo_utils_amd.rate_models import InvariantGammaModel, InvariantSitesModel
    return InvariantSitesModel(0.3) if which == "I" else InvariantGammaModel(0.2, 3, alpha)


CASES = {
    "dna-8x65-I": ("dna-8x65-C3", "I"),
    "dna-8x65-IG3": ("dna-8x65-C3", "IG"),
    "dna-coded-14x700-I": ("dna-coded-14x700-C4", "I"),
    "dna-coded-14x700-IG3": ("dna-coded-14x700-C4", "IG"),
    "protein-8x97-IG3": ("protein-8x97-C4", "IG"),
    "binary-8x70-IG3": ("binary-8x70-Cmax", "IG"),
    "dna-caterpillar-150x130-IG3": ("dna-caterpillar-150x130-C4", "IG"),
}
QUARTET = "dna-pendant-root-4x70-IG3"  # small enough for ancestral_reference.brute_force
_ALL = dict(CASES, **{QUARTET: ("dna-pendant-root-4x70-C4", "IG")})
PENDANT = 0.05  # pendant length the sister query is simulated at


def simulate(rng, tree, model, rm, n_sites):
    """{leaf label: states [S]} down `tree` under the MIXTURE: a site's category is drawn with
    the rate model's weights (synthetic.simulate_states draws them uniformly)."""
    K, C = len(model.freqs), rm.ncat
    cats = rng.choice(C, n_sites, p=rm.weights / rm.weights.sum())
    freqs = np.asarray(model.freqs, dtype=np.float64)
    root = rng.choice(K, n_sites, p=freqs / freqs.sum())
    out, stack = {}, [(c, root) for c in tree.seed_node.children]
    while stack:
        node, parent = stack.pop()
        P = model.p(node.edge_length, rm.rates)  # [C][K][K]
        cum = np.cumsum(P, axis=2)[cats, parent]
        u = rng.random(n_sites)[:, None] * cum[:, -1:]
        st = np.minimum((u > cum).sum(axis=1), K - 1).astype(np.int64)
        st = np.where(rm.rates[cats] == 0.0, parent, st)
        if node.children:
            stack.extend((c, st) for c in node.children)
        else:
            out[node.label] = st
    return out


def problem(case):
    """ancestral_reference.problem's dict with the rate model swapped for the +I model, the data
    simulated anew under it (so that constant patterns occur) through the alphabet's own code
    table, an ambiguity code and a gap placed in one constant and one variable column, pattern
    weights 1..3 with zeros, and place_reference's query dict: a "copy" of a tip, a "sister"
    simulated on a pendant branch at an internal edge, and an all-"gap" query."""
    base, which = _ALL[case]
    prob = dict(AR.problem(base))
    kind = AR.CASES[base][0]
    rm = prob["rm"] = _rm(which, 0.8 if kind == "protein" else 0.5)
    rng = np.random.default_rng(23)
    tree = prepare_tree(prob["tree"])
    tr = Traversal(tree)
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    node = {i: n for n, i in tr.node_dict.items()}
    below = [(int(r[3]), int(r[4])) for r in tr.optimising_traversal[1:]
             if r[3] >= 0 and node[int(r[3])].parent is not tree.seed_node]
    inner = [x for x in below if x[0] in internal] or below  # the quartet has tip edges only
    nod, par = inner[len(inner) // 2]
    clade = frozenset(x.label for x in node[nod].leaves())
    aug = PL.attach(tree, PR._clade_edge(tree, clade), "q1", PENDANT)
    S = prob["codes"].shape[1]
    sts = simulate(rng, aug, prob["model"], rm, S)
    states = np.array([sts[n] for n in prob["names"]], dtype=np.int64)
    table, _ = A.code_table({"binary": A.BINARY, "protein": A.PROTEIN}.get(kind, A.DNA))
    table = np.ascontiguousarray(table, dtype=np.float64)
    K = table.shape[1]
    one_hot = np.array([int(np.flatnonzero((table == np.eye(K)[i]).all(axis=1))[0])
                        for i in range(K)], dtype=np.uint8)
    gap = int(np.flatnonzero((table == 1.0).all(axis=1))[0])
    holds = [[c for c in range(len(table)) if table[c, i] == 1.0 and table[c].sum() > 1]
             for i in range(K)]
    codes = one_hot[states]
    weights = rng.integers(1, 4, size=S).astype(np.float64)
    weights[rng.random(S) < 0.1] = 0.0
    const = (states == states[0]).all(axis=0)
    # an ambiguity code that holds the state and a gap, in the first constant and the first
    # variable column of non-zero weight (the constant one stays constant)
    narrow = [[c for c in h if table[c].sum() < K] for h in holds]  # not the gap's equals
    for cols in (np.flatnonzero(const & (weights > 0)), np.flatnonzero(~const & (weights > 0))):
        col = next((c for c in cols if narrow[states[0, c]]), cols[0])
        codes[0, col] = (narrow[states[0, col]] or holds[states[0, col]])[0]
        codes[1, col] = gap
    t = int(rng.integers(len(prob["names"])))
    q = np.stack([codes[t], one_hot[sts["q1"]], np.full(S, gap, dtype=np.uint8)])
    prob.update(codes=codes, table=table, weights=weights, compact=True, kinds=["copy", "sister",
                                                                               "gap"],
                planted={0: prob["names"][t], 1: (nod, par)},
                queries=dict(names=["q0", "q1", "q2"], codes=np.ascontiguousarray(q),
                             table=table, site_pattern=None, site_weight=weights))
    return prob


def setting(prob):
    """(traversal, eigen dict, tips {node: [S][K]}) of a problem."""
    tr = Traversal(prepare_tree(prob["tree"]))
    e = eigen(prob["model"], prob["rm"])
    tips = {tr.names[n]: prob["table"][prob["codes"][i]] for i, n in enumerate(prob["names"])}
    return tr, e, tips


def without_category_0(e):
    """The eigen dict of the mixture with the invariable category dropped and the weights of the
    others kept as they are (not renormalised): what a kernel that lost the category computes."""
    return dict(e, rates=e["rates"][1:], weights=e["weights"][1:])


def analytic_edge_derivs(x, P, S, n, o, t, e, sw):
    """(lnL, dlnL/dt, d2lnL/dt2) of the edge (n, o) at length t on the yardstick's partials, from
    the analytic form: L_s = sum_c w_c e^{sigma_c - m} F_c(t) over the categories with F_c > 0,
    F_c' and F_c'' with r_c Q P_c and (r_c Q)^2 P_c -- both exactly 0 for the invariable
    category, which adds its constant F_0 to L_s alone."""
    mats = [x.pmatrix_deriv(e["evecs"], e["evals"], e["ivecs"], t, e["rates"], k) for k in range(3)]
    f = [np.einsum("i,sci,cij,scj->sc", e["freqs"], P[n], m, P[o]) for m in mats]
    sigma = S[n] + S[o]
    live = f[0] > 0
    m = np.where(live, sigma, -np.inf).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        we = np.where(live, e["weights"][None, :] * np.exp(sigma - m[:, None]), 0.0)
        L, L1, L2 = ((we * v).sum(axis=1) for v in f)
        use = np.asarray(sw) != 0
        lnl = float(np.dot(sw[use], (m + np.log(L))[use]))
        d1 = float(np.dot(sw[use], (L1 / L)[use]))
        d2 = float(np.dot(sw[use], (L2 / L - (L1 / L) ** 2)[use]))
    return lnl, d1, d2


FIT_SEED = 3  # a seed at which tests/test_invariant.py finds the oracle's maximum over (pinvar,
              # alpha) well inside (0, 1)


def fit_problem():
    """8 taxa x 700 sites simulated under GTR + I + G3 at pinvar 0.2, alpha 0.5."""
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import InvariantGammaModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, random_tree
    rng = np.random.default_rng(FIT_SEED)
    m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), InvariantGammaModel(0.2, 3, 0.5)
    tree = random_tree(rng, 8, lo=0.05, hi=0.3)
    sts = simulate(rng, tree, m, rm, 700)
    names = sorted(sts, key=lambda s: int(s[1:]))
    codes = np.array([sts[n] for n in names], dtype=np.uint8)
    return dict(tree=tree, names=names, codes=codes, table=np.eye(4), model=m, rm=rm,
                weights=np.ones(700), compact=True)
