"""CPU restatement of the regraft score for the tests: the score of a move from the
directed partials of the rest tree, with transition MATRICES (``oracle.pmatrix``), not the
eigen-basis form of the kernel, and the rest tree's partials computed by ``oracle.clv`` on its
own adjacency -- no walk, no re-orientation, nothing shared with ``tree.spr_rows``.  `orc` is the
oracle module (the ``oracle_mod`` fixture)."""
import numpy as np

from nni_reference import eigen, splits, state  # noqa: F401

from phylo_utils_amd import alignment as A
from phylo_utils_amd.tree import Traversal, apply_spr, prepare_tree

# name: (kind, taxa, patterns, categories (None: the kernel's limit), coded tips).  The smallest
# shapes at which k_regraft can go wrong: a partial tile after one full tile (67 patterns), more
# than two tiles (130), one category (no mix) and four, the three alphabets, dense tips, and the
# LDS limit
CASES = {
    "binary-7x67-C4": ("binary", 7, 67, 4, True),
    "binary-7x130-Cmax": ("binary", 7, 130, None, True),
    "dna-7x67-C1": ("dna", 7, 67, 1, True),
    "dna-12x130-C4": ("dna", 12, 130, 4, True),
    "dna-dense-7x130-C4": ("dna", 7, 130, 4, False),
    "protein-7x67-C4": ("protein", 7, 67, 4, True),
    "protein-12x130-C1": ("protein", 12, 130, 1, True),
}
AMBIGUOUS = 0.08  # share of the tip cells recoded as an ambiguity or gap code


def problem(case, n_cat_max=None):
    """dict(tree, names, codes, table, model, rm, compact, weights) of a case: GTR with unequal
    frequencies (TwoState(0.3), LG), data simulated down a random tree, AMBIGUOUS of the cells
    replaced by an ambiguity or gap code of the alphabet's own table that holds the state,
    pattern weights 0..3 (zeros included)."""
    import twostate as T
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem
    kind, n_taxa, n_sites, C, compact = CASES[case]
    if C is None:
        C = n_cat_max
    rm = GammaRateModel(C, 0.8 if kind == "protein" else 0.5) if C > 1 else UniformRateModel()
    rng = np.random.default_rng(7)
    if kind == "binary":
        m = T.TwoState(0.3)
        tree, names, codes, table, _ = T.binary_problem(n_taxa, n_sites, 0.3, rm.rates, seed=3,
                                                        ambiguous=True, gap_taxon=False)
        codes = np.asarray(codes, dtype=np.uint8)
    else:
        m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if kind == "dna" else SM.LG()
        tree, names, st = make_problem(n_taxa, n_sites, m, rm.rates, seed=3)
        table, _ = A.code_table(A.DNA if kind == "dna" else A.PROTEIN)
        table = np.ascontiguousarray(table)
        K = table.shape[1]
        one_hot = [int(np.flatnonzero((table == np.eye(K)[i]).all(axis=1))[0]) for i in range(K)]
        holds = [[c for c in range(len(table)) if table[c, i] == 1.0 and table[c].sum() > 1]
                 for i in range(K)]
        codes = np.array(one_hot, dtype=np.uint8)[st.astype(np.int64)]
        for t, s in np.argwhere(rng.random(codes.shape) < AMBIGUOUS):
            opts = holds[int(st[t, s])]
            codes[t, s] = opts[int(rng.integers(len(opts)))]
    weights = rng.integers(0, 4, size=codes.shape[1]).astype(np.float64)
    weights[:3] = (0.0, 2.0, 0.0)
    return dict(tree=tree, names=names, codes=codes, table=np.asarray(table, dtype=np.float64),
                model=m, rm=rm, compact=compact, weights=weights)


def score_from(orc, e, weights, A_, sA, B_, sB, S_, sS, t, l):
    """The definition on three vectors [S][C][K] and their scalers [S][C]."""
    pm = lambda x: orc.pmatrix(e["evecs"], e["evals"], e["ivecs"], x, e["rates"])
    half, pend = pm(0.5 * t), pm(l)
    g = (e["freqs"][None, None, :] * np.einsum("cij,scj->sci", half, A_) *
         np.einsum("cij,scj->sci", half, B_) * np.einsum("cij,scj->sci", pend, S_)).sum(axis=2)
    sigma = sA + sB + sS
    live = g > 0
    m = np.where(live, sigma, -np.inf).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        we = np.where(live, e["weights"][None, :] * np.exp(sigma - m[:, None]), 0.0)
        site = m + np.log((we * g).sum(axis=1))
    w = np.asarray(weights, dtype=np.float64)
    use = w != 0
    return float(np.dot(w[use], site[use]))


class Restated(object):
    """Scores of the moves of a problem from the definition."""

    def __init__(self, orc, prob):
        self.orc, self.prob = orc, prob
        self.tree = prepare_tree(prob["tree"])
        self.tr = tr = Traversal(self.tree)
        self.e = eigen(prob["model"], prob["rm"])
        self.by_name = {n: prob["table"][prob["codes"][i]] for i, n in enumerate(prob["names"])}
        self.tips = {tr.names[n]: v for n, v in self.by_name.items()}
        self.C = len(self.e["rates"])
        self.adj = {i: {} for i in range(tr.n_nodes)}
        for (a, b), t in tr.brlens.items():
            self.adj[a][b] = float(t)
            self.adj[b][a] = float(t)

    def pm(self, t):
        e = self.e
        return self.orc.pmatrix(e["evecs"], e["evals"], e["ivecs"], t, e["rates"])

    def directed(self, adj, a, b, memo):
        """(vector [S][C][K], scaler [S][C]) at node a pointing at its neighbour b on `adj`."""
        if (a, b) in memo:
            return memo[a, b]
        if len(adj[a]) == 1:
            v = np.repeat(np.asarray(self.tips[a], dtype=np.float64)[:, None, :], self.C, axis=1)
            out = (v, np.zeros(v.shape[:2]))
        else:
            c1, c2 = [z for z in adj[a] if z != b]
            (p1, s1), (p2, s2) = self.directed(adj, c1, a, memo), self.directed(adj, c2, a, memo)
            cml = np.zeros(s1.shape)
            out = (self.orc.clv(self.pm(adj[a][c1]), self.pm(adj[a][c2]), p1, p2, s1, s2, cml),
                   cml)
        memo[a, b] = out
        return out

    def candidates(self):
        """[(n, o)]: every directed edge whose end o is internal and whose rest tree keeps at
        least two edges, in no particular order."""
        out = []
        for n in self.adj:
            for o in self.adj[n]:
                if len(self.adj[o]) == 3:
                    x, y = [z for z in self.adj[o] if z != n]
                    if len(self.adj[x]) > 1 or len(self.adj[y]) > 1:
                        out.append((n, o))
        return out

    def rest(self, n, o):
        """(adjacency of R, x, y, merged length, pendant length, {edge (u, v) sorted: distance})."""
        x, y = [z for z in self.adj[o] if z != n]
        side, todo = {n}, [n]
        while todo:
            for z in self.adj[todo.pop()]:
                if z != o and z not in side:
                    side.add(z)
                    todo.append(z)
        R = {a: {b: t for b, t in nb.items() if b != o} for a, nb in self.adj.items()
             if a != o and a not in side}
        R[x][y] = R[y][x] = self.adj[o][x] + self.adj[o][y]
        depth, todo = {x: 0, y: 0}, [x, y]
        while todo:  # breadth first from both ends of the merged edge
            nxt = []
            for a in todo:
                for b in R[a]:
                    if b not in depth:
                        depth[b] = depth[a] + 1
                        nxt.append(b)
            todo = nxt
        dist = {}
        for a in R:
            for b in R[a]:
                if a < b:
                    dist[a, b] = 0 if {a, b} == {x, y} else min(depth[a], depth[b]) + 1
        return R, x, y, R[x][y], self.adj[n][o], dist

    def ends(self, n, o, u, v, rest=None, memo=None):
        """(A, sA, B, sB, S, sS, t, l) of move (n, o, u, v): A at u pointing at v, B at v pointing
        at u on R; S at n pointing at o on the tree."""
        R, x, y, merged, l, _ = self.rest(n, o) if rest is None else rest
        memo = {} if memo is None else memo
        A_, sA = self.directed(R, u, v, memo)
        B_, sB = self.directed(R, v, u, memo)
        S_, sS = self.directed(self.adj, n, o, self._tree_memo())
        return A_, sA, B_, sB, S_, sS, R[u][v], l

    def _tree_memo(self):
        if not hasattr(self, "_memo"):
            self._memo = {}
        return self._memo

    def all_moves(self, radius=None):
        """{(n, o, u, v) with u < v: (distance, score)} of every move within `radius`."""
        out = {}
        for n, o in self.candidates():
            rest = self.rest(n, o)
            memo = {}
            for (u, v), d in rest[5].items():
                if radius is not None and d > radius:
                    continue
                out[n, o, u, v] = (d, score_from(self.orc, self.e, self.prob["weights"],
                                                 *self.ends(n, o, u, v, rest, memo)))
        return out

    def tree_lnl(self, tree):
        """The oracle's lnL of any tree on the problem's leaves."""
        tr = Traversal(prepare_tree(tree))
        e = self.e
        tips = {tr.names[n]: v for n, v in self.by_name.items()}
        return self.orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                 tr.root_length(), e["evecs"], e["evals"], e["ivecs"], e["freqs"],
                                 e["rates"], e["weights"], site_weights=self.prob["weights"],
                                 n_nodes=tr.n_nodes)[0]

    def moved_lnl(self, n, o, u, v):
        return self.tree_lnl(apply_spr(self.tree, n, o, u, v))


def key(n, o, u, v):
    """A move's key with the regraft edge's ends sorted."""
    return (int(n), int(o)) + tuple(sorted((int(u), int(v))))


# ---------------------------------------------------------------- the search fixture
# 10 taxa x 2000 DNA columns simulated down a random tree G under GTR+G4{0.5} (GTR at its default
# parameters, what `phy -m "GTR+G4{0.5}"` builds); the start tree is
# G with one subtree moved by at least 3 edges.  SEARCH_SEED is the first seed from 1 up at which
# tests/test_spr.py::test_search_precondition holds: at the start tree's lengths after one
# oracle.optimise_sweep the restatement ranks a move back to G's topology within the top KEEP
# pruned subtrees.
SEARCH_SEED = 1
SEARCH_TAXA, SEARCH_SITES, KEEP = 10, 2000, 5


def search_problem(seed=None):
    """dict(G, start, move, model, rm): the generating tree, the start tree and the move (n, o,
    u, v, distance) that made it."""
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import random_tree
    from phylo_utils_amd.tree import spr_rows
    seed = SEARCH_SEED if seed is None else seed
    rng = np.random.default_rng(seed)
    G = prepare_tree(random_tree(rng, SEARCH_TAXA, 0.03, 0.25))
    moves = spr_rows(Traversal(G))[4]
    far = moves[moves[:, 4] >= 3]
    move = tuple(int(z) for z in far[int(rng.integers(len(far)))])
    start = prepare_tree(apply_spr(G, *move[:4]))
    return dict(G=G, start=start, move=move, model=SM.GTR(), rm=GammaRateModel(4, 0.5),
                seed=seed)


def simulated_on_host(sp):
    """The alignment TreeModel.simulate(SEARCH_SITES, seed) draws down G, by the simulator's
    specification on the host (tests/sim_reference.py): {leaf name: states [S]}."""
    import sim_reference as SR
    tr = Traversal(sp["G"])
    m, rm = sp["model"], sp["rm"]
    a, b = tr.root_edge
    cum = SR.cum_rows(m, rm.rates, tr.postorder_traversal, tr.op_lengths(), a, b,
                      tr.root_length(), tr.n_nodes)
    _, nodes = SR.walk(tr.postorder_traversal, a, b, cum, rm.weights, m.freqs, sp["seed"], 0,
                       SEARCH_SITES)
    return {name: nodes[i] for name, i in tr.names.items()}
