"""CPU restatement of the phylogenetic placement for the tests, composed like
tests/counts_reference.py (whose ``state`` and ``eigen`` it shares through
tests/ancestral_reference.py): the same walk with ``clv_c`` and ``pmatrix``, and lnL(q, e, l)
from its definition with transition MATRICES -- P_c(t/2) on the two ends, P_c(l) on the query --
not the eigen-basis form the kernels use.  `orc` is the oracle module (the ``oracle_mod``
fixture)."""
import numpy as np

import ancestral_reference as AR
from ancestral_reference import eigen, state  # noqa: F401

from phylo_utils_amd import alignment as A
from phylo_utils_amd import optimisation as O
from phylo_utils_amd import place as PL
from phylo_utils_amd.tree import Traversal, prepare_tree

LO, HI = 1e-8, 100.0  # the pendant bounds (pu_edge.cpp kMinLen / kMaxLen)
H1 = 1e-6             # step of the central difference for dlnL/dl (tests/test_counts.py's H)
H2 = 1e-4             # step of the second difference: rounding 4 eps |lnL| / H2^2
PENDANT = 0.05        # pendant length the planted sisters are simulated at
REF_AMBIGUOUS = 0.03  # share of the reference cells recoded as an ambiguity / gap code

# name: (base case of ancestral_reference.CASES, query kinds, n_sites through a site map or
# None).  The smallest shapes at which the placement kernels can go wrong: the shapes of
# k_ancestral's cases (several tiles, a tile of one lane, one category, an odd category count,
# the LDS limit, a root edge with a tip end, scalers that differ between the categories on 297
# edges), a site map with repeats and non-unit weights, and a query length of two full
# pre-score chunks (2048 sites) plus a partial one.
# Query kinds: "copy" an exact copy of a tip, "sister" simulated as the sister of an internal
# edge, "+amb" 15 % of the columns replaced by an ambiguity code that holds the state, "+n30"
# 30 % by the gap code, "gap" all gaps, "sparse5" gaps except 5 columns, "noisy" a tip copy
# with 20 % of the columns redrawn.
CASES = {
    "dna-coded-14x700-C4": ("dna-coded-14x700-C4", ["copy", "copy", "sister", "sister",
                                                    "copy+amb", "sister+amb", "copy+n30", "gap",
                                                    "sparse5"], None),
    "dna-dense-8x97-C1": ("dna-dense-8x97-C1", ["copy", "sister", "gap"], None),
    "dna-8x65-C3": ("dna-8x65-C3", ["copy", "sister", "gap"], None),
    "binary-8x70-Cmax": ("binary-8x70-Cmax", ["copy", "sister", "gap"], None),
    "protein-8x97-C4": ("protein-8x97-C4", ["copy", "sister", "gap"], None),
    "dna-pendant-root-4x70-C4": ("dna-pendant-root-4x70-C4", ["copy", "sister", "gap"], None),
    "dna-caterpillar-150x130-C4": ("dna-caterpillar-150x130-C4", ["copy", "sister"], None),
    "dna-mapped-14x700-1000-C4": ("dna-coded-14x700-C4", ["copy", "sister", "gap"], 1000),
    "dna-chunks-8x65-4233-C3": ("dna-8x65-C3", ["copy"] + ["noisy"] * 63 + ["gap"], 4233),
}
SMALL = [c for c in sorted(CASES) if "caterpillar" not in c]
# seeds of the planted data: the first, from 11 up, at which tests/test_place.py finds every
# planted query of the case decided (70 binary columns leave a sister open more often)
SEED = 11
SEEDS = {"binary-8x70-Cmax": 12, "dna-caterpillar-150x130-C4": 12}


def _alphabet(kind):
    return {"binary": A.BINARY, "protein": A.PROTEIN}.get(kind, A.DNA)


def _clade_edge(tree, leaves):
    """(child index, parent index) in Traversal(tree) of the edge above the node whose leaf set,
    query leaves aside, is `leaves`."""
    tr = Traversal(tree)
    below = {}
    for n in tree.seed_node.postorder():
        below[n] = frozenset([n.label]) if n.is_leaf() else \
            frozenset().union(*(below[c] for c in n.children))
        if n is not tree.seed_node and n.parent is not tree.seed_node and \
                frozenset(x for x in below[n] if not x.startswith("q")) == leaves and \
                not (n.is_leaf() and n.label.startswith("q")):
            return tr.node_dict[n], tr.node_dict[n.parent]
    raise ValueError("no such clade")


def problem(case):
    """ancestral_reference.problem's dict (tree, names, codes, table, model, rm, compact,
    weights) with the data simulated anew down the tree WITH the planted sisters attached, so
    that a sister query is a real draw at its edge, plus: queries dict(names, codes uint8
    [Q][n_sites], table) in the alphabet's own code table, kinds [Q], planted {query: (NOD, PAR)
    edge} for the copies and sisters, site_pattern / site_weight (None / the pattern weights
    without a site map)."""
    from phylo_utils_amd.synthetic import simulate_states
    base, kinds, n_sites = CASES[case]
    prob = dict(AR.problem(base))
    kind = AR.CASES[base][0]
    rng = np.random.default_rng(SEEDS.get(case, SEED))
    tree = prepare_tree(prob["tree"])
    tr = Traversal(tree)
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    inner = [(int(r[3]), int(r[4])) for r in tr.optimising_traversal[1:]
             if r[3] >= 0 and int(r[3]) in internal]
    node = {i: n for n, i in tr.node_dict.items()}
    S = prob["codes"].shape[1]
    # the planted edges, by the leaf set below their child end
    planted, clades = {}, {}
    aug = tree
    for k, what in enumerate(kinds):
        if what.startswith("sister"):
            nod, par = inner[int(rng.integers(len(inner)))]
            planted[k] = (nod, par)
            clades[k] = frozenset(x.label for x in node[nod].leaves())
            aug = PL.attach(aug, _clade_edge(aug, clades[k]), "q%d" % k, PENDANT)
    sts = simulate_states(rng, aug, prob["model"], prob["rm"].rates, S)
    ref_states = np.array([sts[n] for n in prob["names"]], dtype=np.int64)
    # the reference tips and the queries go through the alphabet's own code table; REF_AMBIGUOUS
    # of the reference cells become an ambiguity or gap code that holds the state, so that the
    # kernels meet non-unit table rows at the edges' tip ends
    table, _ = A.code_table(_alphabet(kind))
    table = np.ascontiguousarray(table)
    K = table.shape[1]
    one_hot = [int(np.flatnonzero((table == np.eye(K)[i]).all(axis=1))[0]) for i in range(K)]
    gap = int(np.flatnonzero((table == 1.0).all(axis=1))[0])
    holds = [[c for c in range(len(table)) if table[c, i] == 1.0 and table[c].sum() > 1]
             for i in range(K)]
    ref_codes = np.array(one_hot, dtype=np.uint8)[ref_states]
    for t, s_ in np.argwhere(rng.random(ref_states.shape) < REF_AMBIGUOUS):
        opts = holds[ref_states[t, s_]]
        ref_codes[t, s_] = opts[int(rng.integers(len(opts)))]
    prob["codes"], prob["table"] = ref_codes, table
    tips = list(prob["names"])
    codes = np.zeros((len(kinds), S), dtype=np.uint8)
    for k, what in enumerate(kinds):
        head = what.split("+")[0]
        if head in ("copy", "noisy"):
            t = tips[int(rng.integers(len(tips)))]
            st = ref_states[tips.index(t)]
            copied = ref_codes[tips.index(t)] if head == "copy" else None
            if head == "copy":
                planted[k] = (tr.names[t], tr.node_dict[node[tr.names[t]].parent]
                              if node[tr.names[t]].parent is not tree.seed_node else None)
            else:
                redo = rng.random(S) < 0.2
                st = np.where(redo, rng.integers(0, K, S), st)
        elif head == "sister":
            st = sts["q%d" % k].astype(np.int64)
        else:
            st = np.zeros(S, dtype=np.int64)
        row = np.array([one_hot[i] for i in st], dtype=np.uint8)
        if head == "copy":
            row = copied.copy()  # exact: the tip's ambiguity codes too
        if what.endswith("+amb"):
            for s in np.flatnonzero(rng.random(S) < 0.15):
                row[s] = holds[st[s]][int(rng.integers(len(holds[st[s]])))]
        if what.endswith("+n30"):
            row[rng.random(S) < 0.3] = gap
        if head == "gap":
            row[:] = gap
        if head == "sparse5":
            t = tips[int(rng.integers(len(tips)))]
            row[:] = gap
            cols = rng.choice(S, 5, replace=False)
            row[cols] = [one_hot[i] for i in ref_states[tips.index(t)][cols]]
        codes[k] = row
    # a tip on the root edge: its edge is the root edge itself
    left, right = tr.root_edge
    for k, e in planted.items():
        if e[1] is None:
            planted[k] = (left, right)
    if n_sites is None:
        site_pattern, site_weight = None, np.asarray(prob["weights"], dtype=np.float64)
    else:
        site_pattern = rng.integers(0, S, n_sites).astype(np.int32)
        site_pattern[:S // 2] = np.arange(S // 2)  # a stretch in order, then repeats
        site_weight = rng.choice([0.0, 0.5, 1.0, 2.5], n_sites, p=[0.05, 0.25, 0.45, 0.25])
        codes = np.ascontiguousarray(codes[:, site_pattern])
    prob.update(queries=dict(names=["q%d" % k for k in range(len(kinds))], codes=codes,
                             table=table, site_pattern=site_pattern,
                             site_weight=site_weight),
                kinds=list(kinds), planted=planted)
    return prob


class Restated(object):
    """The walk of pu_place_prescore on the CPU: per edge the ends' vectors as the walk leaves
    them, and from them lnL(q, e, l), the pre-score matrix and the pendant optimum."""

    def __init__(self, orc, prob):
        self.orc, self.prob = orc, prob
        self.tr = tr = Traversal(prepare_tree(prob["tree"]))
        self.e = e = eigen(prob["model"], prob["rm"])
        self.tips = {tr.names[n]: prob["table"][prob["codes"][i]]
                     for i, n in enumerate(prob["names"])}
        st = state(orc, self.tips, tr, e, prob["weights"])
        self.lnl = st["lnl"]
        P, S = st["partials"], st["scale"]
        self.post = (P.copy(), S.copy())  # the post-order state (pu_place_edge on a fresh run)
        self.edges, self.lengths, self.ends = [], [], []
        for row in tr.optimising_traversal:
            if row[0] >= 0:
                p, x, y = (int(v) for v in row[:3])
                cml = np.zeros(S[p].shape)
                P[p] = orc.clv_c(self.pm(tr.brlens[p, x]), self.pm(tr.brlens[p, y]), P[x], P[y],
                                 S[x], S[y], cml)
                S[p] = cml
            nod, par = int(row[3]), int(row[4])
            if nod < 0:
                continue
            self.edges.append((nod, par))
            self.lengths.append(float(tr.brlens[nod, par]))
            self.ends.append((P[nod].copy(), S[nod].copy(), P[par].copy(), S[par].copy()))
        self.edges = np.array(self.edges, dtype=np.int32)
        self.lengths = np.array(self.lengths)
        q = prob["queries"]
        self.z = q["table"][q["codes"]]  # [Q][n_sites][K]
        n_sites = q["codes"].shape[1]
        self.map = np.arange(n_sites) if q["site_pattern"] is None else q["site_pattern"]
        self.sw = np.ones(n_sites) if q["site_weight"] is None else q["site_weight"]
        self._mid = {}

    def pm(self, t):
        e = self.e
        return self.orc.pmatrix(e["evecs"], e["evals"], e["ivecs"], t, e["rates"])

    def midpoint(self, k, length=None, ends=None):
        """(a [S][C][K], mix weight [S][C], m [S]) of edge number k at `length` (None: its
        own) from `ends` (None: the walk's)."""
        key = (k, length)
        if ends is None and key in self._mid:
            return self._mid[key]
        A_, sA, B_, sB = self.ends[k] if ends is None else ends
        half = self.pm(0.5 * (self.lengths[k] if length is None else length))
        a = self.e["freqs"][None, None, :] * np.einsum("cij,scj->sci", half, A_) * \
            np.einsum("cij,scj->sci", half, B_)
        sigma = sA + sB
        live = a.sum(axis=2) > 0
        m = np.where(live, sigma, -np.inf).max(axis=1)
        with np.errstate(invalid="ignore"):
            we = np.where(live, self.e["weights"][None, :] * np.exp(sigma - m[:, None]), 0.0)
        if ends is None:
            self._mid[key] = (a, we, m)
        return a, we, m

    def lnl_at(self, q, k, l, mid=None):
        """lnL(q, e, l): query q at the midpoint of edge number k on a pendant branch l."""
        a, we, m = self.midpoint(k) if mid is None else mid
        y = np.einsum("cij,sj->sci", self.pm(l), self.z[q])      # [P_c(l) z](i) per column
        f = np.einsum("sci,sci->sc", a[self.map], y)
        F = (we[self.map] * f).sum(axis=1)
        use = self.sw != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.dot(self.sw[use], (m[self.map] + np.log(F))[use]))

    def prescore(self, l0):
        """[E][Q] lnL(q, e, l0)."""
        Q = len(self.z)
        return np.array([[self.lnl_at(q, k, l0) for q in range(Q)]
                         for k in range(len(self.edges))])

    def optimum(self, q, k, l0):
        """(l*, lnL(l*)) by Brent over [LO, HI] from l0."""
        out = np.zeros(3)
        O.brent(LO, min(max(l0, LO), HI), HI, lambda l: -self.lnl_at(q, k, l), 1e-10, out)
        best = (float(out[0]), -float(out[1]))
        at_lo = self.lnl_at(q, k, LO)  # Brent stops short of the bracket's ends
        return (LO, at_lo) if at_lo >= best[1] else best

    def fd_derivs(self, q, k, l, mid=None):
        """(dlnL/dl, d2lnL/dl2) at l by central differences (steps H1, H2); within a step of the
        lower bound, where the stencil would leave the domain, by the second-order one-sided
        differences on l, l + h, l + 2h(, l + 3h)."""
        f = lambda x: self.lnl_at(q, k, x, mid)
        if l > H2 + LO:
            d1 = (f(l + H1) - f(l - H1)) / (2 * H1)
            d2 = (f(l + H2) - 2 * f(l) + f(l - H2)) / H2 ** 2
        else:
            d1 = (-3 * f(l) + 4 * f(l + H1) - f(l + 2 * H1)) / (2 * H1)
            d2 = (2 * f(l) - 5 * f(l + H2) + 4 * f(l + 2 * H2) - f(l + 3 * H2)) / H2 ** 2
        return d1, d2

    def joined_lnl(self, q, k, l):
        """The oracle's tree_lnl of the (N+1)-taxon tree PL.attach builds: the yardstick's own
        yardstick."""
        tree = PL.attach(self.prob["tree"], self.edges[k], "query", l)
        tr = Traversal(prepare_tree(tree))
        e = self.e
        by_name = {n: self.prob["table"][self.prob["codes"][i]][self.map]
                   for i, n in enumerate(self.prob["names"])}
        by_name["query"] = self.z[q]
        tips = {tr.names[n]: v for n, v in by_name.items()}
        return self.orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                 tr.root_length(), e["evecs"], e["evals"], e["ivecs"],
                                 e["freqs"], e["rates"], e["weights"], site_weights=self.sw,
                                 n_nodes=tr.n_nodes)[0]
