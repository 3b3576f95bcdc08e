"""The inputs that force every safeguard branch of the branch-length Newton rule,
shared by tests/test_newton_reference.py (their reference traces, on the CPU) and
tests/test_gpu_newton_safeguards.py (every copy of the rule on the device).

One 8-taxon topology, written as a Newick string whose lengths carry the starting length of the
scenario's edge:

    ((A,B),(C,D),((E,F),(G,H)):X);

DNA: GTR with unequal frequencies + Gamma4, 130 patterns (three 64-lane tiles, the last of 2
sites); protein: LG + Gamma4, 97 patterns.  Integer pattern weights 0..3, about a quarter zero.

Data sets (tip states simulated down the tree at TRUE lengths, X = 0.02):
  "short"  as simulated: the optimum of X is short;
  "twins"  B made identical to A at every pattern: the optimum of A's pendant edge is 0;
  "split"  (A,B,C,D) and (E,F,G,H) taken from two independent simulations: the lnL rises with X
           over the whole range.

Two conditions the traces must meet (check_conditions) shape the inputs.  A run that converges
ends on accepted steps that change lnL by less than 1e-13 |lnL|, so its last lnL comparisons
have no margin by construction: `overshoot` and `shrink` stop after SHORT_ITER steps, which is
after the branch they are about.  And |d2| where lnL flattens towards the upper bound is 1e-7 to
1e-8 of |d2| at 0.1 (26 seeds per alphabet scanned: at best 1.0e-7), so no run from 0.1 to the
upper bound keeps a sign margin of 1e-6: `upper` starts at 20.  `lower` starts at 0.165, not
0.1: the lengths halve down to the bound, and from 0.1 the last halving before it moves the
length by 0.19e-8 and lnL by 2e-10 |lnL|; from 0.165 by 0.97e-8 and 1.1e-9 |lnL|.

A sign test keeps two margins (SIGN_MARGIN, SIGN_FLOOR below): relative to the largest tested
|d|, not to the largest of every evaluated length as first planned -- the placement `overshoot`
lands on the lower bound, where |d2| is 1e7 to 5e11 against 23 to 95 at the start, which says
nothing about the rounding of the tested value -- and an absolute one against |lnL|.

The starting lengths below were chosen by scanning evaluate(t) of the CPU oracle over 400
log-spaced lengths in [1e-8, 100] for each (alphabet, data set, edge): `overshoot` is the first
scanned length right of the optimum with d2 < 0, t - d1 / d2 < 1e-8 and lnL(1e-8) < lnL(t);
`shrink` the middle (in log t) of the stretch with d1 < 0 <= d2.  No scanned length of any edge
of the tree, of the three arrangements' central lengths or of a pendant length had d1 > 0 with
d2 >= 0 (see tests/test_gpu_newton_safeguards.py): there is no `expand` scenario.
"""
import numpy as np

import newton_reference as NT
import nni_reference as NR

from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, simulate_states
from phylo_utils_amd.tree import Traversal, parse_newick, prepare_tree

TOL = 1e-8
MAX_ITER = 50
NEWICK = ("(({A}:{lA},{B}:{lB}):{lAB},({C}:{lC},{D}:{lD}):{lCD},"
          "(({E}:{lE},{F}:{lF}):{lEF},({G}:{lG},{H}:{lH}):{lGH}):{lX});")
NAMES = list("ABCDEFGH")
TRUE = dict(A=0.1, B=0.15, AB=0.08, C=0.12, D=0.2, CD=0.1, E=0.07, F=0.18, EF=0.09, G=0.14,
            H=0.11, GH=0.12, X=0.02)
# the leaves below the child end of an edge, by the edge's name in NEWICK
BELOW = dict(A="A", X="EFGH")
N_PATTERNS = dict(dna=130, protein=97)
# (seed of the data, seed of the second simulation of "split"): the first second seed from 4 up
# at which lnL of "split" rises over the whole range (about half of them: 130 independent
# columns correlate by chance) with the largest gain per step
SEEDS = dict(dna=(3, 25), protein=(5, 15))
SHORT_ITER = 3  # steps of the scenarios that would otherwise converge (see the docstring)

# id: (data set, edge, starting length by alphabet, max_iter, events the trace must contain,
# final length or None)
SCENARIOS = {
    "lower": ("twins", "A", dict(dna=0.165, protein=0.165), MAX_ITER, ["clamp_lo"], NT.MIN_LEN),
    "lower-start": ("twins", "A", dict(dna=1e-8, protein=1e-8), MAX_ITER, ["stall"],
                    NT.MIN_LEN),
    "lower-start-0": ("twins", "A", dict(dna=0.0, protein=0.0), MAX_ITER, ["clamp_lo", "stall"],
                      NT.MIN_LEN),
    "upper": ("split", "X", dict(dna=20.0, protein=20.0), MAX_ITER, ["clamp_hi"], NT.MAX_LEN),
    "upper-start": ("split", "X", dict(dna=100.0, protein=100.0), MAX_ITER, ["stall"],
                    NT.MAX_LEN),
    "overshoot": ("short", "X", dict(dna=None, protein=None), SHORT_ITER,
                  ["clamp_lo", "reject", "accept"], None),
    "shrink": ("short", "X", dict(dna=None, protein=None), SHORT_ITER, ["shrink"], None),
    "max-iter-0": ("short", "X", dict(dna=None, protein=None), 0, ["max_iter"], None),
    "max-iter-1": ("short", "X", dict(dna=None, protein=None), 1, ["max_iter"], None),
    "max-iter-2": ("short", "X", dict(dna=None, protein=None), 2, ["max_iter"], None),
}
# A sign test must hold both margins: 1e-6 of the largest tested |d|, and 1e-9 |lnL| in absolute
# size.  The second is there because the first is 1 for a trace with a single sign test, however
# small its d.  d1, d2 and lnL are sums of per-site terms over the same sites.  A site's |f'/f|
# and |f''/f| are below (1 / t)^2 + (largest rate x largest |eigenvalue|)^2 -- some 300 where
# differing states meet (the tested lengths there are 0.06 or more), less where the two ends are
# alike -- and its |ln f| is 2 or more, so rounding differences of 1e-16 per site in d are below
# 1e-14 |lnL|: 1e-9 |lnL| is five orders above them.
# The scenarios under one rate ("dna-c1": the DNA data with GammaRateModel(1, .), the other launch
# shape of k_edge_newton), from the same starts.  Left out, by the same scan of 400 lengths:
#   `overshoot`    lnL(1e-8) of X is only 0.21 below the optimum's; the lengths with a higher lnL
#                  are below 0.021 and no Newton step from them reaches the bound.  From 0.066 the
#                  bound is accepted at once (max-iter-1 and -2 still cut that run short);
#   `upper`        with one rate d1 and d2 decay as one exponential, the Newton step is the same
#                  1.44 at every length beyond 5, and after 20 of them the steps gain less than
#                  1e-13 |lnL|: no lnL margin, and |d2| falls to 1e-29 before 100;
#   `upper-start`  at 100 d1 = 2.5e-14 and d2 = -1.2e-29 are rounding residue (sign floor 1e-32):
#                  with d1 < 0 a copy would halve the length and accept.
C1_SCENARIOS = ["lower", "lower-start", "lower-start-0", "shrink", "max-iter-0", "max-iter-1",
                "max-iter-2"]


def scenarios_of(kind):
    return list(C1_SCENARIOS) if kind == "dna-c1" else sorted(SCENARIOS)


LNL_MARGIN, SIGN_MARGIN, SIGN_FLOOR = 1e-9, 1e-6, 1e-9


def model(kind):
    if kind == "dna":
        return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    if kind == "dna-c1":  # the DNA data under one rate: k_edge_newton's other launch shape
        return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(1, 0.5)
    return SM.LG(), GammaRateModel(4, 0.8)


def _base(kind):
    return kind.split("-")[0]


def newick(lengths=None):
    lens = dict(TRUE, **(lengths or {}))
    return NEWICK.format(**dict({n: n for n in NAMES}, **{"l" + k: repr(float(v))
                                                           for k, v in lens.items()}))


_DATA = {}


def data(kind, which):
    """(codes uint8 [8][S] in NAMES' order, pattern weights [S]) of a data set; computed once."""
    kind = _base(kind)
    if (kind, which) not in _DATA:
        m, rm = model(kind)
        S = N_PATTERNS[kind]
        sims = [simulate_states(np.random.default_rng(seed), parse_newick(newick()), m,
                                rm.rates, S) for seed in SEEDS[kind]]
        codes = np.array([sims[0][n] for n in NAMES], dtype=np.uint8)
        if which == "twins":
            codes[1] = codes[0]
        elif which == "split":
            codes[4:] = np.array([sims[1][n] for n in NAMES[4:]], dtype=np.uint8)
        elif which != "short":
            raise ValueError(which)
        w = np.random.default_rng(SEEDS[kind][0] + 100).choice(
            [0.0, 1.0, 2.0, 3.0], S, p=[0.25, 0.35, 0.25, 0.15])
        codes.setflags(write=False)
        w.setflags(write=False)
        _DATA[kind, which] = (codes, w)
    return _DATA[kind, which]


def edge_of(tree, tr, name):
    """(NOD, PAR) in Traversal `tr` of prepared `tree` of the edge NEWICK calls `name`."""
    want = frozenset(BELOW[name])
    below = {}
    for n in tree.seed_node.postorder():
        below[n] = frozenset([n.label]) if n.is_leaf() else \
            frozenset().union(*(below[c] for c in n.children))
        if below[n] == want and n is not tree.seed_node:
            assert n.parent is not tree.seed_node
            return tr.node_dict[n], tr.node_dict[n.parent]
    raise ValueError(name)


class Case(object):
    """One (alphabet, data set, edge, starting length): the tree, the oracle's partials as the
    optimising traversal holds them on the edge, and evaluate(t) of the edge."""

    def __init__(self, orc, kind, which, edge, t0):
        self.kind, self.which, self.edge_name, self.t0 = kind, which, edge, t0
        self.model, self.rm = model(kind)
        self.codes, self.weights = data(kind, which)
        self.table = np.eye(len(self.model.freqs))
        self.newick = newick({edge: t0})
        self.tree = prepare_tree(self.newick)
        self.tr = Traversal(self.tree)
        self.e = NR.eigen(self.model, self.rm)
        self.tips = {self.tr.names[n]: self.table[self.codes[i]] for i, n in enumerate(NAMES)}
        self.edge = edge_of(self.tree, self.tr, edge)
        st = NT.oracle_state(orc, self.tips, self.tr, self.e, self.weights)
        self.lnl0 = st["lnl"]
        self.P, self.S, self.rows = NT.walk_to(orc, st, self.tr, self.e, self.edge)
        self.evaluate = NT.edge_evaluate(orc, self.P, self.S, self.edge[0], self.edge[1], self.e,
                                         self.weights)
        self.orc = orc

    def quartet(self):
        """(nodes x0..x3, pendant lengths [4]) of the quartet around an internal edge, as
        nni_reference.sweep names them."""
        tr = self.tr
        child = {int(p): (int(a), int(b)) for p, a, b in tr.postorder_traversal}
        nod, par = self.edge
        row = self.rows[-1]
        nodes = child[nod] + (int(row[1]), int(row[2]))
        lens = [tr.brlens[nodes[0], nod], tr.brlens[nodes[1], nod], tr.brlens[nodes[2], par],
                tr.brlens[nodes[3], par]]
        return nodes, lens

    def quartet_evaluate(self, k=0):
        nodes, lens = self.quartet()
        return NT.quartet_evaluate(self.orc, self.P, self.S, nodes, lens, k, self.e, self.weights)


def scenario(orc, kind, sid, starts=None):
    """(Case, max_iter, required events, final length or None) of scenario `sid`."""
    which, edge, t0, max_iter, events, end = SCENARIOS[sid]
    t0 = t0[_base(kind)]
    if t0 is None:
        t0 = (starts or STARTS)[kind]["shrink" if sid == "shrink" else "overshoot"]
    return Case(orc, kind, which, edge, t0), max_iter, events, end


def check_conditions(trace, events, what=""):
    """The conditions on the input: the trace takes the branches asked for, in that order, and
    no decision of it is near enough to flip under the copies' rounding differences."""
    have = iter(trace.events)
    assert all(ev in have for ev in events), (what, events, trace.events)
    assert all(m >= LNL_MARGIN for m in trace.lnl_margins), (what, min(trace.lnl_margins))
    assert all(m >= SIGN_MARGIN for m in trace.sign_margins), (what, min(trace.sign_margins))
    assert all(m >= SIGN_FLOOR for m in trace.sign_floors), (what, min(trace.sign_floors))


# ------------------------------------------------------------------ placement
# Queries on the "short" data at edge X from pendant length l0: "random" states drawn from the
# model's frequencies (the pendant optimum is the upper bound), "near" tip E with every 25th
# column changed to the next state (a short pendant optimum).
def queries(kind):
    m, _ = model(kind)
    K = len(m.freqs)
    codes, _ = data(kind, "short")
    S = codes.shape[1]
    rng = np.random.default_rng(SEEDS[_base(kind)][1] + 200)
    f = np.asarray(m.freqs, dtype=np.float64)
    rand = rng.choice(K, S, p=f / f.sum()).astype(np.uint8)
    near = codes[NAMES.index("E")].copy()
    near[::25] = (near[::25] + 1) % K
    return np.stack([rand, near])


def place_problem(kind):
    """A place_reference.problem-like dict of the "short" data with the two queries."""
    m, rm = model(kind)
    codes, w = data(kind, "short")
    table = np.eye(len(m.freqs))
    return dict(tree=newick(), names=list(NAMES), codes=np.asarray(codes), table=table, model=m,
                rm=rm, compact=True, weights=np.asarray(w),
                queries=dict(names=["random", "near"], codes=queries(kind), table=table,
                             site_pattern=None, site_weight=np.asarray(w)))


def place_edge_number(ref):
    """The number of edge X among the edges of a place_reference.Restated of place_problem."""
    tree = prepare_tree(newick())
    return [tuple(e) for e in ref.edges.tolist()].index(edge_of(tree, Traversal(tree), "X"))


# query index, starting pendant length by alphabet (None: STARTS), max_iter, events
PLACE_SCENARIOS = {
    "upper": (0, "place-upper", MAX_ITER, ["clamp_hi"], NT.MAX_LEN),
    "overshoot": (1, "place-overshoot", SHORT_ITER, ["clamp_lo", "reject", "accept"], None),
    "shrink": (1, "place-shrink", SHORT_ITER, ["shrink"], None),
    "max-iter-0": (1, "place-overshoot", 0, ["max_iter"], None),
    "max-iter-1": (1, "place-overshoot", 1, ["max_iter"], None),
    "max-iter-2": (1, "place-overshoot", 2, ["max_iter"], None),
}

# the scanned starting lengths (see the module's docstring)
STARTS = {
    "dna": {"overshoot": 0.066, "shrink": 5.0, "place-upper": 20.0, "place-overshoot": 0.25,
            "place-shrink": 6.0},
    "dna-c1": {"overshoot": 0.066, "shrink": 5.0},
    "protein": {"overshoot": 0.2, "shrink": 6.0, "place-upper": 20.0, "place-overshoot": 0.55,
                "place-shrink": 9.0},
}
