"""The cases of the extended-precision fixtures (tests/golden/hp_*.npz): models, rate models,
trees and tips, and the oracle's evaluation of them.  No mpmath here: the generator
(tests/golden/make_golden_hp.py) and tests/test_hp_reference.py add tests/hp_reference.py; the
GPU tests read the fixtures only and use ``model_of`` / ``rate_model_of`` to rebuild the models.
"""
import numpy as np

import hp_check as CK

from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, InvariantGammaModel, UniformRateModel
from phylo_utils_amd.tree import Traversal, prepare_tree

MODELS = ("gtr", "lg")
GTR_RATES = (0.5, 3.0, 0.2, 0.1, 6.0, 1.0)
GTR_FREQS = (0.45, 0.05, 0.1, 0.4)
P_RATE_MODELS = ("c1", "g05", "g01")       # the P-matrix cases
TREE_RATE_MODELS = ("c1", "g01", "g05i")   # the 8-taxon cases


def model_of(name):
    return SM.GTR(GTR_RATES, GTR_FREQS) if name == "gtr" else SM.LG()


def rate_model_of(name):
    return {"c1": UniformRateModel, "g05": lambda: GammaRateModel(4, 0.5),
            "g01": lambda: GammaRateModel(4, 0.1),
            "g05i": lambda: InvariantGammaModel(0.2, 4, 0.5)}[name]()


def table_of(model):
    """(code table [n_codes][K], the code of every state's one-hot vector, the gap code)."""
    table = A.code_table(A.DNA if model == "gtr" else A.PROTEIN)[0]
    K = table.shape[1]
    state = np.array([int(np.where((table == np.eye(K)[k]).all(axis=1))[0][0])
                      for k in range(K)], dtype=np.uint8)
    return table, state, int(np.where(table.all(axis=1))[0][0])


def schedule(newick, names):
    """(Traversal, {node: row of `names`}) of a Newick string."""
    tr = Traversal(prepare_tree(newick))
    return tr, {tr.names[n]: i for i, n in enumerate(names)}


# ---------------------------------------------------------------- P matrices: 12-taxon caterpillar
P_LENGTHS = (0.0, 1e-14, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2, 1.0, 10.0, 100.0, 1000.0)
P_NAMES = ["t%d" % i for i in range(12)]


def p_newick():
    """A 12-taxon caterpillar (t0, t1, X2), X_i = (t_i, X_{i+1}), X10 = (t10, t11): the eleven
    lengths of P_LENGTHS on pendant and internal edges in turn, every other edge 0.1."""
    pend = {0: 0.0, 1: 1e-10, 2: 1e-6, 3: 1e-2, 4: 10.0, 5: 1000.0}
    inner = {2: 1e-14, 3: 1e-8, 4: 1e-4, 5: 1.0, 6: 100.0}
    s = "(t10:0.1,t11:0.1)"
    for i in range(9, 1, -1):
        s = "(t%d:%r,%s:%r)" % (i, pend.get(i, 0.1), s, inner.get(i + 1, 0.1))
    return "(t0:%r,t1:%r,%s:%r);" % (pend[0], pend[1], s, inner[2])


def p_codes():
    return np.random.default_rng(12).integers(0, 4, (12, 4)).astype(np.uint8)


# ---------------------------------------------------------------- the 8-taxon tree
T8_NAMES = ["t%d" % i for i in range(1, 9)]
# unrooted: N12 = (t1, t2), N34 = (t3, t4), NA = (N12, N34), NB = (t5, t6), NC = (t7, t8) around
# the centre R0 = (NA, NB, NC).  Every length of {1e-8, 1e-4, 0.1, 5} is on a pendant and on an
# internal edge; t1 and t2 are sisters on 1e-8 pendant edges.
_N34 = "(t3:0.1,t4:5.0)"
_NB = "(t5:0.0001,t6:0.1)"
_NC = "(t7:5.0,t8:0.0001)"
_REST = "(%s:0.0001,%s:0.0001)" % (_NB, _NC)
T8_ROOTINGS = ("r5", "r01", "r1e8", "rp")
EDGE_T = (1e-8, 1e-3, 1.0)   # plus the edge's own length
EDGE_ROOTINGS = ("rp", "r01", "r5")


def t8_newick(rooting, sister=1e-8):
    """The 8-taxon tree with one of its edges as the root edge -- "r5": (NA, R0), length 5;
    "r01": (N12, NA), the internal 0.1 edge; "r1e8": (N34, NA), the internal 1e-8 edge; "rp":
    (t1, N12), a 1e-8 pendant edge.  `sister`: the length of t1's and t2's pendant edges (0.0 in
    the zero-length cases).  In "r5" the root edge's far end has two children on equal lengths."""
    n12 = "(t1:%r,t2:%r)" % (float(sister), float(sister))
    if rooting == "r5":
        return "((%s:0.1,%s:1e-08):5.0,%s:0.0001,%s:0.0001);" % (n12, _N34, _NB, _NC)
    if rooting == "r01":
        return "(%s:0.1,%s:1e-08,%s:5.0);" % (n12, _N34, _REST)
    if rooting == "r1e8":
        return "(%s:1e-08,%s:0.1,%s:5.0);" % (_N34, n12, _REST)
    if rooting == "rp":
        return "(t1:%r,t2:%r,(%s:1e-08,%s:5.0):0.1);" % (float(sister), float(sister), _N34, _REST)
    raise ValueError(rooting)


def t8_tips(model, S=80):
    """(codes uint8 [8][S], pattern weights [S]): random states with about 12 % ambiguity and
    gap codes, then the constructed columns -- 0 constant, 1 all gaps, 2 t1 and t2 in different
    states and the rest constant, 3 t1 and t2 in different states in a random column -- and
    weights 1..5 with zeros at patterns 10 and 70 (one in each tile of 64)."""
    table, state, gap = table_of(model)
    K = table.shape[1]
    rng = np.random.default_rng(80 + K)
    codes = state[rng.integers(0, K, (8, S))]
    amb = rng.random((8, S)) < 0.12
    codes[amb] = rng.integers(0, len(table), int(amb.sum())).astype(np.uint8)
    codes[:, 0] = state[0]
    codes[:, 1] = gap
    codes[:, 2] = state[0]
    codes[1, 2] = state[1]
    codes[0, 3], codes[1, 3] = state[0], state[1]
    w = rng.integers(1, 6, S).astype(np.float64)
    w[[10, 70]] = 0.0
    return np.ascontiguousarray(codes, dtype=np.uint8), w


# ---------------------------------------------------------------- rescaling: 200-taxon caterpillar
DEEP_NAMES = ["t%d" % i for i in range(200)]


def deep_newick():
    """Lengths 0.6, 0.9 and 1.3 in turn: every tip multiplies the likelihood by about 1/4, so
    the unscaled partials pass 2^-128 several times on the way up."""
    L = (0.6, 0.9, 1.3)
    s = "(t198:0.6,t199:0.9)"
    for i in range(197, 1, -1):
        s = "(t%d:%r,%s:%r)" % (i, L[i % 3], s, L[(i + 1) % 3])
    return "(t0:0.9,t1:1.3,%s:0.6);" % s


def deep_tips():
    table, state, gap = table_of("gtr")
    rng = np.random.default_rng(200)
    codes = state[rng.integers(0, 4, (200, 8))]
    codes[rng.random((200, 8)) < 0.03] = gap
    return np.ascontiguousarray(codes, dtype=np.uint8), np.array([1., 2, 3, 1, 0, 4, 1, 2])


# ---------------------------------------------------------------- the oracle on a case
def oracle_tree(orc, newick, names, codes, table, model, rm, weights, eigen_scale=1.0,
                cat_scale=None):
    """oracle.tree_lnl of a case with every buffer, plus its Traversal.  `eigen_scale`
    multiplies every eigenvalue and `cat_scale` = (category, factor) scales that category's
    root partials: the deliberate errors of the checker's own tests."""
    tr, rows = schedule(newick, names)
    tips = {n: table[codes[i]] for n, i in rows.items()}
    ev, el, iv = model.engine_eigen()
    res = orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                       tr.root_length(), ev, el * eigen_scale, iv, model.freqs, rm.rates,
                       rm.weights, site_weights=weights, n_nodes=tr.n_nodes, return_all=True)
    if cat_scale is not None:
        c, factor = cat_scale
        rp = res["root_partials"].copy()
        rp[:, c] *= factor
        with np.errstate(divide="ignore"):
            site = orc.logsumexp_cats(orc.lnl_node(model.freqs, rp, res["root_scale"]),
                                      rm.weights)
        res = dict(res, site_lnl=site, lnl=float(np.dot(weights, site)))
    res["tr"] = tr
    return res


def oracle_edge(orc, res, model, rm, weights, t):
    """oracle.edge_derivs at length t of the root edge of `res` (an oracle_tree result)."""
    a, b = res["tr"].root_edge
    ev, el, iv = model.engine_eigen()
    return orc.edge_derivs(res["partials"][a], res["scale"][a], res["partials"][b],
                           res["scale"][b], ev, el, iv, t, rm.rates, rm.weights, model.freqs,
                           weights)


def reroot(ops, lens, root_edge, root_len, edge):
    """The schedule of the same unrooted tree rooted on `edge` = (a, b): (ops [n][3], lens [n][2],
    the length of (a, b)).  Node numbers are kept."""
    adj = {}
    for (p, c1, c2), (l1, l2) in zip(np.asarray(ops).tolist(), np.asarray(lens).tolist()):
        for c, l in ((c1, l1), (c2, l2)):
            adj.setdefault(p, {})[c] = l
            adj.setdefault(c, {})[p] = l
    ra, rb = (int(v) for v in root_edge)
    adj.setdefault(ra, {})[rb] = float(root_len)
    adj.setdefault(rb, {})[ra] = float(root_len)
    a, b = (int(v) for v in edge)
    if b not in adj.get(a, {}):
        raise ValueError("no edge (%d, %d)" % (a, b))
    new_ops, new_lens = [], []
    for start, came in ((a, b), (b, a)):
        stack = [(start, came, False)]
        while stack:
            u, frm, done = stack.pop()
            kids = [w for w in adj[u] if w != frm]
            if not kids:
                continue
            if done:
                new_ops.append((u, kids[0], kids[1]))
                new_lens.append((adj[u][kids[0]], adj[u][kids[1]]))
                continue
            stack.append((u, frm, True))
            for w in reversed(kids):
                stack.append((w, u, False))
    return (np.array(new_ops, dtype=np.int32).reshape(-1, 3),
            np.array(new_lens, dtype=np.float64).reshape(-1, 2), adj[a][b])


# ---------------------------------------------------------------- the oracle's errors (E_orc_*)
# One evaluation of the oracle is one fp64 rounding of the formula, and its error at a single
# value -- one pattern, one length of one edge -- can be small by chance (it changes sign from
# value to value).  The yardstick E_orc_* of such a value is therefore the largest error over
# several roundings of the same formula, every one as legitimate as the oracle's own:
#   * V diag(d) V^-1, on the eigen-system the device is given, formed as (V d) V^-1 (the
#     oracle's pmatrix), as V (d V^-1), or as one sum over k;
#   * for a site lnL the four rootings of the tree (the pulley principle: one value, four
#     orders of arithmetic); for an edge quantity the edge's two orientations.
# E_orc0_* is the error of the oracle as it stands (the first of these roundings).
def text(a):
    return bytes(np.asarray(a)).decode()


def p_builders(model):
    """[pm(t, rates, order) -> [C][K][K]]: d^order/dt^order P(t r) in three fp64 roundings of
    the product on the model's eigen-system; the first is oracle.pmatrix_deriv."""
    ev, el, iv = model.engine_eigen()
    out = []
    for kind in range(3):
        def pm(t, rates, order, kind=kind):
            mats = []
            for r in rates:
                d = (el * r) ** order * np.exp(el * (t * r))
                mats.append((ev * d).dot(iv) if kind == 0 else
                            ev.dot(d[:, None] * iv) if kind == 1 else
                            np.einsum("ik,k,kj->ij", ev, d, iv))
            return np.stack(mats)
        out.append(pm)
    return out


def draw_tree(orc, pm, tips, ops, lens, root_edge, root_len, model, rm, weights, n_nodes):
    """oracle.tree_lnl_p with every buffer on the matrices of one builder."""
    P = np.stack([np.stack([pm(l1, rm.rates, 0), pm(l2, rm.rates, 0)]) for l1, l2 in lens])
    Proot = np.stack([pm(0.0, rm.rates, 0), pm(root_len, rm.rates, 0)])
    return orc.tree_lnl_p(tips, ops, P, Proot, tuple(int(v) for v in root_edge), model.freqs,
                          rm.weights, weights, n_nodes, return_all=True)


def _rooting_of(newick, names, g):
    tr, rows = schedule(newick, names)
    tips = {n: g["table"][g["codes"][i]] for n, i in rows.items()}
    return tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge, tr.root_length(), tr.n_nodes


def _site_errors(orc, g, key, rootings, model, rm):
    """E_orc_site [S], E_orc_lnl and their E_orc0 twins for one case over its `rootings` =
    [(tips, ops, lens, root_edge, root_len, n_nodes)], the first the case's own."""
    site, zero = g[key + "_site"], g[key + "_zero"]
    lnl = float(g[key + "_lnl"]) if key + "_lnl" in g else None
    e_site, e_lnl = [], []
    for i, (tips, ops, lens, re, rl, nn) in enumerate(rootings):
        for j, pm in enumerate(p_builders(model)):
            if i == j == 0:
                ev, el, iv = model.engine_eigen()
                o = orc.tree_lnl(tips, ops, lens, re, rl, ev, el, iv, model.freqs, rm.rates,
                                 rm.weights, site_weights=g["weights"], n_nodes=nn,
                                 return_all=True)
            else:
                o = draw_tree(orc, pm, tips, ops, lens, re, rl, model, rm, g["weights"], nn)
            with np.errstate(invalid="ignore"):
                e_site.append(np.where(zero, 0.0, np.abs(o["site_lnl"] - site)))
            if lnl is not None:
                e_lnl.append(abs(o["lnl"] - lnl) / abs(lnl))
    out = {key + "_E_orc_site": np.max(e_site, axis=0), key + "_E_orc0_site": e_site[0]}
    if lnl is not None:
        out[key + "_E_orc_lnl"] = np.float64(max(e_lnl))
        out[key + "_E_orc0_lnl"] = np.float64(e_lnl[0])
    return out


def edge_draws(orc, g, model, rm, rooting, rmn):
    """[draw][n_t][3]: (lnL, d1, d2) of the root edge of `rooting` at the fixture's lengths, for
    every builder and both orientations of the edge; draw 0 is oracle.edge_derivs as it stands."""
    tips, ops, lens, re, rl, nn = _rooting_of(text(g["newick_" + rooting]), T8_NAMES, g)
    a, b = (int(v) for v in re)
    ts = g["%s_edge_%s_t" % (rmn, rooting)]
    out = []
    for j, pm in enumerate(p_builders(model)):
        o = draw_tree(orc, pm, tips, ops, lens, re, rl, model, rm, g["weights"], nn)
        for x, y in ((a, b), (b, a)):
            out.append([orc.edge_derivs_p(
                o["partials"][x], o["scale"][x], o["partials"][y], o["scale"][y],
                (pm(0.0, rm.rates, 0),) + tuple(pm(float(t), rm.rates, k) for k in range(3)),
                rm.weights, model.freqs, g["weights"]) for t in ts])
    o = oracle_tree(orc, text(g["newick_" + rooting]), T8_NAMES, g["codes"], g["table"], model,
                    rm, g["weights"])
    out[0] = [oracle_edge(orc, o, model, rm, g["weights"], float(t)) for t in ts]
    return np.array(out)


def oracle_errors_pmat(orc, g, name):
    """The E_orc_* entries of hp_pmat_<name>: per matrix, the oracle's largest absolute error and
    its largest relative error over the entries whose true value is non-zero."""
    model = model_of(name)
    ev, el, iv = model.engine_eigen()
    out = {}
    for rmn in P_RATE_MODELS:
        T, lens, rates = g[rmn + "_P"], g[rmn + "_len"], g[rmn + "_rates"]
        O = np.array([[orc.pmatrix(ev, el, iv, t, rates) for t in row] for row in lens])
        out[rmn + "_E_orc_abs"], out[rmn + "_E_orc_rel"] = CK.p_errors(O, T)
    return out


def oracle_errors_tree8(orc, g, name):
    """The E_orc_* entries of hp_tree8_<name>: per pattern |site lnL error| (0 where the truth is
    -inf), the total's relative error, every edge quantity's error relative to max(1, |value|)
    -- each the largest over the roundings described above, with the oracle's own as E_orc0_* --
    and E_orc_P0 = the largest |P(0) - I| of the oracle."""
    model = model_of(name)
    ev, el, iv = model.engine_eigen()
    K = len(model.freqs)
    out = {"E_orc_P0": np.float64(np.abs(orc.pmatrix(ev, el, iv, 0.0, [1.0])[0] - np.eye(K)).max())}
    order = ["r5"] + [r for r in T8_ROOTINGS if r != "r5"]
    for rmn in TREE_RATE_MODELS:
        rm = rate_model_of(rmn)
        out.update(_site_errors(orc, g, rmn, [_rooting_of(text(g["newick_" + r]), T8_NAMES, g)
                                              for r in order], model, rm))
        out.update(_site_errors(orc, g, rmn + "_z", [_rooting_of(t8_newick(r, 0.0), T8_NAMES, g)
                                                     for r in order], model, rm))
        for r in EDGE_ROOTINGS:
            err = CK.deriv_error(edge_draws(orc, g, model, rm, r, rmn),
                                 g["%s_edge_%s" % (rmn, r)][None])
            out["%s_E_orc_edge_%s" % (rmn, r)] = err.max(axis=0)
            out["%s_E_orc0_edge_%s" % (rmn, r)] = err[0]
    return out


def oracle_errors_deep(orc, g):
    """hp_deep: the caterpillar's own rooting and three more, at a quarter, half and three
    quarters of its depth."""
    tips, ops, lens, re, rl, nn = _rooting_of(text(g["newick"]), DEEP_NAMES, g)
    rootings = [(tips, ops, lens, re, rl, nn)]
    for o in (len(ops) // 4, len(ops) // 2, 3 * len(ops) // 4):
        edge = (int(ops[o][0]), int(ops[o][2]))
        ops2, lens2, t = reroot(ops, lens, re, rl, edge)
        rootings.append((tips, ops2, lens2, edge, t, nn))
    return _site_errors(orc, g, "g05", rootings, model_of("gtr"), rate_model_of("g05"))
