"""Phylogenetic placement of query sequences on a TreeModel's resident partials (DESIGN 4.19;
the reference has none).

The reference tree and alignment stay fixed; every query is attached to the tree without
rebuilding it.  While the optimising traversal stands on edge (NOD, PAR), ``partials[NOD]`` holds
the subtree below NOD and ``partials[PAR]``, re-oriented, everything else, so a query joined at
the edge's midpoint is a third vector meeting those two at a new node: its likelihood is a local
computation, at the same cost for any tree size.  One walk scores every query at every edge at a
fixed pendant length (``pu_place_prescore``: per edge a per-pattern log table, then a
gather-and-sum per query); a second walk optimises the pendant length of the best few edges of
every query inside a kernel (``pu_place_refine``).  By the pulley principle the refined lnL is
the lnL of the (N+1)-taxon tree with the edge split into halves and the query on a branch of the
pendant length, every other length unchanged.

* ``place(tm, queries, keep=5)``     -- pre-score, candidate selection, refinement, LWR.
* ``prescore`` / ``refine`` / ``place_edge`` -- the three device calls on encoded queries.
* ``attach(tree, edge, name, pendant)`` -- the tree with a query joined at an edge's midpoint.
* ``write_jplace(path, tree, result)`` -- jplace version 3.

Not built: the attachment point stays at the midpoint (no proximal-position optimisation), the
edge's own length is not re-optimised, queries are dense over all columns (no sparse site
lists), one device.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import _native as N
from . import alignment as A
from .nni import _check
from .tree import Node, Traversal, prepare_tree, with_lengths

MAX_CODES = 32  # rows of a query code table (pu_place.hip kMaxCodes)
JPLACE_FIELDS = ["edge_num", "likelihood", "like_weight_ratio", "distal_length",
                 "pendant_length"]


def place_max_cat(n_states):
    """The largest category count the placement kernels take for 2, 4 or 20 states."""
    n = N.lib().pu_place_max_cat(int(n_states))
    if n < 0:
        raise ValueError("placement does not support %d states" % n_states)
    return n


# ------------------------------------------------------------------ queries
def encode_queries(tm, queries, alphabet=None):
    """dict(names, codes uint8 [Q][n_sites], table [n_codes][K], site_pattern int32 [n_sites] or
    None, site_weight [n_sites] or None) for the device calls.  `queries` is [(name, seq)] (or a
    dict, or records with .name/.seq) of the alignment's full, uncompressed length, encoded with
    the code table of `alphabet` (default: the alphabet of ``tm.set_alignment``); or an already
    coded triple (names, codes, table).  Columns map to the model's patterns through
    ``tm.inverse_index``; where the model holds one pattern per column (no compression) the
    pattern weights are the columns' weights."""
    if isinstance(queries, tuple) and len(queries) == 3 and isinstance(queries[1], np.ndarray):
        names, codes, table = queries
        names = list(names)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        table = np.ascontiguousarray(table, dtype=np.float64)
    else:
        alphabet = getattr(tm, "_alphabet", None) if alphabet is None else alphabet
        if alphabet is None:
            raise ValueError("place: sequences need an alphabet (the model's alignment was not "
                             "set from sequences)")
        codes, table, by_name = A.char_codes(queries, alphabet)
        names = sorted(by_name, key=by_name.get)
    K = tm.alignment.shape[2]
    if codes.ndim != 2 or table.ndim != 2 or table.shape[1] != K or len(names) != len(codes):
        raise ValueError("place: queries of shape %s on a table of shape %s for %d states"
                         % (codes.shape, table.shape, K))
    if len(table) > MAX_CODES:
        raise ValueError("place: a query code table has at most %d rows" % MAX_CODES)
    ii = np.asarray(tm.inverse_index)
    n_pat = tm._n_patterns()
    if codes.shape[1] != len(ii):
        raise ValueError("place: queries have %d columns, the alignment %d"
                         % (codes.shape[1], len(ii)))
    identity = len(ii) == n_pat and np.array_equal(ii, np.arange(n_pat))
    return dict(names=names, codes=codes, table=table,
                site_pattern=None if identity else np.ascontiguousarray(ii, dtype=np.int32),
                site_weight=N.f64(tm.siteweights) if identity else None)


def _query_args(q):
    codes = q["codes"]
    return (codes.shape[0], codes.shape[1], N.ptr(codes), N.ptr(q["site_pattern"]),
            N.ptr(q["site_weight"]), len(q["table"]), N.ptr(q["table"]))


def default_pendant(tm):
    """The tree's mean edge length (at least the optimisers' lower bound)."""
    return max(float(np.mean(list(tm.traversal.brlens.values()))), 1e-8)


# ------------------------------------------------------------------ device calls
def place_edge(tm, q, node, other, length=None, pendant0=None, tol=1e-8, max_iter=50):
    """All queries of `q` (``encode_queries``) at edge (node, other) on the nodes' current
    partials, at `length` (None: the edge's current length) (pu_place_edge): dict(score [Q] at
    pendant0, pendant [Q], lnl [Q], derivs [Q][2]).  max_iter = 0: the pre-score alone.  Changes
    nothing in the model."""
    _check(tm, "place_edge")
    tm._ensure()
    Q = len(q["codes"])
    t = float(tm.traversal.brlens[int(node), int(other)]) if length is None else float(length)
    l0 = default_pendant(tm) if pendant0 is None else float(pendant0)
    score, pendant, lnl, derivs = np.zeros(Q), np.zeros(Q), np.zeros(Q), np.zeros((Q, 2))
    N.check(N.lib().pu_place_edge(tm._ctx, int(node), int(other), t, *_query_args(q), l0,
                                  float(tol), int(max_iter), N.ptr(score), N.ptr(pendant),
                                  N.ptr(lnl), N.ptr(derivs)), tm._ctx, "pu_place_edge")
    return dict(score=score, pendant=pendant, lnl=lnl, derivs=derivs)


def prescore(tm, q, pendant0=None):
    """Every query at every edge at pendant length `pendant0` in one pass of the optimising
    traversal (pu_place_prescore): dict(edges int32 [E][2] = (NOD, PAR), lengths [E], scores
    [E][Q], pendant0), E = 2N - 3 edges in the order the traversal meets them, row 0 the root
    edge.  The model's partials, lnL and sitewise lnL are left as a traversal leaves them."""
    _check(tm, "prescore")
    tm._ensure()
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    Q = len(q["codes"])
    cap = max(2 * len(tm.names) - 3, 1)
    l0 = default_pendant(tm) if pendant0 is None else float(pendant0)
    edges = np.zeros((cap, 2), dtype=np.int32)
    lengths = np.zeros(cap)
    scores = np.zeros((cap, Q))
    n = ctypes.c_int()
    N.check(N.lib().pu_place_prescore(tm._ctx, len(rows), N.ptr(rows), *_query_args(q), l0,
                                      N.ptr(edges), N.ptr(lengths), N.ptr(scores),
                                      ctypes.byref(n)), tm._ctx, "pu_place_prescore")
    tm._site_valid = True
    n = n.value
    return dict(edges=edges[:n], lengths=lengths[:n], scores=scores[:n], pendant0=l0)


def refine(tm, q, candidates, n_edges, pendant0=None, tol=1e-8, max_iter=50):
    """The pendant length of every (edge_num, query) pair of `candidates` optimised by the
    library's Newton rule from `pendant0`, in one pass of the optimising traversal
    (pu_place_refine); edge numbers are ``prescore``'s, `n_edges` their count.  Returns
    dict(edge_num, query int32 [n], pendant, lnl [n], derivs [n][2], iters int32 [n]) sorted by
    (edge_num, query)."""
    _check(tm, "refine")
    tm._ensure()
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    cand = sorted(set((int(e), int(k)) for e, k in candidates))
    if cand and not (0 <= cand[0][0] and cand[-1][0] < n_edges):
        raise ValueError("refine: an edge number outside [0, %d)" % n_edges)
    e_num = np.array([e for e, _ in cand], dtype=np.int32)
    query = np.ascontiguousarray([k for _, k in cand], dtype=np.int32)
    off = np.zeros(n_edges + 1, dtype=np.int64)
    np.cumsum(np.bincount(e_num, minlength=n_edges), out=off[1:])
    n = max(len(cand), 1)
    l0 = default_pendant(tm) if pendant0 is None else float(pendant0)
    pendant, lnl, derivs = np.zeros(n), np.zeros(n), np.zeros((n, 2))
    iters = np.zeros(n, dtype=np.int32)
    N.check(N.lib().pu_place_refine(tm._ctx, len(rows), N.ptr(rows), *_query_args(q), l0,
                                    float(tol), int(max_iter), int(n_edges), N.ptr(off),
                                    N.ptr(query), N.ptr(pendant), N.ptr(lnl), N.ptr(derivs),
                                    N.ptr(iters)), tm._ctx, "pu_place_refine")
    tm._site_valid = True
    k = len(cand)
    return dict(edge_num=e_num, query=query, pendant=pendant[:k], lnl=lnl[:k], derivs=derivs[:k],
                iters=iters[:k])


def kernel_ms(tm):
    """(table, prescore, newton) HIP-event times in ms of the last launches made while the
    context profiled (pu_place_kernel_ms)."""
    out = [ctypes.c_double() for _ in range(3)]
    N.check(N.lib().pu_place_kernel_ms(tm._ctx, *[ctypes.byref(v) for v in out]), tm._ctx,
            "pu_place_kernel_ms")
    return tuple(v.value for v in out)


# ------------------------------------------------------------------ placement
def select_candidates(scores, keep):
    """[Q] lists of edge numbers: per query the `keep` best pre-scores, descending, ties by edge
    order (scores [E][Q])."""
    scores = np.asarray(scores)
    keep = max(1, min(int(keep), scores.shape[0]))
    return [np.argsort(-scores[:, k], kind="stable")[:keep].tolist()
            for k in range(scores.shape[1])]


def weight_ratios(lnl):
    """exp(lnL - max) / sum over one query's refined candidates."""
    lnl = np.asarray(lnl, dtype=np.float64)
    w = np.exp(lnl - lnl.max())
    return w / w.sum()


def place(tm, queries, keep=5, pendant0=None, tol=1e-8, max_iter=50, alphabet=None):
    """Place `queries` (``encode_queries``) on the model's tree: the pre-score of every query at
    every edge at `pendant0` (default: the tree's mean edge length), then, per query, the `keep`
    best edges (ties by edge order) refined by Newton on the pendant length.  Returns
    dict(names, edges [E][2], lengths [E], prescore [E][Q], pendant0, placements): per query the
    refined candidates sorted by lnL (ties by edge order), each dict(edge (NOD, PAR), edge_num,
    lnl, pendant, distal = half the edge's length, lwr = exp(lnL - max) / sum over that query's
    candidates, iters).  The model is left as a traversal leaves it."""
    q = encode_queries(tm, queries, alphabet)
    l0 = default_pendant(tm) if pendant0 is None else float(pendant0)
    pre = prescore(tm, q, l0)
    chosen = select_candidates(pre["scores"], keep)
    cand = [(e, k) for k, es in enumerate(chosen) for e in es]
    ref = refine(tm, q, cand, len(pre["edges"]), l0, tol, max_iter)
    by_query = [[] for _ in q["names"]]
    for i, (e, k) in enumerate(zip(ref["edge_num"], ref["query"])):
        by_query[k].append(dict(edge=(int(pre["edges"][e][0]), int(pre["edges"][e][1])),
                                edge_num=int(e), lnl=float(ref["lnl"][i]),
                                pendant=float(ref["pendant"][i]),
                                distal=0.5 * float(pre["lengths"][e]),
                                iters=int(ref["iters"][i])))
    for rows in by_query:
        rows.sort(key=lambda r: (-r["lnl"], r["edge_num"]))
        for r, w in zip(rows, weight_ratios([r["lnl"] for r in rows])):
            r["lwr"] = float(w)
    return dict(names=q["names"], edges=pre["edges"], lengths=pre["lengths"],
                prescore=pre["scores"], pendant0=l0, placements=by_query)


# ------------------------------------------------------------------ trees
def attach(tree, edge, name, pendant):
    """prepare_tree(tree) with leaf `name` joined at the midpoint of `edge` = (a, b), two node
    indices of Traversal(prepare_tree(tree)) joined by an edge, on a branch of length `pendant`:
    the edge is split into two halves at a new node, every other length is kept.  The result is
    a binary Tree."""
    t = prepare_tree(tree)
    tr = Traversal(t)
    node = {i: n for n, i in tr.node_dict.items()}
    a, b = int(edge[0]), int(edge[1])
    if a not in node or b not in node:
        raise ValueError("no node %r or %r in the tree" % (a, b))
    if name in tr.names:
        raise ValueError("the tree already has a leaf %r" % name)
    na, nb = node[a], node[b]
    seed = t.seed_node
    left, right = seed.children
    leaf = Node(name, float(pendant))
    if (na is left and nb is right) or (na is right and nb is left):
        half = 0.5 * float(tr.brlens[a, b])
        new = Node(None, half)
        seed.children = []
        seed.add(new)
        seed.add(right)
        left.length, right.length = half, 0.0
        new.add(left)
        new.add(leaf)
        return t
    child, par = (na, nb) if na.parent is nb else (nb, na)
    if child.parent is not par:
        raise ValueError("nodes %d and %d are not joined by an edge" % (a, b))
    half = 0.5 * child.edge_length
    new = Node(None, half)
    par.children[par.children.index(child)] = new
    new.parent = par
    child.length = half
    new.add(child)
    new.add(leaf)
    return t


def current_tree(tm):
    """The model's prepared tree at its current branch lengths."""
    return with_lengths(tm.tree, tm.traversal.brlens)


def jplace_tree(tree, edges):
    """The jplace tree string of the prepared `tree`: unrooted (the seed's zero-length child is
    dissolved, so that every node below the seed is one edge), ``{edge_num}`` after every length,
    edge numbers the rows of `edges` [E][2] = (NOD, PAR) over Traversal(tree)'s node indices."""
    t = tree.copy()
    tr = Traversal(t)
    num = {}
    for k, (nod, par) in enumerate(np.asarray(edges).tolist()):
        num[nod] = k
    seed = t.seed_node
    left, right = seed.children
    length = float(tr.brlens[tr.root_edge])
    drop, keep = (right, left) if right.children else (left, right)
    if not drop.children:
        raise ValueError("a tree of two leaves has no unrooted form")
    k_root = num.get(tr.node_dict[left], num.get(tr.node_dict[right]))
    edge_of = {n: num[i] for n, i in tr.node_dict.items() if n is not drop and i in num}
    edge_of[keep] = k_root
    keep.length = length
    pos = seed.children.index(drop)
    for c in drop.children:
        c.parent = seed
    seed.children[pos:pos + 1] = drop.children
    parts = {}
    for n in seed.postorder():
        s = ""
        if n.children:
            s = "(" + ",".join(parts.pop(id(c)) for c in n.children) + ")"
        if n.label is not None:
            s += n.label if all(ch not in n.label for ch in " (),:;[]'{}") else \
                "'" + n.label.replace("'", "''") + "'"
        if n is not seed:
            s += ":%s{%d}" % (repr(float(n.edge_length)), edge_of[n])
        parts[id(n)] = s
    return parts[id(seed)] + ";"


def jplace(tree, result, invocation="phylo_utils_amd.place"):
    """The jplace (version 3) document of a ``place`` result on the prepared `tree` it was
    computed on, as a dict."""
    placements = []
    for name, rows in zip(result["names"], result["placements"]):
        placements.append(dict(
            p=[[r["edge_num"], r["lnl"], r["lwr"], r["distal"], r["pendant"]] for r in rows],
            n=[name]))
    return dict(tree=jplace_tree(tree, result["edges"]), placements=placements,
                metadata=dict(invocation=invocation), version=3, fields=list(JPLACE_FIELDS))


def write_jplace(path, tree, result, invocation="phylo_utils_amd.place"):
    """Write ``jplace(tree, result)`` to `path` as JSON."""
    with open(path, "w") as fh:
        json.dump(jplace(tree, result, invocation), fh, indent=1)
        fh.write("\n")
