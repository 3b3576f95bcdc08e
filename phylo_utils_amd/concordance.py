"""Concordance factors of every internal branch of a tree: how much the sites (sCF)
and a set of trees (gCF) agree with a branch, beside the supports that measure sampling variance
(Minh, Hahn & Lanfear 2020).  The reference has no concordance factors; the rule is DESIGN 4.29's.

The tree is an edge list ``[2n-3][2]`` in DESIGN 4.22's form -- tips ``0..n-1`` are the alignment's
rows, internal nodes ``n..2n-3`` -- or a ``tree.Tree`` / Newick string, which is brought to its op
order (``parsimony.tree_schedule``: edge ``2i`` = (left_i, parent_i), ``2i+1`` = (right_i,
parent_i), then the root edge).  Edge ``e = (x, y)`` is internal iff both ends are internal nodes;
x's other two edges, in increasing edge id, lead to clades A and B, y's to C and D.

* ``site_concordance`` -- per branch up to ``n_quartets`` quartets (a, b, c, d), one tip of each
  clade: all ``m = |A||B||C||D|`` of them where ``m <= n_quartets``, else draws of the library's
  Philox stream (counter word 3 = 2).  Per quartet the weighted numbers of decisive patterns --
  all four codes a single state -- that support ab|cd, ac|bd and ad|bc come from the HIP kernels of
  ``pu_scf.hip`` (pu_scf_counts); the means over the quartets are taken here in float64.
* ``gene_concordance`` -- the share of a tree set that holds AB|CD, AC|BD and AD|BC, looked up in
  the split table of ``treeset.compare`` (pu_treeset_compare).
* ``label_tree`` -- the values as labels of the internal nodes of a copy of the tree.

There is no host fallback: every count and every split table comes from the device.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from . import treeset
from .parsimony import _alignment, _prepared_schedule, integer_weights
from .tree import Traversal, Tree, prepare_tree

SITE_FIELDS = ("sCF", "sDF1", "sDF2", "sN", "sQ")
GENE_FIELDS = ("gCF", "gDF1", "gDF2", "gDFP", "gN")


class ConcordanceResult(object):
    """``edges`` int32 [2n-3][2] and ``internal`` (the ids of its internal edges, ascending);
    every factor is an array over ``internal``.  Site factors (None without them): ``sCF``,
    ``sDF1``, ``sDF2`` in percent, ``sN`` the mean number of decisive sites, ``sQ`` the number of
    quartets with a decisive site; ``nq`` int32 [2n-3], ``counts`` uint64 [2n-3][Q][3] and
    ``taxa`` int32 [2n-3][Q][4], the device's result by edge id.  Gene factors (None without
    them): ``gCF``, ``gDF1``, ``gDF2``, ``gDFP`` in percent and ``gN``.  ``tree`` and ``pairs``
    (a tree given as ``Tree`` or Newick only): the prepared tree and per edge its ends as
    ``Traversal`` node indices, child end first; ``names`` the tips' labels in row order."""

    def __init__(self, edges, names=None, tree=None, pairs=None):
        self.edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self.n = (len(self.edges) + 3) // 2
        self.internal = np.flatnonzero((self.edges >= self.n).all(axis=1))
        self.names = None if names is None else [str(x) for x in names]
        self.tree = tree
        self.pairs = pairs
        self.nq = self.counts = self.taxa = None
        for f in SITE_FIELDS + GENE_FIELDS:
            setattr(self, f, None)


def _tree_edges(tree, names, prepared=False):
    """(edges int32 [2n-3][2], prepared Tree or None, pairs or None) of a Tree, a Newick string
    or an edge list."""
    if isinstance(tree, (str, Tree)):
        if names is None:
            raise ValueError("mapping a Tree onto rows needs their names")
        t = tree if prepared and isinstance(tree, Tree) else prepare_tree(tree)
        ops, root, pairs = _prepared_schedule(t, names)
        # op order: (left_i, parent_i), (right_i, parent_i) per op, then the root edge
        ops = np.asarray(ops, dtype=np.int32).reshape(-1, 3)
        edges = np.concatenate([ops[:, [1, 0, 2, 0]].reshape(-1, 2),
                                np.asarray(root, dtype=np.int32).reshape(1, 2)])
        return np.ascontiguousarray(edges, dtype=np.int32), t, pairs
    e = np.ascontiguousarray(tree, dtype=np.int32)
    if e.ndim != 2 or e.shape[1] != 2 or e.shape[0] % 2 != 1:
        raise ValueError("a tree is a Tree, a Newick string or an edge list [2n-3][2], not %r"
                         % (e.shape,))
    return e, None, None


def finish(counts, nq):
    """The float64 finish of DESIGN 4.29 for one branch: (sCF, sDF1, sDF2, sN, sQ) of counts
    [Q][3] and the branch's number of quartets.  Over the quartets with t = n1 + n2 + n3 > 0: 100
    times the means of n1 / t, n2 / t, n3 / t, the mean of t, and their number; without one the
    factors are NaN and sN is 0."""
    c = np.asarray(counts[:int(nq)], dtype=np.uint64).reshape(-1, 3)
    t = c.sum(axis=1)
    live = t > 0
    k = int(live.sum())
    if k == 0:
        return np.nan, np.nan, np.nan, 0.0, 0
    tf = t[live].astype(np.float64)
    share = [100.0 * float(np.mean(c[live, i].astype(np.float64) / tf)) for i in range(3)]
    return share[0], share[1], share[2], float(np.mean(tf)), k


def site_concordance(coded_alignment, tree, n_quartets=100, seed=0, weights=None, device=0,
                     _prepared=False):
    """pu_scf_counts and the finish: the site concordance factors of every internal branch of
    `tree` (a ``Tree``, a Newick string or an edge list [2n-3][2]) on the coded alignment
    ``(codes [n][n_pat], table [n_codes][K], names)`` with integer pattern `weights` (None: all
    1).  Returns a ``ConcordanceResult`` with the site fields set."""
    codes, table, names = _alignment(coded_alignment)
    n, n_pat = codes.shape
    edges, prepared, pairs = _tree_edges(tree, names, _prepared)
    if len(edges) != 2 * n - 3:
        raise ValueError("%d rows need an edge list of %d edges, not %d"
                         % (n, 2 * n - 3, len(edges)))
    Q = int(n_quartets)
    w = integer_weights(weights, n_pat)
    E = len(edges)
    counts = np.zeros((E, max(Q, 0), 3), dtype=np.uint64)
    nq = np.zeros(E, dtype=np.int32)
    taxa = np.zeros((E, max(Q, 0), 4), dtype=np.int32)
    N.check(N.lib().pu_scf_counts(int(device), n, n_pat, table.shape[0], table.shape[1],
                                  N.ptr(codes), N.ptr(table), N.ptr(w), N.ptr(edges), Q,
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, N.ptr(counts), N.ptr(nq),
                                  N.ptr(taxa)), None, "pu_scf_counts")
    r = ConcordanceResult(edges, names, prepared, pairs)
    r.nq, r.counts, r.taxa = nq, counts, taxa
    rows = np.array([finish(counts[e], nq[e]) for e in r.internal], dtype=np.float64).reshape(-1, 5)
    r.sCF, r.sDF1, r.sDF2, r.sN = (rows[:, i].copy() for i in range(4))
    r.sQ = rows[:, 4].astype(np.int64)
    return r


def branch_clades(edges):
    """{internal edge id: (A, B, C, D)} of an edge list, every clade a Python int whose bit i is
    tip i: for e = (x, y) the tips beyond x's other two edges in increasing edge id, then y's."""
    edges = np.asarray(edges).reshape(-1, 2)
    n = (len(edges) + 3) // 2
    n_nodes = 2 * n - 2
    adj = [[] for _ in range(n_nodes)]
    for g, (a, b) in enumerate(edges):
        a, b = int(a), int(b)
        if not (0 <= a < n_nodes and 0 <= b < n_nodes) or a == b:
            raise ValueError("edge %d = (%d, %d) of %d nodes" % (g, a, b, n_nodes))
        adj[a].append((g, b))
        adj[b].append((g, a))
    if any(len(adj[v]) != (1 if v < n else 3) for v in range(n_nodes)):
        raise ValueError("the edges are no binary tree over %d tips" % n)
    # rooted on edge 0: below[v] = the tips on v's side of the edge to its parent
    r0, r1 = int(edges[0, 0]), int(edges[0, 1])
    par = {r0: r1, r1: r0}
    order, stack = [], [r0, r1]
    while stack:
        v = stack.pop()
        order.append(v)
        for g, f in adj[v]:
            if f != par[v]:
                par[f] = v
                stack.append(f)
    if len(order) != n_nodes:
        raise ValueError("the edges are not connected")
    below = [0] * n_nodes
    for v in reversed(order):
        if v < n:
            below[v] = 1 << v
        if v not in (r0, r1):
            below[par[v]] |= below[v]
    full = (1 << n) - 1
    out = {}
    for e, (x, y) in enumerate(edges):
        x, y = int(x), int(y)
        if x < n or y < n:
            continue
        # beyond an edge seen from `end`: below f where f hangs under `end` (the ends of edge 0
        # hang under each other), else everything that is not below `end`
        out[e] = tuple(below[f] if par[f] == end else full ^ below[end]
                       for end in (x, y) for g, f in adj[end] if g != e)
    return out


def _ref_edges(ref, names, prepared=False):
    """The reference tree of ``gene_concordance`` as an edge list in its form's own edge order."""
    if isinstance(ref, (str, Tree)):
        return _tree_edges(ref, names, prepared)
    e, _ = treeset.edge_lists(ref, names)
    if len(e) != 1:
        raise ValueError("the reference is one tree")
    return np.ascontiguousarray(e[0]), None, None


def gene_concordance(ref, trees, names=None, device=0, form=None, _prepared=False):
    """The gene concordance factors of every internal branch of `ref` in the tree set `trees`
    (any of the three forms ``treeset.compare`` takes, all T trees over the same n tips as
    `ref`; `ref` is a ``Tree`` or Newick, which needs `names`, or one tree in array form).  For
    a branch with clades A, B, C, D: ``gCF`` is 100 times the share of the T trees whose split
    table holds AB|CD, ``gDF1`` the same for AC|BD, ``gDF2`` for AD|BC, ``gDFP = 100 - gCF - gDF1
    - gDF2`` and ``gN = T``.  The split table and its counts are ``treeset.compare``'s, made on
    the device; the three bitsets per branch are built here in its convention, the side without
    tip 0.  Trees with missing taxa are refused, as ``treeset.compare`` refuses them: every tree
    must hold exactly the tips of `ref`.  Returns a ``ConcordanceResult`` with the gene fields
    set."""
    r = treeset.compare(trees, names=names, rows=0, device=device, form=form)
    n, T, names = r.n, r.n_trees, r.names
    edges, prepared, pairs = _ref_edges(ref, names, _prepared)
    if len(edges) != 2 * n - 3:
        raise ValueError("the reference has %d edges, the trees have %d tips" % (len(edges), n))
    nw = (n + 63) // 64
    table = {row.tobytes(): int(c) for row, c in zip(np.ascontiguousarray(r.bits), r.count)}
    full, word = (1 << n) - 1, (1 << 64) - 1

    def share(s):
        if s & 1:
            s = full ^ s
        key = np.array([(s >> (64 * w)) & word for w in range(nw)], dtype=np.uint64).tobytes()
        return 100.0 * (table.get(key, 0) / float(T))  # 100 x treeset.support's frequency

    out = ConcordanceResult(edges, names, prepared, pairs)
    clades = branch_clades(edges)
    rows = np.array([[share(A | B), share(A | C), share(A | D)]
                     for A, B, C, D in (clades[int(e)] for e in out.internal)],
                    dtype=np.float64).reshape(-1, 3)
    out.gCF, out.gDF1, out.gDF2 = rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()
    out.gDFP = 100.0 - out.gCF - out.gDF1 - out.gDF2
    out.gN = np.full(len(out.internal), T, dtype=np.int64)
    return out


def merge(site, gene):
    """One result with `site`'s site fields and `gene`'s gene fields (the same tree)."""
    if not np.array_equal(site.edges, gene.edges):
        raise ValueError("the two results are not of one tree")
    for f in GENE_FIELDS:
        setattr(site, f, getattr(gene, f))
    return site


def format_value(v, fmt="%.1f"):
    return "NA" if v is None or (isinstance(v, float) and np.isnan(v)) else fmt % v


def labels(result, keys=None, fmt="%.1f"):
    """{``Traversal`` node index: label} of the internal edges of a result made from a ``Tree``:
    the values of `keys` (default: gCF and sCF, those the result has) joined by ``/`` on the
    edge's child end -- for the root edge the seed's first child, where ``support.label_tree``
    puts its label too."""
    if result.pairs is None:
        raise ValueError("labels need a result made from a Tree or a Newick string")
    if keys is None:
        keys = [k for k in ("gCF", "sCF") if getattr(result, k) is not None]
    for k in keys:
        if getattr(result, k, None) is None:
            raise ValueError("the result has no %s" % k)
    return {int(result.pairs[int(e)][0]):
            "/".join(format_value(float(getattr(result, k)[i]), fmt) for k in keys)
            for i, e in enumerate(result.internal)}


def label_tree(tree, result, keys=None, fmt="%.1f", prefix=None):
    """A copy of the prepared `tree` (None: ``result.tree``; the numbering the result was made
    on) whose internal edges carry ``labels(result, keys, fmt)`` as the label of the edge's child
    end, as ``treeset.support`` and ``support.label_tree`` label theirs.  `prefix` ({node index:
    text}, say the SH-aLRT/aBayes labels) comes first, joined by ``/``."""
    lab = labels(result, keys, fmt)
    base = result.tree if tree is None else tree
    t = prepare_tree(base) if isinstance(base, str) else base.copy()
    node = {i: x for x, i in Traversal(t).node_dict.items()}
    for i, text in lab.items():
        if node[i].is_leaf():
            raise ValueError("node %d is a leaf" % i)
        head = None if prefix is None else prefix.get(i)
        node[i].label = text if head is None else "%s/%s" % (head, text)
    return t


def profile(on, device=0):
    """Switch the event timing of ``site_concordance`` on `device` on or off."""
    N.check(N.lib().pu_scf_profile(int(device), int(bool(on))), None, "pu_scf_profile")


def kernel_ms(device=0):
    """(picks, states, counts): the kernel times of the last ``site_concordance`` on `device`
    while profiling, in ms, summed over its chunks."""
    p, s, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    N.check(N.lib().pu_scf_kernel_ms(int(device), ctypes.byref(p), ctypes.byref(s),
                                     ctypes.byref(c)), None, "pu_scf_kernel_ms")
    return p.value, s.value, c.value
