"""Sets of trees compared on the GPU: the table of their distinct splits, a split id
per edge, the number of trees that hold each split, the Robinson-Foulds matrix; and what follows
from them on the host: split frequencies, topology classes, the majority-rule consensus tree and
the support of any tree's edges in any tree set.

The reference has no tree comparison; the rule is DESIGN 4.27's.  The trees share ``n`` tips
``0..n-1``; the split of an edge is the set of tips on its side without tip 0, a bitset of
``ceil(n / 64)`` uint64 words (tip i at bit ``i & 63`` of word ``i >> 6``); a pendant edge has no
split; ``U`` holds the distinct splits of all trees in ascending order as integers (the last word
the most significant), a split's id is its index in ``U``, ``count[u]`` the trees that hold it, and
``RF(a, b) = 2(n-3) - 2 |ids(a) & ids(b)|``.

A tree set is a list of ``tree.Tree`` or Newick strings (mapped to rows by `names` through
``parsimony.tree_schedule``), ``(ops [T][n-2][3], roots [T][2])`` arrays, an ``nj.nj_joins``-style
``(joins [T][n-2][2], roots [T][2])`` batch (``form="joins"``) or an edge batch ``[T][2n-3][2]``
as ``parsimony.stepwise_addition`` returns it (or a list of edge lists).  Each form has its own
edge order: op order (edge ``2i`` = (left_i, parent_i), ``2i+1`` = (right_i, parent_i), then the
root edge) for the first three, the list's own for an edge batch.

Trees with branch lengths: ``distances`` gives the weighted Robinson-Foulds,
branch-score (Kuhner-Felsenstein), path-difference and weighted path-difference distances,
``split_lengths`` the mean length of every split and of every tip's edge, which ``consensus``
writes onto its tree.  ``Tree`` and Newick bring their own lengths; the array forms take
``lengths [T][2n-3]`` in the form's edge order.

There is no host fallback for the device work: splits, ids, counts and distances come from the
HIP kernels of ``pu_treeset.hip`` and ``pu_treedist.hip``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .bootstrap import _join_arrays, support_label
from .parsimony import _prepared_schedule
from .tree import Node, Traversal, Tree, parse_newick, prepare_tree

FORMS = {"ops": 0, "joins": 1, "edges": 2}
METRICS = ("wrf", "kf", "path", "wpath")


class TreeSetResult(object):
    """What ``compare`` returns.  ``edge_ids`` int32 [T][2n-3] (-1 on a pendant edge), ``bits``
    uint64 [U][nw], ``count`` int32 [U], ``rf`` int32 [rows][T] (None where no row was asked
    for), ``n``, ``n_trees``, ``names`` (the tips' labels in row order, or None), ``form`` and
    ``edges`` int32 [T][2n-3][2]: every tree's edges as (child end, parent end) node pairs in the
    form's edge order.  ``pairs`` (trees given as ``Tree`` or Newick only) lists per tree the
    same edges as ``Traversal`` node indices of ``prepare_tree(tree)``."""

    def __init__(self, n, n_trees, bits, count, edge_ids=None, rf=None, names=None, form="ops",
                 edges=None, pairs=None):
        self.n = int(n)
        self.n_trees = int(n_trees)
        self.bits = np.asarray(bits, dtype=np.uint64).reshape(-1, max((self.n + 63) // 64, 1))
        self.count = np.asarray(count, dtype=np.int32).reshape(-1)
        if len(self.bits) != len(self.count):
            raise ValueError("%d splits with %d counts" % (len(self.bits), len(self.count)))
        self.edge_ids = edge_ids
        self.rf = rf
        self.names = None if names is None else [str(x) for x in names]
        if self.names is not None and len(self.names) != self.n:
            raise ValueError("%d names for %d tips" % (len(self.names), self.n))
        self.form = form
        self.edges = edges
        self.pairs = pairs

    @property
    def n_unique(self):
        return len(self.count)


def _op_edges(ops, roots):
    """[T][2n-3][2]: the edges of op lists in op order, child end first."""
    T, n_ops = ops.shape[:2]
    e = np.empty((T, 2 * n_ops + 1, 2), dtype=np.int32)
    e[:, 0:2 * n_ops:2, 0] = ops[:, :, 1]
    e[:, 1:2 * n_ops:2, 0] = ops[:, :, 2]
    e[:, 0:2 * n_ops:2, 1] = ops[:, :, 0]
    e[:, 1:2 * n_ops:2, 1] = ops[:, :, 0]
    e[:, 2 * n_ops] = roots
    return e


def _joins_as_ops(joins):
    T, n_ops = joins.shape[:2]
    ops = np.empty((T, n_ops, 3), dtype=np.int32)
    ops[:, :, 0] = n_ops + 2 + np.arange(n_ops, dtype=np.int32)
    ops[:, :, 1:] = joins
    return ops


def _batch_prepared(prepared, names):
    """_batch of trees that ``prepare_tree`` has prepared already."""
    if names is None:
        names = sorted(x.label for x in prepared[0].leaf_nodes())
    sched = [_prepared_schedule(t, names) for t in prepared]
    ops = np.ascontiguousarray(np.stack([s[0] for s in sched]), dtype=np.int32)
    ops = ops.reshape(len(sched), -1, 3)
    roots = np.ascontiguousarray(np.stack([s[1] for s in sched]), dtype=np.int32)
    return "ops", ops, roots, names, [s[2] for s in sched]


def _batch(trees, names, form):
    """(form, arrays int32 [T][..], roots [T][2] or None, names, pairs) of a tree set."""
    if form is not None and form not in FORMS:
        raise ValueError("form must be one of %s, not %r" % (sorted(FORMS), form))
    if isinstance(trees, (str, Tree)):
        trees = [trees]
    if isinstance(trees, list) and trees and all(isinstance(t, (str, Tree)) for t in trees):
        return _batch_prepared([prepare_tree(t) for t in trees], names)
    if isinstance(trees, (tuple, list)) and trees and not isinstance(trees[0], (str, Tree)):
        shapes = [np.shape(x) for x in trees]
        if len(shapes[0]) == 2 and shapes[0][1] == 2 and shapes[0][0] % 2 == 1 \
                and all(sh == shapes[0] for sh in shapes):
            trees = np.stack([np.asarray(x) for x in trees])  # a list of edge lists
    if isinstance(trees, (tuple, list)) and len(trees) in (2, 4, 5) and not isinstance(trees[0], (str, Tree)):
        a, roots = _join_arrays(trees)
        if a.ndim == 2:
            a, roots = a[None], roots.reshape(1, 2)
        if a.ndim != 3 or a.shape[2] not in (2, 3) or roots.shape != (len(a), 2):
            raise ValueError("a tree set of arrays is (ops [T][n-2][3] or joins [T][n-2][2], "
                             "roots [T][2]), not %r and %r" % (a.shape, roots.shape))
        got = "ops" if a.shape[2] == 3 else "joins"
        if form not in (None, got):
            raise ValueError("form=%r, but the arrays are the %s form" % (form, got))
        return got, np.ascontiguousarray(a), np.ascontiguousarray(roots), names, None
    e = np.asarray(trees)
    if e.dtype.kind in "iu" and e.ndim in (2, 3) and e.shape[-1] == 2 and form in (None, "edges"):
        e = np.ascontiguousarray(e if e.ndim == 3 else e[None], dtype=np.int32)
        return "edges", e, None, names, None
    raise ValueError("a tree set is a list of Tree or Newick, (ops, roots), (joins, roots) or an "
                     "edge batch [T][2n-3][2]")


def edge_lists(trees, names=None, form=None):
    """(edges int32 [T][2n-3][2], names): every tree of a tree set -- any form ``compare`` takes
    -- as (child end, parent end) node pairs in its form's own edge order, what
    ``TreeSetResult.edges`` holds, without a device call."""
    form, a, roots, names, _ = _batch(trees, names, form)
    if form == "edges":
        return a, names
    return _op_edges(a if form == "ops" else _joins_as_ops(a), roots), names


def compare(trees, names=None, rows=None, device=0, form=None, want_table=True):
    """pu_treeset_compare: the ``TreeSetResult`` of a tree set.  `rows` None: the full RF matrix
    [T][T]; an integer k: trees 0..k-1 against all, [k][T]; 0: no distances.  `want_table` False
    leaves ``bits`` and ``count`` out (empty)."""
    form, a, roots, names, pairs = _batch(trees, names, form)
    T = len(a)
    if T < 1:
        raise ValueError("no tree")
    n = a.shape[1] + 2 if form != "edges" else (a.shape[1] + 3) // 2
    if form == "edges" and a.shape[1] != 2 * n - 3:
        raise ValueError("an edge list has 2n-3 rows, not %d" % a.shape[1])
    if names is not None and len(names) != n:
        raise ValueError("%d names for trees of %d tips" % (len(names), n))
    k = T if rows is None else int(rows)
    E, ns, nw = 2 * n - 3, max(n - 3, 0), (n + 63) // 64
    edge_ids = np.empty((T, E), dtype=np.int32)
    U = np.zeros(1, dtype=np.int64)
    bits = np.zeros((T * ns, nw), dtype=np.uint64) if want_table else None
    count = np.zeros(T * ns, dtype=np.int32) if want_table else None
    rf = np.zeros((k, T), dtype=np.int32) if 0 < k <= T else None
    N.check(N.lib().pu_treeset_compare(int(device), n, T, FORMS[form], N.ptr(a), N.ptr(roots), k,
                                       N.ptr(edge_ids), N.ptr(U), N.ptr(bits), N.ptr(count),
                                       N.ptr(rf)), None, "pu_treeset_compare")
    u = int(U[0])
    if want_table:
        bits, count = bits[:u].copy(), count[:u].copy()
    else:
        bits, count = np.zeros((0, nw), dtype=np.uint64), np.zeros(0, dtype=np.int32)
    if form == "edges":
        edges = a
    else:
        edges = _op_edges(a if form == "ops" else _joins_as_ops(a), roots)
    return TreeSetResult(n, T, bits, count, edge_ids, rf, names, form, edges, pairs)


def rf_distances(trees, names=None, normalised=False, device=0, form=None):
    """The Robinson-Foulds matrix [T][T] of a tree set, int32; `normalised`: divided by
    ``2(n-3)``, float64 (all 0 for n = 3)."""
    r = compare(trees, names, None, device, form, want_table=False)
    if not normalised:
        return r.rf
    return r.rf / float(2 * (r.n - 3)) if r.n > 3 else np.zeros(r.rf.shape)


def split_frequencies(result):
    """``count / T``: the share of the trees that hold each split of ``result.bits``."""
    return result.count / float(result.n_trees)


def topology_classes(result):
    """int [T]: for every tree the index of the first tree with the same set of split ids."""
    first, out = {}, np.empty(result.n_trees, dtype=np.int64)
    for t, row in enumerate(np.asarray(result.edge_ids)):
        key = np.sort(row[row >= 0]).tobytes()
        out[t] = first.setdefault(key, t)
    return out


def split_tips(bits, n):
    """The tips of one split's bitset (uint64 [nw]), ascending."""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8)
    return np.flatnonzero(np.unpackbits(b, bitorder="little")[:n])


def consensus(result, threshold=0.5, min_length=None, lengths=None):
    """The majority-rule consensus tree of `result`'s trees: the splits with ``count / T >
    threshold`` -- at threshold 1.0 those with ``count == T``, the strict consensus -- nested by
    ascending tip count into a ``tree.Tree`` that may hold polytomies.  Every internal node that
    carries a split is labelled ``bootstrap.support_label(count / T)``; edges carry no length
    (`min_length` is accepted for the tree builders' common signature and has nothing to act
    on) unless `lengths` = ``(split_mean [U], tip_mean [n])`` of ``split_lengths`` is given: then
    the edge above every kept split and every tip's edge carries its mean length.  A kept split
    that holds all tips but tip 0 and one other cannot occur (it would be trivial), so no two
    kept nodes share an edge.  Thresholds outside [0.5, 1] are refused: below 0.5 the splits need
    not be compatible (greedy consensus is not offered)."""
    threshold = float(threshold)
    if not 0.5 <= threshold <= 1.0:
        raise ValueError("threshold must be within [0.5, 1], not %r" % threshold)
    n, T = result.n, result.n_trees
    if lengths is not None:
        split_mean, tip_mean = (np.asarray(x, dtype=np.float64).reshape(-1) for x in lengths)
        if len(split_mean) != result.n_unique or len(tip_mean) != n:
            raise ValueError("lengths is (split_mean [%d], tip_mean [%d]), not [%d] and [%d]"
                             % (result.n_unique, n, len(split_mean), len(tip_mean)))
    names = result.names if result.names is not None else [str(i) for i in range(n)]
    count = np.asarray(result.count, dtype=np.int64)
    keep = np.flatnonzero(count == T if threshold >= 1.0 else count > threshold * T)
    tips = [split_tips(result.bits[u], n) for u in keep]
    order = sorted(range(len(keep)), key=lambda i: (len(tips[i]), i))
    top = [Node(str(x)) for x in names]  # per tip: the highest node made so far that holds it
    if lengths is not None:
        for x, node in enumerate(top):
            node.length = float(tip_mean[x])
    for i in order:
        node = Node(support_label(count[keep[i]] / float(T)))
        if lengths is not None:
            node.length = float(split_mean[keep[i]])
        seen = set()
        for x in tips[i]:
            c = top[x]
            if id(c) not in seen:
                seen.add(id(c))
                node.add(c)
            top[x] = node
    seed, seen = Node(), set()
    for c in top:
        if id(c) not in seen:
            seen.add(id(c))
            seed.add(c)
    return Tree(seed)


def _edges_as_ops(edges):
    """(ops [T][n-2][3], roots [T][2]) of an edge batch, each tree rooted on its edge 0: the form
    conversion on the host that lets edge lists meet trees of another form."""
    T, E = edges.shape[:2]
    n = (E + 3) // 2
    ops = np.empty((T, n - 2, 3), dtype=np.int32)
    for t in range(T):
        adj = {}
        for a, b in edges[t]:
            adj.setdefault(int(a), []).append(int(b))
            adj.setdefault(int(b), []).append(int(a))
        if sorted(adj) != list(range(2 * n - 2)) or \
                any(len(adj[v]) != (1 if v < n else 3) for v in adj):
            raise ValueError("tree %d: the edges are no binary tree over %d tips" % (t, n))
        ra, rb = int(edges[t, 0, 0]), int(edges[t, 0, 1])
        out, stack = [], [(ra, rb, False), (rb, ra, False)]
        while stack:
            v, came, done = stack.pop()
            if v < n:
                continue
            kids = [x for x in adj[v] if x != came]
            if done:
                out.append((v, kids[0], kids[1]))
            else:
                stack.append((v, came, True))
                stack += [(x, v, False) for x in kids]
        if len(out) != n - 2:
            raise ValueError("tree %d: the edges are not connected" % t)
        ops[t] = out
    return ops, np.ascontiguousarray(edges[:, 0, :], dtype=np.int32)


def _as_ops(form, a, roots):
    if form == "ops":
        return a, roots
    if form == "joins":
        return _joins_as_ops(a), roots
    return _edges_as_ops(a)


def support(ref, trees, names=None, device=0, form=None):
    """The support of every edge of `ref` in the tree set `trees`: (support float64 [2n-3],
    tree).  ``compare`` runs on ``trees + [ref]``; per edge of `ref` in its edge order the value
    is ``(count[id] - 1) / T``, NaN on a pendant edge.  Where `ref` is a ``Tree`` or Newick,
    `tree` is ``prepare_tree(ref)`` with every internal node below an internal edge labelled
    ``bootstrap.support_label`` of it (both ends of the root edge), else None.  `ref` and `trees`
    may differ in form (a ``Tree`` against a batch of join arrays or of edge lists): the trees
    are then all brought to op lists on the host first."""
    fa, a, ra, names, _ = _batch(trees, names, form)
    prepared = None
    if isinstance(ref, (str, Tree)):
        prepared = prepare_tree(ref)
        if names is None:
            raise ValueError("mapping a Tree onto arrays needs the names of the rows")
        ops, root, pairs = _prepared_schedule(prepared, names)
        fb, b, rb = "ops", np.asarray(ops, dtype=np.int32).reshape(1, -1, 3), root.reshape(1, 2)
    else:
        fb, b, rb, _, _ = _batch(ref, names, form)
        if len(b) != 1:
            raise ValueError("the reference is one tree")
    if fa == fb:
        both = np.concatenate([a, b])
        roots = None if ra is None else np.concatenate([ra, rb])
        arg = both if fa == "edges" else (both, roots)
    else:
        (a, ra), (b, rb) = _as_ops(fa, a, ra), _as_ops(fb, b, rb)
        fa, arg = "ops", (np.concatenate([a, b]), np.concatenate([ra, rb]))
    r = compare(arg, names, 0, device, fa)
    T = r.n_trees - 1
    ids = r.edge_ids[-1]
    out = np.full(len(ids), np.nan)
    live = ids >= 0
    out[live] = (r.count[ids[live]] - 1) / float(T)
    if prepared is not None:
        index = {i: node for node, i in Traversal(prepared).node_dict.items()}
        for e, (c, p) in enumerate(pairs):
            if not live[e]:
                continue
            ends = (c, p) if e == len(pairs) - 1 else (c,)
            for v in ends:
                index[v].label = support_label(out[e])
    return out, prepared


def _tree_lengths(pairs_of, prepared):
    """float64 [T][2n-3]: the lengths of prepared trees in op edge order (the root edge's as
    ``Traversal`` gives it)."""
    out = []
    for pairs, p in zip(pairs_of, prepared):
        bl = Traversal(p).brlens
        out.append([float(bl[pair]) for pair in pairs])
    return np.array(out, dtype=np.float64)


def _refuse_missing_lengths(trees):
    """A ``Tree`` or Newick with an edge that has no length is refused, the tree named."""
    for t, tree in enumerate(trees):
        parsed = parse_newick(tree) if isinstance(tree, str) else tree
        seed = parsed.seed_node
        for node in seed.postorder():
            if node is not seed and node.length is None:
                raise ValueError("tree %d: the edge above %s has no length" % (
                    t, repr(node.label) if node.label is not None else "an internal node"))


def _batch_with_lengths(trees, names, form, lengths):
    """_batch and float64 lengths [T][2n-3] in the form's edge order, checked."""
    if isinstance(trees, (str, Tree)):
        trees = [trees]
    own = isinstance(trees, list) and trees and all(isinstance(t, (str, Tree)) for t in trees)
    if own:
        if lengths is not None:
            raise ValueError("Tree and Newick input brings its own lengths")
        _refuse_missing_lengths(trees)
        if form not in (None, "ops"):
            raise ValueError("form=%r, but Tree and Newick input is the ops form" % form)
        prepared = [prepare_tree(t) for t in trees]
        form, a, roots, names, pairs = _batch_prepared(prepared, names)
        lengths = _tree_lengths(pairs, prepared)
    else:
        form, a, roots, names, pairs = _batch(trees, names, form)
        if lengths is None:
            raise ValueError("the array forms need lengths [T][2n-3] in the form's edge order")
        lengths = np.ascontiguousarray(lengths, dtype=np.float64)
    T = len(a)
    n = a.shape[1] + 2 if form != "edges" else (a.shape[1] + 3) // 2
    if form == "edges" and a.shape[1] != 2 * n - 3:
        raise ValueError("an edge list has 2n-3 rows, not %d" % a.shape[1])
    if lengths.ndim == 1 and T == 1:
        lengths = lengths[None]
    if lengths.shape != (T, 2 * n - 3):
        raise ValueError("lengths must be [%d][%d], not %r" % (T, 2 * n - 3, lengths.shape))
    bad = np.argwhere(~(np.isfinite(lengths) & (lengths >= 0.0)))
    if len(bad):
        raise ValueError("tree %d edge %d: length %r is not a finite number >= 0"
                         % (bad[0][0], bad[0][1], float(lengths[tuple(bad[0])])))
    if names is not None and len(names) != n:
        raise ValueError("%d names for trees of %d tips" % (len(names), n))
    return form, a, roots, names, pairs, np.ascontiguousarray(lengths), n


def _treedist(form, a, roots, lengths, n, k, want, sums, device):
    """pu_treedist: dict of the matrices named in `want` ("wrf", "kf2", "path2", "wpath2") and,
    with `sums`, "U", "split_sum" [U] and "tip_sum" [n]."""
    T = len(a)
    out = {}
    for key in want:
        out[key] = np.zeros((k, T), dtype=np.uint64 if key == "path2" else np.float64)
    buf = {key: (out[key] if k > 0 and key in out else None)
           for key in ("wrf", "kf2", "path2", "wpath2")}
    U = np.zeros(1, dtype=np.int64) if sums else None
    ssum = np.zeros(max(T * (n - 3), 1), dtype=np.float64) if sums else None
    tsum = np.zeros(n, dtype=np.float64) if sums else None
    N.check(N.lib().pu_treedist(int(device), n, T, FORMS[form], N.ptr(a), N.ptr(roots),
                                N.ptr(lengths), k, N.ptr(buf["wrf"]), N.ptr(buf["kf2"]),
                                N.ptr(buf["path2"]), N.ptr(buf["wpath2"]), N.ptr(U), N.ptr(ssum),
                                N.ptr(tsum)), None, "pu_treedist")
    if sums:
        out["U"] = int(U[0])
        out["split_sum"] = ssum[:out["U"]].copy()
        out["tip_sum"] = tsum
    return out


_RAW = {"wrf": "wrf", "kf": "kf2", "path": "path2", "wpath": "wpath2"}


def distances(trees, metric, names=None, lengths=None, rows=None, device=0, form=None,
              squared=False):
    """pu_treedist: distances between trees with branch lengths, float64 [rows][T].  `metric`:
    ``"wrf"`` (weighted Robinson-Foulds, Robinson & Foulds 1979), ``"kf"`` (branch score, Kuhner
    & Felsenstein 1994), ``"path"`` (topological path difference, Steel & Penny 1993),
    ``"wpath"`` (the same on patristic distances), or a tuple of them: then a dict of arrays.
    `rows` as in ``compare``.  ``Tree`` and Newick input brings its own lengths (one without a
    length on some edge is refused); the array forms need `lengths` [T][2n-3] in the form's edge
    order.  ``kf``, ``path`` and ``wpath`` are the host's square roots of the device's sums of
    squares; `squared` True returns those sums themselves (``path``: uint64, exact)."""
    one = isinstance(metric, str)
    metrics = (metric,) if one else tuple(metric)
    for m in metrics:
        if m not in METRICS:
            raise ValueError("metric must be one of %s, not %r" % (list(METRICS), m))
    if not metrics:
        raise ValueError("no metric")
    form, a, roots, names, _, lengths, n = _batch_with_lengths(trees, names, form, lengths)
    T = len(a)
    k = T if rows is None else int(rows)
    if not 0 <= k <= T:
        raise ValueError("rows = %d is outside [0, %d]" % (k, T))
    raw = _treedist(form, a, roots, lengths, n, k, [_RAW[m] for m in metrics], False, device)
    out = {}
    for m in metrics:
        x = raw[_RAW[m]]
        out[m] = x if m == "wrf" or squared else np.sqrt(x.astype(np.float64))
    return out[metric] if one else out


def split_lengths(trees, names=None, lengths=None, device=0, form=None):
    """(result, split_mean [U], tip_mean [n]): ``compare``'s ``TreeSetResult`` of the tree set
    (no distances) and the mean length of every split of ``result.bits`` over the trees that hold
    it (the device's sum in ascending tree order / ``count``) and of every tip's edge (sum / T)."""
    form, a, roots, names, pairs, lengths, n = _batch_with_lengths(trees, names, form, lengths)
    arg = a if form == "edges" else (a, roots)
    result = compare(arg, names, 0, device, form)
    result.pairs = pairs
    raw = _treedist(form, a, roots, lengths, n, 0, [], True, device)
    if raw["U"] != result.n_unique:
        raise RuntimeError("pu_treedist and pu_treeset_compare disagree on the split table")
    return result, raw["split_sum"] / result.count, raw["tip_sum"] / float(result.n_trees)


def profile(on, device=0):
    """Switch the event timing of ``compare`` on `device` on or off."""
    N.check(N.lib().pu_treeset_profile(int(device), int(bool(on))), None, "pu_treeset_profile")


def kernel_ms(device=0):
    """(splits, ids, rf): the stage times of the last ``compare`` on `device` while profiling,
    in ms."""
    s, i, r = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    N.check(N.lib().pu_treeset_kernel_ms(int(device), ctypes.byref(s), ctypes.byref(i),
                                         ctypes.byref(r)), None, "pu_treeset_kernel_ms")
    return s.value, i.value, r.value


def distance_profile(on, device=0):
    """Switch the event timing of ``distances`` and ``split_lengths`` on `device` on or off."""
    N.check(N.lib().pu_treedist_profile(int(device), int(bool(on))), None, "pu_treedist_profile")


def distance_kernel_ms(device=0):
    """(ids, weighted, paths, path2, wpath2): the stage times of the last pu_treedist call on
    `device` while profiling, in ms."""
    v = [ctypes.c_double() for _ in range(5)]
    N.check(N.lib().pu_treedist_kernel_ms(int(device), *[ctypes.byref(x) for x in v]), None,
            "pu_treedist_kernel_ms")
    return tuple(x.value for x in v)
