"""Fitch parsimony on the GPU: tree lengths, exact insertion lengths and randomised
stepwise-addition trees; and parsimony SPR: the exact lengths of all SPR neighbours
of a tree given as an edge list, and the search on them.

The reference has no parsimony; the rule is DESIGN 4.22's: state sets are the states a tip's code
allows, ``c(A, B)`` is the intersection where it is non-empty and the union otherwise, and a
change is counted where it is empty.  Every result is an integer (unsigned 64-bit sums) and does
not depend on the launch shape or on ``PU_PARS_CHUNK``.

An alignment is given coded, as ``TreeModel._coded_alignment()`` returns it: ``(codes
[n_taxa][n_pat] uint8, table [n_codes][K], names in row order)``.  A tree is a ``tree.Tree``, a
Newick string -- leaves are mapped to rows by name, as ``set_tree`` does -- or a schedule ``(ops
int32 [n-2][3], root_edge [2])`` on the library's node ids: a tip is its alignment row, the
internal nodes are ``n .. 2n-3``.  The ``2n - 3`` edges of a schedule are, in *op order*,
``2i = (left_i, parent_i)``, ``2i + 1 = (right_i, parent_i)`` and, last, the root edge.

There is no host fallback: every count comes from the HIP kernels of ``pu_parsimony.hip``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .tree import BranchLengths, Node, Traversal, Tree, prepare_tree, with_lengths

MAX_STATES = 32


def state_masks(table):
    """The state sets of a code table [n_codes][K] as bit masks: bit k of mask c is set where
    ``table[c][k] > 0``; uint8 for K <= 8, else uint32.  A code that allows no state, or more
    than 32 states, is refused."""
    table = np.asarray(table, dtype=np.float64)
    if table.ndim != 2 or table.shape[1] < 1:
        raise ValueError("table must be [n_codes][K], not %r" % (table.shape,))
    K = table.shape[1]
    if K > MAX_STATES:
        raise ValueError("parsimony takes at most %d states, not %d" % (MAX_STATES, K))
    bits = (table > 0).astype(np.uint64) << np.arange(K, dtype=np.uint64)
    masks = bits.sum(axis=1)
    if (masks == 0).any():
        raise ValueError("code %d allows no state (an all-zero table row)"
                         % int(np.flatnonzero(masks == 0)[0]))
    return masks.astype(np.uint8 if K <= 8 else np.uint32)


def integer_weights(weights, n_pat):
    """`weights` as int64 [n_pat], or None as it is; non-integral weights are refused (the
    sign is the library's to refuse)."""
    if weights is None:
        return None
    w = np.asarray(weights)
    if w.shape != (n_pat,):
        raise ValueError("weights must be [%d], not %r" % (n_pat, w.shape))
    if w.dtype.kind not in "iu":
        wf = np.asarray(w, dtype=np.float64)
        if not np.all(np.isfinite(wf)) or np.any(wf != np.rint(wf)) or np.any(np.abs(wf) >= 2.0 ** 62):
            raise ValueError("parsimony needs integral weights")
        w = wf
    return np.ascontiguousarray(w, dtype=np.int64)


def _alignment(coded_alignment):
    codes, table, names = coded_alignment
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.float64)
    if codes.ndim != 2 or table.ndim != 2:
        raise ValueError("codes must be [n_taxa][n_pat] and table [n_codes][K]")
    names = list(names)
    if len(names) != codes.shape[0]:
        raise ValueError("%d names for %d rows" % (len(names), codes.shape[0]))
    return codes, table, names


def tree_schedule(tree, names):
    """(ops int32 [n-2][3], root_edge int32 [2], pairs) of `tree` on the alignment whose rows are
    `names`: the post-order of ``prepare_tree(tree)`` with every leaf renamed to its row and the
    internal node of op i to n + i; `pairs` lists, in op order, each edge as its pair of
    ``Traversal`` node indices (child end first)."""
    return _prepared_schedule(prepare_tree(tree), names)


def _prepared_schedule(t, names):
    """tree_schedule of a tree that is prepared already (prepare_tree is not idempotent where the
    seed's second child is a leaf)."""
    tr = Traversal(t)
    names = list(names)
    n = len(names)
    row = {name: i for i, name in enumerate(names)}
    if sorted(tr.names) != sorted(row) or len(row) != n:
        raise ValueError("the tree's leaves are not the alignment's %d names" % n)
    ids = {idx: row[name] for name, idx in tr.names.items()}
    for i, op in enumerate(tr.postorder_traversal):
        ids[int(op[0])] = n + i
    ops = np.array([[ids[int(v)] for v in op] for op in tr.postorder_traversal],
                   dtype=np.int32).reshape(-1, 3)
    root = np.array([ids[int(v)] for v in tr.root_edge], dtype=np.int32)
    pairs = []
    for p, a, b in tr.postorder_traversal:
        pairs += [(int(a), int(p)), (int(b), int(p))]
    pairs.append((int(tr.root_edge[0]), int(tr.root_edge[1])))
    return ops, root, pairs


def _schedule(tree, names):
    if isinstance(tree, (tuple, list)) and len(tree) == 2 and not isinstance(tree[0], str):
        ops = np.ascontiguousarray(tree[0], dtype=np.int32).reshape(-1, 3)
        root = np.ascontiguousarray(tree[1], dtype=np.int32).reshape(-1)
        if len(ops) != len(names) - 2 or len(root) != 2:
            raise ValueError("a schedule of %d taxa has %d ops and a root edge of 2 nodes"
                             % (len(names), len(names) - 2))
        return ops, root
    return tree_schedule(tree, names)[:2]


def _is_one_tree(trees):
    if isinstance(trees, (str, Tree)):
        return True
    return isinstance(trees, tuple) and len(trees) == 2 and not isinstance(trees[0], (str, Tree)) \
        and np.asarray(trees[0]).ndim == 2


def fitch_lengths(coded_alignment, trees, weights=None, per_pattern=False, per_edge=False,
                  device=0):
    """pu_fitch_lengths: the parsimony length of every tree of `trees` (one tree, or a list) on
    the alignment, uint64 [n_trees] (a Python int for one tree).  With `per_pattern` also the
    unweighted changes of every pattern, uint32 [n_trees][n_pat]; with `per_edge` also the
    weighted change count of every edge in op order, uint64 [n_trees][2n-3]: returned as a tuple
    (lengths, per-pattern, per-edge) without the ones not asked for."""
    codes, table, names = _alignment(coded_alignment)
    single = _is_one_tree(trees)
    scheds = [_schedule(t, names) for t in ([trees] if single else list(trees))]
    if not scheds:
        raise ValueError("no tree")
    n, n_pat = codes.shape
    w = integer_weights(weights, n_pat)
    ops = np.ascontiguousarray(np.stack([s[0] for s in scheds]), dtype=np.int32)
    roots = np.ascontiguousarray(np.stack([s[1] for s in scheds]), dtype=np.int32)
    T = len(scheds)
    lengths = np.zeros(T, dtype=np.uint64)
    pp = np.zeros((T, n_pat), dtype=np.uint32) if per_pattern else None
    pe = np.zeros((T, max(2 * n - 3, 0)), dtype=np.uint64) if per_edge else None
    N.check(N.lib().pu_fitch_lengths(int(device), n, n_pat, table.shape[0], table.shape[1],
                                     N.ptr(codes), N.ptr(table), N.ptr(w), T, N.ptr(ops),
                                     N.ptr(roots), N.ptr(lengths), N.ptr(pp), N.ptr(pe)), None,
            "pu_fitch_lengths")
    out = [int(lengths[0]) if single else lengths]
    if per_pattern:
        out.append(pp[0] if single else pp)
    if per_edge:
        out.append(pe[0] if single else pe)
    return out[0] if len(out) == 1 else tuple(out)


def insertion_lengths(coded_alignment, tree, query_codes, weights=None, device=0):
    """pu_fitch_insert_lengths: uint64 [n_query][2n-3], the exact length of `tree` with query
    row q (`query_codes` [n_query][n_pat], coded with the alignment's table) attached on edge e,
    edges in op order (``tree_schedule``)."""
    codes, table, names = _alignment(coded_alignment)
    ops, root = _schedule(tree, names)
    n, n_pat = codes.shape
    q = np.ascontiguousarray(query_codes, dtype=np.uint8)
    if q.ndim != 2 or q.shape[1] != n_pat:
        raise ValueError("query_codes must be [n_query][%d], not %r" % (n_pat, q.shape))
    w = integer_weights(weights, n_pat)
    out = np.zeros((q.shape[0], max(2 * n - 3, 0)), dtype=np.uint64)
    N.check(N.lib().pu_fitch_insert_lengths(int(device), n, n_pat, table.shape[0], table.shape[1],
                                            N.ptr(codes), N.ptr(table), N.ptr(w), N.ptr(ops),
                                            N.ptr(root), q.shape[0], N.ptr(q), N.ptr(out)), None,
            "pu_fitch_insert_lengths")
    return out


def random_orders(n_taxa, n_rep, seed):
    """int32 [n_rep][n_taxa]: replicate r is the r-th ``permutation(n_taxa)`` drawn from
    ``numpy.random.default_rng(seed)``, on the host."""
    rng = np.random.default_rng(seed)
    return np.array([rng.permutation(int(n_taxa)) for _ in range(int(n_rep))],
                    dtype=np.int32).reshape(int(n_rep), int(n_taxa))


def stepwise_addition(coded_alignment, orders=None, n_rep=1, seed=0, weights=None, device=0):
    """pu_parsimony_stepwise: one stepwise-addition tree per addition order (`orders` int32
    [n_rep][n_taxa], default ``random_orders(n_taxa, n_rep, seed)``): (edges int32
    [n_rep][2n-3][2] in DESIGN 4.22's numbering, step_lengths uint64 [n_rep][n-2] -- the tree
    length after each step, entry 0 the three-taxon star --, lengths uint64 [n_rep])."""
    codes, table, names = _alignment(coded_alignment)
    n, n_pat = codes.shape
    if orders is None:
        orders = random_orders(n, n_rep, seed)
    orders = np.ascontiguousarray(orders, dtype=np.int32)
    if orders.ndim == 1:
        orders = orders[None]
    if orders.ndim != 2 or orders.shape[1] != n:
        raise ValueError("orders must be [n_rep][%d], not %r" % (n, orders.shape))
    R = orders.shape[0]
    w = integer_weights(weights, n_pat)
    edges = np.zeros((R, max(2 * n - 3, 0), 2), dtype=np.int32)
    steps = np.zeros((R, max(n - 2, 0)), dtype=np.uint64)
    lengths = np.zeros(R, dtype=np.uint64)
    N.check(N.lib().pu_parsimony_stepwise(int(device), n, n_pat, table.shape[0], table.shape[1],
                                          N.ptr(codes), N.ptr(table), N.ptr(w), R,
                                          N.ptr(orders), N.ptr(edges), N.ptr(steps),
                                          N.ptr(lengths)), None, "pu_parsimony_stepwise")
    return edges, steps, lengths


SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)  # a score entry that is no (valid direction, target) pair


def _edge_batch(edges, n):
    """(int32 [T][2n-3][2], whether `edges` was one edge list)."""
    e = np.ascontiguousarray(edges, dtype=np.int32)
    single = e.ndim == 2
    if single:
        e = e[None]
    if e.ndim != 3 or e.shape[1:] != (max(2 * n - 3, 0), 2) or e.shape[0] < 1:
        raise ValueError("edges must be [2n-3][2] or [T][2n-3][2] with n = %d, not %r"
                         % (n, np.shape(edges)))
    return np.ascontiguousarray(e), single


def spr_scores(coded_alignment, edges, weights=None, radius=None, device=0):
    """pu_fitch_spr_scores: the exact parsimony length of every SPR neighbour of
    the tree `edges` (int32 [2n-3][2] in DESIGN 4.22's form, or a batch [T][2n-3][2]).  Returns
    (length, scores): L(T) (a Python int, or uint64 [T]) and uint64 [2(2n-3)][2n-3] (or
    [T][...]), ``scores[d][f]`` the length after pruning direction ``d = 2e + side`` and
    regrafting on edge f, ``SENTINEL`` where that is no move.  `radius` None or 0: no limit."""
    codes, table, names = _alignment(coded_alignment)
    n, n_pat = codes.shape
    e, single = _edge_batch(edges, n)
    w = integer_weights(weights, n_pat)
    T, E = e.shape[0], e.shape[1]
    lengths = np.zeros(T, dtype=np.uint64)
    scores = np.zeros((T, 2 * E, E), dtype=np.uint64)
    N.check(N.lib().pu_fitch_spr_scores(int(device), n, n_pat, table.shape[0], table.shape[1],
                                        N.ptr(codes), N.ptr(table), N.ptr(w), T, N.ptr(e),
                                        int(radius or 0), N.ptr(lengths), N.ptr(scores)), None,
            "pu_fitch_spr_scores")
    return (int(lengths[0]), scores[0]) if single else (lengths, scores)


def spr_search(coded_alignment, edges, weights=None, radius=None, max_rounds=0,
               return_moves=False, device=0):
    """pu_parsimony_spr: per tree of `edges` (one edge list or a batch), rounds of
    "score all SPR neighbours, take the shortest (ties: the lowest direction, then the lowest
    edge) if it is shorter than the tree" until none is, or `max_rounds` rounds (0: no limit).
    Returns (edges, length, rounds) -- for a batch int32 [T][2n-3][2], uint64 [T], int32 [T] --
    and with `return_moves` (needs ``max_rounds > 0``) also the moves, uint64 [rounds][3] =
    (d, f, length after) per tree."""
    codes, table, names = _alignment(coded_alignment)
    n, n_pat = codes.shape
    e, single = _edge_batch(edges, n)
    e = e.copy()
    w = integer_weights(weights, n_pat)
    max_rounds = int(max_rounds)
    if return_moves and max_rounds <= 0:
        raise ValueError("return_moves needs max_rounds > 0")
    T = e.shape[0]
    lengths = np.zeros(T, dtype=np.uint64)
    rounds = np.zeros(T, dtype=np.int32)
    moves = np.zeros((T, max_rounds, 3), dtype=np.uint64) if return_moves else None
    N.check(N.lib().pu_parsimony_spr(int(device), n, n_pat, table.shape[0], table.shape[1],
                                     N.ptr(codes), N.ptr(table), N.ptr(w), T, N.ptr(e),
                                     int(radius or 0), max_rounds, N.ptr(lengths), N.ptr(rounds),
                                     N.ptr(moves)), None, "pu_parsimony_spr")
    out = [e[0], int(lengths[0]), int(rounds[0])] if single else [e, lengths, rounds]
    if return_moves:
        per_tree = [moves[t, :int(rounds[t])] for t in range(T)]
        out.append(per_tree[0] if single else per_tree)
    return tuple(out)


def apply_spr_edges(edges, d, f):
    """The edge list after the SPR move (d, f) of DESIGN 4.26, on the host: with ``(s, u)`` the
    ends of edge ``d // 2`` (reversed for an odd d), ``ea < eb`` u's other two edges and a, b
    their far ends, and ``(x, y) = edges[f]``: ``edges[ea] = (a, b)``, ``edges[f] = (x, u)``,
    ``edges[eb] = (u, y)``.  A direction whose u is a tip, and an f that is no target's id
    (edge d // 2, ea, eb, or an edge of the pruned subtree -- the last is not checked), are
    refused."""
    out = np.array(edges, dtype=np.int32).reshape(-1, 2)
    n = (len(out) + 3) // 2
    d, f = int(d), int(f)
    e, side = d >> 1, d & 1
    if not (0 <= e < len(out) and 0 <= f < len(out)):
        raise ValueError("move (%d, %d) of %d edges" % (d, f, len(out)))
    u = int(out[e, 1 - side])
    if u < n:
        raise ValueError("direction %d prunes towards tip %d" % (d, u))
    (ea, a), (eb, b) = sorted((g, int(out[g, 0] if out[g, 1] == u else out[g, 1]))
                              for g in np.flatnonzero((out == u).any(axis=1)) if g != e)
    if f in (e, ea, eb):
        raise ValueError("edge %d is no target of direction %d" % (f, d))
    x, y = out[f]
    out[ea] = (a, b)
    out[f] = (x, u)
    out[eb] = (u, y)
    return out


def edges_to_tree(edges, names, lengths=None):
    """The ``tree.Tree`` of an edge list [2n-3][2] over tips 0..n-1 (labelled names[i]) and
    internal nodes n..2n-3: derooted at node n, whose three neighbours are the seed's children
    in edge order.  `lengths` [2n-3], when given, are the edges' lengths by edge id."""
    names = list(names)
    n = len(names)
    edges = np.asarray(edges).reshape(-1, 2)
    if n < 3 or len(edges) != 2 * n - 3:
        raise ValueError("%d names need %d edges, not %d" % (n, 2 * n - 3, len(edges)))
    adj = {v: [] for v in range(2 * n - 2)}
    for e, (a, b) in enumerate(edges):
        a, b = int(a), int(b)
        if a not in adj or b not in adj or a == b:
            raise ValueError("edge %d = (%d, %d) of %d nodes" % (e, a, b, 2 * n - 2))
        adj[a].append((b, e))
        adj[b].append((a, e))
    if any(len(adj[v]) != (1 if v < n else 3) for v in adj):
        raise ValueError("the edges are no binary tree over %d tips" % n)
    seed = Node()
    stack = [(n, -1, seed)]
    seen = 0
    while stack:
        v, came, node = stack.pop()
        seen += 1
        if seen > 2 * n - 2:  # a cycle: the walk would not end
            break
        for u, e in adj[v]:
            if u != came:
                child = node.add(Node(str(names[u]) if u < n else None,
                                      None if lengths is None else float(lengths[e])))
                stack.append((u, v, child))
    if seen != 2 * n - 2:
        raise ValueError("the edges are not connected")
    return Tree(seed)


def edge_lengths_tree(tree, names, per_edge, total, min_length=1e-8):
    """``prepare_tree(tree)`` with every branch length set to ``max(changes / total,
    min_length)``: `per_edge` are the edge change counts of ``fitch_lengths(per_edge=True)`` on
    that tree, in op order, `total` the sum of the weights."""
    t = prepare_tree(tree)
    pairs = _prepared_schedule(t, names)[2]
    bl = BranchLengths()
    for pair, c in zip(pairs, per_edge):
        bl[tuple(sorted(pair))] = max(float(int(c)) / float(total), float(min_length))
    return with_lengths(t, bl)


def profile(on, device=0):
    """Switch the event timing of the parsimony calls on `device` on or off."""
    N.check(N.lib().pu_parsimony_profile(int(device), int(bool(on))), None, "pu_parsimony_profile")


def kernel_ms(device=0):
    """The kernel time of the last parsimony call on `device` while profiling, in ms, summed
    over its chunks and steps."""
    ms = ctypes.c_double()
    N.check(N.lib().pu_parsimony_kernel_ms(int(device), ctypes.byref(ms)), None,
            "pu_parsimony_kernel_ms")
    return ms.value
