"""DESIGN 4.31 in plain Python ints and floats, to the letter, and beside it an independent second
statement that only checks the first (``check_*``: breadth-first searches over the adjacency
lists, splits as frozensets found by cutting every edge, sums by ``math.fsum``).

The rule.  Trees, forms and edge orders are DESIGN 4.27's (tests/treeset_reference.py).  Every tree
has ``lengths [2n-3]`` in its form's edge order, finite and >= 0.  A tree's lengths are indexed by
key: pendant key i is the edge at tip i, split key u the edge whose non-trivial split has id u; a
key the tree does not hold has length 0.

* ``wRF(a, b) = sum |l_a - l_b|`` and ``KF2(a, b) = sum (l_a - l_b)^2`` over the keys: the pendant
  keys 0..n-1 ascending, then the split keys of a or b in ascending id; one serial sum from 0.0,
  the square rounded on its own before it is added.
* ``Path2(a, b) = sum_{i<j} (e_a(i,j) - e_b(i,j))^2``, ``e`` the number of edges between two tips;
  integers.
* ``WPath2``: the same with ``p(i,j)``.  Root the tree at tip 0; ``l`` is the node of the path
  i..j nearest tip 0; ``h(i->l)`` adds the edge lengths from tip i up to ``l`` serially, starting
  with i's pendant edge; ``p = h(i->l) + h(j->l)``.  The rounded squares of ``p_a - p_b`` are
  summed over the pairs in order (i, then j) in segments of 2048 consecutive pairs, each added
  serially from 0.0, the segment sums then added serially in segment order.
* ``split_sum[u]``: the lengths of the edges that carry split u added serially over the trees in
  ascending tree index; ``tip_sum[i]`` likewise over tip i's pendant edges.
"""
import math
from collections import deque

import treeset_reference as TR

SEGMENT = 2048


# ---- the first statement: the rule to the letter --------------------------------------------

def keyed(form, tree, lengths):
    """(pend [n], {split int: length}) of one tree."""
    edges = TR.form_edges(form, tree)
    n = (len(edges) + 3) // 2
    splits = TR.edge_splits(form, tree)
    pend, by_split = [None] * n, {}
    for (a, b), s, x in zip(edges, splits, lengths):
        if s is None:
            pend[a if a < n else b] = float(x)
        else:
            by_split[s] = float(x)
    assert None not in pend and len(by_split) == n - 3
    return pend, by_split


def rooted_at_tip0(form, tree, lengths):
    """(parent, depth, length of the edge to the parent) per node of the tree rooted at tip 0."""
    edges = TR.form_edges(form, tree)
    adj = {}
    for (a, b), x in zip(edges, lengths):
        adj.setdefault(a, []).append((b, float(x)))
        adj.setdefault(b, []).append((a, float(x)))
    par, dep, up = {0: None}, {0: 0}, {0: 0.0}
    todo = [0]
    while todo:
        v = todo.pop()
        for x, ln in adj[v]:
            if x not in dep:
                par[x], dep[x], up[x] = v, dep[v] + 1, ln
                todo.append(x)
    return par, dep, up


def paths(form, tree, lengths):
    """(e [n(n-1)/2] ints, p [n(n-1)/2] floats) in pair order (i ascending, then j)."""
    n = (len(TR.form_edges(form, tree)) + 3) // 2
    par, dep, up = rooted_at_tip0(form, tree, lengths)
    e, p = [], []
    for i in range(n):
        for j in range(i + 1, n):
            a, b, hi, hj, k = i, j, 0.0, 0.0, 0
            while a != b:
                da, db = dep[a], dep[b]
                if da >= db:
                    hi, a, k = hi + up[a], par[a], k + 1
                if db >= da:
                    hj, b, k = hj + up[b], par[b], k + 1
            e.append(k)
            p.append(hi + hj)
    return e, p


def weighted_pair(ka, kb, index):
    """(wRF, KF2) of two keyed trees; `index`: split int -> id."""
    w = q = 0.0
    for la, lb in zip(ka[0], kb[0]):
        d = la - lb
        w += abs(d)
        sq = d * d
        q += sq
    for s in sorted(set(ka[1]) | set(kb[1]), key=index.__getitem__):
        d = ka[1].get(s, 0.0) - kb[1].get(s, 0.0)
        w += abs(d)
        sq = d * d
        q += sq
    return w, q


def path2_pair(ea, eb):
    return sum((x - y) * (x - y) for x, y in zip(ea, eb))


def wpath2_pair(pa, pb):
    total = 0.0
    for g in range(0, len(pa), SEGMENT):
        seg = 0.0
        for x, y in zip(pa[g:g + SEGMENT], pb[g:g + SEGMENT]):
            d = x - y
            sq = d * d
            seg += sq
        total += seg
    return total


def distances(form, trees, lengths, rows=None, want=("wrf", "kf2", "path2", "wpath2")):
    """dict(n, U, wrf, kf2, path2, wpath2: [rows][T] lists; split_sum [U], tip_sum [n]) of a
    tree set with lengths [T][2n-3]."""
    T = len(trees)
    rows = T if rows is None else rows
    keys = [keyed(form, t, x) for t, x in zip(trees, lengths)]
    n = len(keys[0][0])
    U = sorted(set(s for k in keys for s in k[1]))
    index = {s: i for i, s in enumerate(U)}
    out = dict(n=n, U=U)
    if "wrf" in want or "kf2" in want:
        both = [[weighted_pair(keys[a], keys[b], index) for b in range(T)] for a in range(rows)]
        out["wrf"] = [[x[0] for x in r] for r in both]
        out["kf2"] = [[x[1] for x in r] for r in both]
    if "path2" in want or "wpath2" in want:
        ep = [paths(form, t, x) for t, x in zip(trees, lengths)]
        if "path2" in want:
            out["path2"] = [[path2_pair(ep[a][0], ep[b][0]) for b in range(T)] for a in range(rows)]
        if "wpath2" in want:
            out["wpath2"] = [[wpath2_pair(ep[a][1], ep[b][1]) for b in range(T)] for a in range(rows)]
    split_sum = [0.0] * len(U)
    tip_sum = [0.0] * n
    for pend, by_split in keys:
        for i in range(n):
            tip_sum[i] += pend[i]
        for s, x in by_split.items():
            split_sum[index[s]] += x
    out["split_sum"], out["tip_sum"] = split_sum, tip_sum
    out["count"] = [sum(1 for k in keys if s in k[1]) for s in U]
    return out


# ---- the second statement: used only to check the first --------------------------------------

def _adjacency(form, tree, lengths):
    adj = {}
    for (a, b), x in zip(TR.form_edges(form, tree), lengths):
        adj.setdefault(a, []).append((b, float(x)))
        adj.setdefault(b, []).append((a, float(x)))
    return adj


def check_paths(form, tree, lengths):
    """(e, p, hops): per pair in order the edge count by breadth-first search, the fsum of the
    lengths along the path, and the count again for the error bound."""
    adj = _adjacency(form, tree, lengths)
    n = (len(adj) + 2) // 2
    e, p = [], []
    for i in range(n):
        seen = {i: (0, ())}
        todo = deque([i])
        while todo:
            v = todo.popleft()
            for x, ln in adj[v]:
                if x not in seen:
                    seen[x] = (seen[v][0] + 1, seen[v][1] + (ln,))
                    todo.append(x)
        for j in range(i + 1, n):
            e.append(seen[j][0])
            p.append(math.fsum(seen[j][1]))
    return e, p


def check_keyed(form, tree, lengths):
    """{frozenset of the tips on the side without tip 0: length} of every edge, by cutting it."""
    edges = TR.form_edges(form, tree)
    adj = _adjacency(form, tree, lengths)
    n = (len(edges) + 3) // 2
    out = {}
    for (a, b), x in zip(edges, lengths):
        side, todo = {a}, [a]  # what a reaches without crossing (a, b)
        while todo:
            v = todo.pop()
            for y, _ in adj[v]:
                if y not in side and not (v == a and y == b):
                    side.add(y)
                    todo.append(y)
        tips = frozenset(v for v in side if v < n)
        if 0 in tips:
            tips = frozenset(range(n)) - tips
        out[tips] = float(x)
    assert len(out) == len(edges)
    return out


def check_weighted(da, db):
    """(wRF, KF2) of two ``check_keyed`` dicts by fsum."""
    keys = set(da) | set(db)
    diffs = [da.get(k, 0.0) - db.get(k, 0.0) for k in keys]
    return math.fsum(abs(d) for d in diffs), math.fsum(d * d for d in diffs)
