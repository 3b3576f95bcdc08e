"""DESIGN 4.26 (parsimony SPR) restated in numpy on top of tests/parsimony_reference.py: prune
directions, targets with their distance, the move on an edge list, and the search.  The score
of a move is brute force -- apply the move, then ``parsimony_reference.lengths`` on the new edge
list from scratch -- so the yardstick never uses the directional-set shortcut; ``formula_scores``
is the rule's shortcut, kept apart and checked against the brute force in test_parsimony_spr.py.
"""
import numpy as np

import parsimony_reference as PR

SENTINEL = 2 ** 64 - 1


def n_taxa_of(edges):
    return (len(edges) + 3) // 2


def _incident(edges):
    """{node: [(neighbour, edge id)] in edge order}."""
    adj = {}
    for g, (u, v) in enumerate(edges):
        adj.setdefault(int(u), []).append((int(v), g))
        adj.setdefault(int(v), []).append((int(u), g))
    return adj


def direction(edges, d):
    """dict(e, s, u, ea, a, eb, b) of direction d, or None where u is a tip."""
    n = n_taxa_of(edges)
    e, side = d // 2, d % 2
    s, u = (int(v) for v in edges[e])
    if side:
        s, u = u, s
    if u < n:
        return None
    (ea, a), (eb, b) = sorted((g, x) for x, g in _incident(edges)[u] if g != e)
    return dict(e=e, s=s, u=u, ea=ea, a=a, eb=eb, b=b)


def valid_directions(edges):
    return [d for d in range(2 * len(edges)) if direction(edges, d) is not None]


def rest_tree(edges, d):
    """T' of direction d as {edge id: (x, y)}: T without s's side, u dissolved, the merged edge
    (a, b) under id ea."""
    m = direction(edges, d)
    adj = _incident(edges)
    gone, todo = {m["e"], m["eb"]}, [(m["s"], m["u"])]
    while todo:  # the edges on s's side
        v, came = todo.pop()
        for x, g in adj[v]:
            if x != came:
                gone.add(g)
                todo.append((x, v))
    rest = {g: (int(x), int(y)) for g, (x, y) in enumerate(edges) if g not in gone}
    rest[m["ea"]] = (m["a"], m["b"])
    return rest


def targets(edges, d, radius=0):
    """{f: dist(f)} of direction d: the edges of T' other than the merged one, breadth first
    from the merged edge; `radius` 0 is no limit."""
    m = direction(edges, d)
    if m is None:
        return {}
    rest = rest_tree(edges, d)
    at = {}
    for g, (x, y) in rest.items():
        at.setdefault(x, []).append(g)
        at.setdefault(y, []).append(g)
    dist = {m["ea"]: 0}
    front = [m["ea"]]
    while front:
        nxt = []
        for g in front:
            for v in rest[g]:
                for h in at[v]:
                    if h not in dist:
                        dist[h] = dist[g] + 1
                        nxt.append(h)
        front = nxt
    del dist[m["ea"]]
    return {f: k for f, k in dist.items() if radius == 0 or k <= radius}


def apply_spr_edges(edges, d, f):
    m = direction(edges, d)
    out = [tuple(int(v) for v in ed) for ed in edges]
    x, y = out[f]
    out[m["ea"]] = (m["a"], m["b"])
    out[f] = (x, m["u"])
    out[m["eb"]] = (m["u"], y)
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def brute_scores(edges, S, w=None, radius=0):
    """(L(T), {(d, f): length of the tree after the move, scored from scratch})."""
    out = {}
    for d in valid_directions(edges):
        for f in targets(edges, d, radius):
            out[(d, f)] = PR.lengths(apply_spr_edges(edges, d, f), S, w)
    return PR.lengths(edges, S, w), out


def formula_scores(edges, S, w=None, radius=0):
    """The same by the rule: score = L - miss(ea) + miss(f), the edge sets of T' from the
    directional sets of T by the walk outward from the merged edge."""
    D = PR.directional_sets(edges, S)
    adj = _incident(edges)
    L = PR.lengths(edges, S, w)
    out = {}
    for d in valid_directions(edges):
        m = direction(edges, d)
        s, u, a, b = m["s"], m["u"], m["a"], m["b"]
        Ds = D[(s, u)]
        miss = lambda Eg: PR._wsum(w, (Ds & Eg) == 0)  # noqa: E731
        base = L - miss(PR.combine(D[(a, u)], D[(b, u)]))
        # (node entered, where from in T, the set arriving, dist of its further edges)
        todo = [(a, u, D[(b, u)], 1), (b, u, D[(a, u)], 1)]
        while todo:
            v, came, X, k = todo.pop()
            kids = [(x, g) for x, g in adj[v] if x != came]
            if not kids or (radius and k > radius):
                continue
            (c1, g1), (c2, g2) = kids
            for (c, g), (o, _) in (((c1, g1), (c2, g2)), ((c2, g2), (c1, g1))):
                Y = PR.combine(D[(o, v)], X)
                out[(d, g)] = base + miss(PR.combine(D[(c, v)], Y))
                todo.append((c, v, Y, k + 1))
    return L, out


def score_matrix(edges, scores):
    """uint64-valued object array [2E][E] of a {(d, f): score} dict, SENTINEL elsewhere."""
    E = len(edges)
    out = np.full((2 * E, E), SENTINEL, dtype=object)
    for (d, f), v in scores.items():
        out[d, f] = v
    return out


def search(edges, S, w=None, radius=0, max_rounds=0, scores=brute_scores):
    """dict(edges, length, rounds, moves [(d, f, length after)])."""
    edges = np.array(edges, dtype=np.int32).reshape(-1, 2)
    moves = []
    L = PR.lengths(edges, S, w)
    while True:
        _, sc = scores(edges, S, w, radius)
        if not sc:
            break
        best, d, f = min((v, d, f) for (d, f), v in sc.items())
        if best >= L:
            break
        edges = apply_spr_edges(edges, d, f)
        L = best
        moves.append((d, f, best))
        if max_rounds and len(moves) == max_rounds:
            break
    return dict(edges=edges, length=L, rounds=len(moves), moves=moves)


def splits(edges):
    """The non-trivial bipartitions of an edge list, each as the frozenset of tips on the side
    without tip 0."""
    n = n_taxa_of(edges)
    adj = _incident(edges)
    out = set()

    def tips(v, came):
        if v < n:
            return {v}
        return set().union(*[tips(x, v) for x, _ in adj[v] if x != came])

    for u, v in edges:
        side = tips(int(u), int(v))
        if 1 < len(side) < n - 1:
            out.add(frozenset(side if 0 not in side else set(range(n)) - side))
    return frozenset(out)


def nni_neighbours(edges):
    """The topologies (split sets) of the 2 (n - 3) NNI neighbours: across every internal edge
    (p, q), swap one neighbour of p with each of the two of q."""
    n = n_taxa_of(edges)
    base = [tuple(int(v) for v in ed) for ed in edges]
    adj = _incident(edges)
    out = []
    for g, (p, q) in enumerate(base):
        if p < n or q < n:
            continue
        (x, gx) = [(x, h) for x, h in adj[p] if h != g][0]
        for y, gy in [(y, h) for y, h in adj[q] if h != g]:
            new = list(base)
            new[gx] = tuple(q if v == p else v for v in base[gx])
            new[gy] = tuple(p if v == q else v for v in base[gy])
            out.append(splits(new))
    return out
