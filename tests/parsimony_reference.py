"""DESIGN 4.22 (Fitch parsimony) restated in numpy, with plain integer masks and no device, and
Sankoff's dynamic programme as an independent algorithm that never forms a Fitch set.

A tree is an edge list [(u, v)] of an unrooted binary tree: tips are alignment rows (< n), every
other node is internal.  State sets are uint64 masks [P] per tip.  All sums are Python integers.
"""
import sys

import numpy as np

sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))


def masks_of(table):
    """Bit k of mask c is set where table[c][k] > 0 (uint64; an empty set is refused)."""
    out = []
    for row in np.asarray(table):
        m = 0
        for k, v in enumerate(row):
            if v > 0:
                m |= 1 << k
        if m == 0:
            raise ValueError("a code that allows no state")
        out.append(m)
    return np.array(out, dtype=np.uint64)


def tip_sets(codes, table):
    """[n][P] uint64 state sets of coded rows."""
    return masks_of(table)[np.asarray(codes)]


def combine(A, B):
    I = A & B
    return np.where(I != 0, I, A | B)


def _wsum(w, flags):
    """sum of w[p] over the patterns where flags[p] (times flags[p] for counts), exactly."""
    f = np.asarray(flags).astype(object)
    if w is None:
        return int(f.sum()) if len(f) else 0
    return int((np.asarray(w).astype(object) * f).sum()) if len(f) else 0


def _adjacency(edges):
    adj = {}
    for u, v in edges:
        adj.setdefault(int(u), []).append(int(v))
        adj.setdefault(int(v), []).append(int(u))
    return adj


class _Directional(object):
    """D(u -> v) and the changes inside u's side, by the rule: a tip's set is its own, an
    internal node's is the combination of the sets arriving from its two other neighbours."""

    def __init__(self, edges, S):
        self.adj = _adjacency(edges)
        self.S = S
        self.memo = {}

    def get(self, u, v):
        key = (u, v)
        if key not in self.memo:
            others = [x for x in self.adj[u] if x != v]
            if not others:
                P = self.S.shape[1]
                self.memo[key] = (self.S[u], np.zeros(P, dtype=np.int64))
            else:
                x, y = others
                (A, ca), (B, cb) = self.get(x, u), self.get(y, u)
                self.memo[key] = (combine(A, B), ca + cb + ((A & B) == 0))
        return self.memo[key]


def pattern_changes(edges, S, root_edge=0):
    """Changes per pattern in a post-order over the tree rooted on edge `root_edge`."""
    D = _Directional(edges, S)
    a, b = (int(x) for x in edges[root_edge])
    (A, ca), (B, cb) = D.get(a, b), D.get(b, a)
    return ca + cb + ((A & B) == 0)


def lengths(edges, S, w=None, root_edge=0):
    return _wsum(w, pattern_changes(edges, S, root_edge))


def directional_sets(edges, S):
    """{(u, v): D(u -> v)} for both directions of every edge."""
    D = _Directional(edges, S)
    out = {}
    for u, v in edges:
        u, v = int(u), int(v)
        out[(u, v)] = D.get(u, v)[0]
        out[(v, u)] = D.get(v, u)[0]
    return out


def edge_sets(edges, S):
    """[E][P]: E(e) = c(D(u -> v), D(v -> u))."""
    D = directional_sets(edges, S)
    return np.array([combine(D[(int(u), int(v))], D[(int(v), int(u))]) for u, v in edges],
                    dtype=np.uint64).reshape(len(edges), -1)


def edge_changes(edges, S, w=None):
    """Per edge: sum of w over the patterns whose two directional sets are disjoint."""
    D = directional_sets(edges, S)
    return [_wsum(w, (D[(int(u), int(v))] & D[(int(v), int(u))]) == 0) for u, v in edges]


def insertion_lengths(edges, S, Q, w=None):
    """[Q][E] Python ints: L(T) + sum of w over the patterns where the query's set misses E(e)."""
    L = lengths(edges, S, w)
    E = edge_sets(edges, S)
    return [[L + _wsum(w, (q & E[e]) == 0) for e in range(len(edges))] for q in Q]


def attach(edges, e, x, m):
    """The edge list with tip x attached on edge e through new node m, numbered as a step of
    stepwise addition numbers it: e = (a, b) becomes (a, m); (m, b) and (x, m) are appended."""
    out = [tuple(int(v) for v in ed) for ed in edges]
    a, b = out[e]
    out[e] = (a, m)
    out.append((m, b))
    out.append((int(x), m))
    return out


def stepwise(S, order, w=None):
    """Stepwise addition of rows `order` (a permutation): dict(edges [2n-3][2], step_lengths
    [n-2], length, tied [n-3] -- edges tied for the minimum at each step --, chosen [n-3])."""
    n = len(order)
    order = [int(v) for v in order]
    edges = [(order[0], n), (order[1], n), (order[2], n)]
    steps = [lengths(edges, S, w)]
    tied, chosen = [], []
    for k in range(3, n):
        L = steps[-1]
        E = edge_sets(edges, S)
        cand = [L + _wsum(w, (S[order[k]] & E[e]) == 0) for e in range(len(edges))]
        best = min(cand)
        e = cand.index(best)  # the lowest edge id among the ties
        tied.append(cand.count(best))
        chosen.append(e)
        edges = attach(edges, e, order[k], n + k - 2)
        steps.append(best)
    return dict(edges=np.array(edges, dtype=np.int32).reshape(-1, 2), step_lengths=steps,
                length=lengths(edges, S, w), tied=tied, chosen=chosen)


# ---- Sankoff -----------------------------------------------------------------------------

def sankoff_length(edges, allowed, w=None, root_edge=0):
    """Unit-cost Sankoff: allowed [n][P][K] bool per tip; cost vectors [P][K], 0 on a tip's
    allowed states and infinite elsewhere; an internal node's cost of state s is the sum over
    its two subtrees of min_t (cost[t] + [s != t]).  No set is ever formed."""
    adj = _adjacency(edges)
    memo = {}
    INF = np.inf

    def below(C):
        """min over t of C[p][t] + [s != t], for every s."""
        m = C.min(axis=1, keepdims=True)
        return np.minimum(C, m + 1.0)

    def cost(u, v):
        key = (u, v)
        if key not in memo:
            others = [x for x in adj[u] if x != v]
            if not others:
                memo[key] = np.where(allowed[u], 0.0, INF)
            else:
                memo[key] = below(cost(others[0], u)) + below(cost(others[1], u))
        return memo[key]

    a, b = (int(x) for x in edges[root_edge])
    total = (below(cost(a, b)) + cost(b, a)).min(axis=1)
    assert np.all(np.isfinite(total))
    return _wsum(w, total.astype(np.int64))


# ---- schedules and fixtures ---------------------------------------------------------------

def schedule_edges(ops, root):
    """The edges of a schedule in op order: (left, parent), (right, parent) per op, then the
    root edge."""
    out = []
    for p, l, r in np.asarray(ops).reshape(-1, 3):
        out += [(int(l), int(p)), (int(r), int(p))]
    out.append((int(root[0]), int(root[1])))
    return out


def edges_schedule(edges, n, root_edge=0):
    """(ops int32 [n-2][3], root int32 [2], ids [2n-3]) of an edge list rooted on edge
    `root_edge`: a post-order, and per op-order edge its index in `edges`."""
    adj = {}
    for e, (u, v) in enumerate(edges):
        adj.setdefault(int(u), []).append((int(v), e))
        adj.setdefault(int(v), []).append((int(u), e))
    ops, ids = [], []

    def walk(u, came):
        kids = [(x, e) for x, e in adj[u] if x != came]
        if not kids:
            return
        for x, _ in kids:
            walk(x, u)
        ops.append((u, kids[0][0], kids[1][0]))
        ids.extend([kids[0][1], kids[1][1]])

    a, b = (int(x) for x in edges[root_edge])
    walk(a, b)
    walk(b, a)
    ids.append(root_edge)
    return (np.array(ops, dtype=np.int32).reshape(-1, 3), np.array([a, b], dtype=np.int32),
            np.array(ids, dtype=np.int64))


def random_edges(rng, n):
    """A random unrooted binary tree over tips 0..n-1: random attachments in random order."""
    order = rng.permutation(n)
    edges = [(int(order[0]), n), (int(order[1]), n), (int(order[2]), n)]
    for k in range(3, n):
        edges = attach(edges, int(rng.integers(len(edges))), int(order[k]), n + k - 2)
    return edges


def caterpillar_schedule(n):
    """The deepest op chain: ((((0, 1), 2), 3), ...)."""
    ops = [(n, 0, 1)] + [(n + i, n + i - 1, i + 1) for i in range(1, n - 2)]
    return np.array(ops, dtype=np.int32).reshape(-1, 3), np.array([2 * n - 3, n - 1], dtype=np.int32)


def balanced_schedule(n):
    """The shallowest op chains: neighbours paired level by level."""
    level, nxt, ops = list(range(n)), n, []
    while len(level) > 2:
        new = []
        i = 0
        while i + 1 < len(level) and len(new) + len(level) - i > 2:  # nodes left without a parent
            ops.append((nxt, level[i], level[i + 1]))
            new.append(nxt)
            nxt += 1
            i += 2
        level = new + level[i:]
    return np.array(ops, dtype=np.int32).reshape(-1, 3), np.array(level, dtype=np.int32)


def random_alignment(rng, n, P, K, n_codes=None, ambiguity=0.05):
    """(codes uint8 [n][P], table [n_codes][K]): codes 0..K-1 are the states, code K the full
    set (a gap), the further codes random proper subsets of two or more states; about
    `ambiguity` of the cells carry one of those, and column 0 is all gaps where P > 1."""
    n_codes = K + 3 if n_codes is None else n_codes
    table = np.zeros((n_codes, K))
    table[:K] = np.eye(K)
    table[K] = 1.0
    for c in range(K + 1, n_codes):
        size = int(rng.integers(2, max(K, 3)))
        table[c, rng.choice(K, size=min(size, K), replace=False)] = 1.0
    # a shared ancestral column with some noise, so that the trees carry signal
    base = rng.integers(K, size=P)
    codes = np.where(rng.random((n, P)) < 0.35, rng.integers(K, size=(n, P)), base[None])
    amb = rng.random((n, P)) < ambiguity
    codes = np.where(amb, rng.integers(K, n_codes, size=(n, P)), codes)
    if P > 1:
        codes[:, 0] = K
    return np.ascontiguousarray(codes, dtype=np.uint8), table


# the stepwise-addition cases the CPU and the device tests share: short alignments, so that
# several edges tie for the minimum (tests/test_parsimony.py asserts that they do)
STEP_TAXA = (3, 4, 5, 17, 65)
STEP_PATTERNS = 37


def stepwise_case(n, K=4):
    """(codes, table, weights int64 [P] with zeros, orders int32 [9][n]: the identity, its
    reverse and seven random permutations)."""
    rng = np.random.default_rng(1000 * K + n)
    codes, table = random_alignment(rng, n, STEP_PATTERNS, K)
    w = rng.integers(0, 4, size=STEP_PATTERNS).astype(np.int64)
    orders = [np.arange(n), np.arange(n)[::-1]] + [rng.permutation(n) for _ in range(7)]
    return codes, table, w, np.array(orders, dtype=np.int32)
