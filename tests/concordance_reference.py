"""DESIGN 4.29 in plain Python and numpy, on a path independent of the library's: clades are
sorted tip lists found by walking away from the branch, picks index those lists, counts are numpy
masks over the pattern axis, the gene factors use tests/treeset_reference.py's split sets.  Philox
is tests/sim_reference.py's.

The rule.  The tree is an edge list [2n-3][2], tips 0..n-1 the alignment's rows, internal nodes
n..2n-3.  Edge e = (x, y) is internal iff both ends are internal nodes; x's other two edges in
increasing edge id lead to clades A and B, y's to C and D; a clade lists the tips beyond its
edge in ascending order.  Q = n_quartets, m = |A||B||C||D|.  m <= Q: nq[e] = m, quartet q is the
mixed-radix number (ia, ib, ic, id), id fastest.  Else nq[e] = Q and clade k of quartet q takes
the tip at index min(floor(u |X|), |X| - 1), u = philox_u(seed, g = q, c2 = 4e + k, c3 = 2).  A
pattern is decisive for a quartet iff all four state sets are singletons; its weight goes to n1
where sa = sb, sc = sd, sa != sc, to n2 where sa = sc, sb = sd, sa != sb, to n3 where sa = sd,
sb = sc, sa != sb.  Finish, over the quartets with t = n1 + n2 + n3 > 0: sCF = 100 mean(n1 / t),
sDF1, sDF2 alike, sN = mean(t), sQ their number; sQ = 0: NaN factors, sN = 0.
"""
import numpy as np

import sim_reference as SR
import treeset_reference as TR


def adjacency(edges):
    edges = [(int(a), int(b)) for a, b in np.asarray(edges).reshape(-1, 2)]
    adj = {}
    for g, (a, b) in enumerate(edges):
        adj.setdefault(a, []).append((g, b))
        adj.setdefault(b, []).append((g, a))
    return edges, adj


def tips_beyond(adj, n, start, came):
    """The tips reached from `start` without going back to `came`, ascending."""
    out, stack = [], [(start, came)]
    while stack:
        v, c = stack.pop()
        if v < n:
            out.append(v)
        for _, f in adj[v]:
            if f != c:
                stack.append((f, v))
    return sorted(out)


def clades(edges):
    """{internal edge id: [A, B, C, D]}, each a list of tips in ascending order."""
    edges, adj = adjacency(edges)
    n = (len(edges) + 3) // 2
    out = {}
    for e, (x, y) in enumerate(edges):
        if x < n or y < n:
            continue
        four = []
        for end in (x, y):
            for g, f in sorted(adj[end]):
                if g != e:
                    four.append(tips_beyond(adj, n, f, end))
        out[e] = four
    return out


def philox_u(seed, q, c2):
    """u of counter (q lo, q hi, c2, 2) under the 64-bit seed, for arrays q and c2 that broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.asarray(q, dtype=np.uint64)
    q, c2 = np.broadcast_arrays(q, np.asarray(c2, dtype=np.uint64))
    x = SR.philox4x32_10((q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), c2, np.uint64(2)),
                         (seed & 0xFFFFFFFF, seed >> 32))
    m = ((x[1] >> np.uint64(5)) << np.uint64(26)) | (x[0] >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def quartets(edges, Q, seed):
    """(nq [2n-3], taxa [2n-3][Q][4]) with -1 in every slot that holds no quartet."""
    E = len(np.asarray(edges).reshape(-1, 2))
    nq = np.zeros(E, dtype=np.int32)
    taxa = np.full((E, Q, 4), -1, dtype=np.int32)
    for e, four in clades(edges).items():
        size = [len(c) for c in four]
        m = size[0] * size[1] * size[2] * size[3]
        if m <= Q:
            nq[e] = m
            for q in range(m):
                t, idx = q, [0, 0, 0, 0]
                for k in (3, 2, 1):
                    idx[k] = t % size[k]
                    t //= size[k]
                idx[0] = t
                taxa[e, q] = [four[k][idx[k]] for k in range(4)]
        else:
            nq[e] = Q
            u = philox_u(seed, np.arange(Q)[:, None], 4 * e + np.arange(4)[None, :])
            for q in range(Q):
                for k in range(4):
                    i = min(int(np.floor(u[q, k] * size[k])), size[k] - 1)
                    taxa[e, q, k] = four[k][i]
    return nq, taxa


def single_states(codes, table):
    """int [n][n_pat]: the single state of every code, -1 where the state set is no singleton."""
    table = np.asarray(table, dtype=np.float64)
    single = np.array([int(np.flatnonzero(row > 0)[0]) if (row > 0).sum() == 1 else -1
                       for row in table])
    return single.astype(np.int8)[np.asarray(codes)]  # states are below 32


def counts(codes, table, weights, nq, taxa):
    """uint64 [2n-3][Q][3] of the picks."""
    s = single_states(codes, table)
    n_pat = s.shape[1]
    w = np.ones(n_pat, dtype=np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    out = np.zeros(taxa.shape[:2] + (3,), dtype=np.uint64)
    for e in np.flatnonzero(nq):
        for q in range(int(nq[e])):
            a, b, c, d = (s[t] for t in taxa[e, q])
            dec = (a >= 0) & (b >= 0) & (c >= 0) & (d >= 0)
            out[e, q, 0] = w[dec & (a == b) & (c == d) & (a != c)].sum(dtype=np.uint64)
            out[e, q, 1] = w[dec & (a == c) & (b == d) & (a != b)].sum(dtype=np.uint64)
            out[e, q, 2] = w[dec & (a == d) & (b == c) & (a != b)].sum(dtype=np.uint64)
    return out


def site(codes, table, weights, edges, Q, seed):
    """dict(nq, taxa, counts) of a call."""
    nq, taxa = quartets(edges, Q, seed)
    return dict(nq=nq, taxa=taxa, counts=counts(codes, table, weights, nq, taxa))


def finish(counts_e, nq_e):
    """(sCF, sDF1, sDF2, sN, sQ) of one branch, in Python floats."""
    shares, ts = [[], [], []], []
    for q in range(int(nq_e)):
        n = [int(v) for v in counts_e[q]]
        t = n[0] + n[1] + n[2]
        if t > 0:
            ts.append(t)
            for i in range(3):
                shares[i].append(n[i] / t)
    if not ts:
        return float("nan"), float("nan"), float("nan"), 0.0, 0
    k = len(ts)
    return (100.0 * (sum(shares[0]) / k), 100.0 * (sum(shares[1]) / k), 100.0 * (sum(shares[2]) / k),
            sum(ts) / k, k)


def bitset(tips):
    s = 0
    for t in tips:
        s |= 1 << int(t)
    return s


def gene(ref_edges, form, trees):
    """{internal edge id of the reference: (gCF, gDF1, gDF2, gDFP, gN)}: the shares of `trees`
    (a list in `form`, as tests/treeset_reference.py takes them) that hold AB|CD, AC|BD, AD|BC."""
    n = (len(np.asarray(ref_edges).reshape(-1, 2)) + 3) // 2
    held = [set(s for s in TR.edge_splits(form, t) if s is not None) for t in trees]
    T = len(held)
    out = {}
    for e, (A, B, C, D) in clades(ref_edges).items():
        share = []
        for other in (B, C, D):
            s = TR.canonical(bitset(A) | bitset(other), n)
            share.append(100.0 * (sum(1 for h in held if s in h) / T))
        out[e] = (share[0], share[1], share[2], 100.0 - share[0] - share[1] - share[2], T)
    return out
