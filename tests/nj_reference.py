"""numpy restatement of the neighbour-joining / BIONJ specification, written from
the rule and not from the kernels, and the tree helpers its tests need: bipartitions and the
Robinson-Foulds distance, branch lengths by bipartition and patristic distances of a
``tree.Tree``.

Test infrastructure: nothing under ``phylo_utils_amd/`` imports it.  Every sum the rule orders is
a sequential add (``np.cumsum(...)[-1]``), every expression is grouped as the rule groups it, and
numpy contracts nothing, so the device result can be compared bit for bit.
"""
import numpy as np


def _seq_sum(x):
    """x_0 + x_1 + ... left to right."""
    return np.cumsum(np.asarray(x, dtype=np.float64))[-1]


def nj(D, method="nj", gaps=True):
    """The rule on one matrix D [n][n] (upper triangle read, diagonal ignored).  Returns a dict:
    joins int32 [n-2][2], lens [n-2][2], root int32 [2], root_len, q [n-3], and -- with `gaps`
    -- gap [n-3], the relative gap (Q_second - Q_best) / max(|Q_best|, |Q_second|) between the
    best and the second-best criterion of every join.  With four clusters a pair and its
    complement have the same Q identically (Q_ab = -(D_ac + D_ad + D_bc + D_bd) = Q_cd), and
    joining either gives the same unrooted tree, so there the second-best is taken outside the
    chosen pair and its complement."""
    bionj = {"nj": False, "bionj": True}[method]
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    assert D.shape == (n, n) and n >= 3
    N = 2 * n - 2
    lower = np.tril(np.full((n, n), np.inf))  # + inf on and below the diagonal
    up = np.triu(D, 1)
    W = np.zeros((N, N))
    W[:n, :n] = up + up.T
    V = W.copy() if bionj else None
    R = np.zeros(N)
    for i in range(n):
        R[i] = _seq_sum(np.delete(W[i, :n], i))
    RV = R.copy() if bionj else None  # V = D: the same adds
    live = list(range(n))
    joins = np.zeros((n - 2, 2), dtype=np.int32)
    lens = np.zeros((n - 2, 2))
    q = np.zeros(max(n - 3, 0))
    gap = np.zeros(max(n - 3, 0))
    for m in range(n - 3):
        r = n - m
        L = np.array(live)
        sub = W[np.ix_(L, L)]
        Rl = R[L]
        Q = ((r - 2.0) * sub - Rl[:, None]) - Rl[None, :]
        # pairs a < b only; row-major, so the first minimum is the smallest (a, b)
        flat = (Q + lower[:r, :r]).ravel()
        e = int(np.argmin(flat))
        i, j = divmod(e, r)
        a, b = int(L[i]), int(L[j])
        q[m] = Q[i, j]
        if gaps:
            if r == 4:  # the best pair outside the chosen pair and its complement
                other = [x for x in range(4) if x != i and x != j]
                rest = Q + lower[:r, :r]
                rest[i, j] = rest[other[0], other[1]] = np.inf
                second = rest.min()
            else:
                second = np.partition(flat, 1)[1]
            scale = max(abs(q[m]), abs(second))
            gap[m] = (second - q[m]) / scale if scale > 0 else 0.0
        u = n + m
        dab = W[a, b]
        den = 2.0 * (r - 2.0)
        la = 0.5 * dab + (R[a] - R[b]) / den
        lb = dab - la
        joins[m] = (a, b)
        lens[m] = (la, lb)
        K = np.array([k for k in live if k != a and k != b])
        dak, dbk = W[a, K], W[b, K]
        if bionj:
            vab = V[a, b]
            lam = 0.5
            if vab != 0.0:
                lam = 0.5 + (RV[b] - RV[a]) / (den * vab)
                lam = 0.0 if lam < 0.0 else (1.0 if lam > 1.0 else lam)
            oml = 1.0 - lam
            c = (lam * oml) * vab
            duk = lam * (dak - la) + oml * (dbk - lb)
            vak, vbk = V[a, K], V[b, K]
            vuk = (lam * vak + oml * vbk) - c
            V[u, K] = V[K, u] = vuk
            RV[K] = ((RV[K] - vak) - vbk) + vuk
            RV[u] = _seq_sum(vuk)
        else:
            duk = 0.5 * ((dak + dbk) - dab)
        W[u, K] = W[K, u] = duk
        R[K] = ((R[K] - dak) - dbk) + duk
        R[u] = _seq_sum(duk)
        live = [k for k in live if k != a and k != b] + [u]
    a, b, c = live
    dab, dac, dbc = W[a, b], W[a, c], W[b, c]
    joins[n - 3] = (a, b)
    lens[n - 3] = (0.5 * ((dab + dac) - dbc), 0.5 * ((dab + dbc) - dac))
    return dict(joins=joins, lens=lens, root=np.array([2 * n - 3, c], dtype=np.int32),
                root_len=0.5 * ((dac + dbc) - dab), q=q, gap=gap)


# ---------------------------------------------------------------------------- trees
def _leafsets(tree):
    """{node: frozenset of the leaf labels below it} of every non-seed node."""
    below = {}
    for node in tree.seed_node.postorder():
        if node.is_leaf():
            below[node] = frozenset([node.label])
        else:
            below[node] = frozenset().union(*(below[c] for c in node.children))
    below.pop(tree.seed_node)
    return below


def split_lengths(tree):
    """{bipartition: length} of the unrooted tree: a bipartition is the frozenset of the leaf
    labels on the side without the smallest label; edges with the same bipartition (the two at
    a bifurcating seed) add up."""
    below = _leafsets(tree)
    every = frozenset().union(*below.values())
    ref = min(every)
    out = {}
    for node, s in below.items():
        key = every - s if ref in s else s
        if key:
            out[key] = out.get(key, 0.0) + node.edge_length
    return out


def bipartitions(tree):
    """The non-trivial bipartitions of the unrooted tree."""
    n = len(tree.leaf_nodes())
    return {s for s in split_lengths(tree) if 1 < len(s) < n - 1}


def robinson_foulds(tree_a, tree_b):
    return len(bipartitions(tree_a) ^ bipartitions(tree_b))


def patristic(tree, names):
    """[n][n] path lengths between the leaves `names` of the tree."""
    adj = {}
    for node in tree.seed_node.postorder():
        for c in node.children:
            adj.setdefault(node, []).append((c, c.edge_length))
            adj.setdefault(c, []).append((node, c.edge_length))
    leaf = {x.label: x for x in tree.leaf_nodes()}
    out = np.zeros((len(names), len(names)))
    for i, name in enumerate(names):
        dist = {leaf[name]: 0.0}
        stack = [leaf[name]]
        while stack:
            x = stack.pop()
            for y, l in adj[x]:
                if y not in dist:
                    dist[y] = dist[x] + l
                    stack.append(y)
        out[i] = [dist[leaf[m]] for m in names]
    return 0.5 * (out + out.T)


# ---------------------------------------------------------------------------- fixtures
def random_matrix(seed, n):
    """A symmetric matrix with uniform(0.05, 2) entries and a zero diagonal."""
    rng = np.random.default_rng(seed)
    up = np.triu(rng.uniform(0.05, 2.0, (n, n)), 1)
    return up + up.T


def perturbed_additive(seed, n, noise=0.05):
    """The patristic matrix of a synthetic.random_tree, every entry scaled by 1 + noise *
    uniform(-1, 1), symmetric."""
    from phylo_utils_amd.synthetic import random_tree
    rng = np.random.default_rng(seed)
    tree = random_tree(rng, n, 0.02, 0.3)
    D = patristic(tree, ["t%d" % i for i in range(n)])
    up = np.triu(D * (1.0 + noise * rng.uniform(-1.0, 1.0, (n, n))), 1)
    return up + up.T
