"""Tree sets for the tree-set tests, each encoded in the library's three forms, and their
reference results (tests/treeset_reference.py), computed once per shape."""
import functools

import numpy as np

import parsimony_reference as PR
import parsimony_spr_reference as PS
import treeset_reference as TR


def random_moves(rng, edges, k):
    """`edges` after k random SPR moves of DESIGN 4.26 (fewer where the tree has none)."""
    edges = np.array(edges, dtype=np.int32).reshape(-1, 2)
    for _ in range(k):
        for _ in range(50):
            d = int(rng.integers(2 * len(edges)))
            if PS.direction(edges, d) is None:
                continue
            tg = sorted(PS.targets(edges, d))
            if tg:
                edges = PS.apply_spr_edges(edges, d, tg[int(rng.integers(len(tg)))])
                break
    return edges


def random_tree(rng, n):
    """PR.random_edges' rule -- random attachments in random order, numbered as stepwise
    addition numbers them -- without copying the list at every step (thousands of tips)."""
    order = rng.permutation(n)
    edges = [(int(order[0]), n), (int(order[1]), n), (int(order[2]), n)]
    for k in range(3, n):
        e, m = int(rng.integers(len(edges))), n + k - 2
        a, b = edges[e]
        edges[e] = (a, m)
        edges += [(m, b), (int(order[k]), m)]
    return np.array(edges, dtype=np.int32)


def tip0_trees(n):
    """Edge lists with tip 0 in a cherry, on the root edge (edge 0 of the list) and deep in a
    caterpillar (n >= 5)."""
    ops, root = PR.caterpillar_schedule(n)       # ((0, 1), 2), ...: tip 0 in a cherry, deepest
    cherry = np.array(PR.schedule_edges(ops, root), dtype=np.int32)
    on_root = np.array([(b, a) if a == 0 else (a, b) for a, b in cherry], dtype=np.int32)
    k = int(np.flatnonzero((on_root == 0).any(axis=1))[0])
    on_root[[0, k]] = on_root[[k, 0]]            # tip 0's pendant edge is the edge list's first
    relabel = np.arange(2 * n - 2)
    relabel[0], relabel[n // 2] = n // 2, 0      # tip 0 in the middle of the chain
    deep = relabel[cherry].astype(np.int32)
    return [cherry, on_root, deep]


def edge_set(n, T, seed):
    """int32 [T][2n-3][2]: one random tree and a caterpillar, each copy 0 to 3 random SPR moves
    away, with exact duplicates, the tip-0 cases and one tree unrelated to the rest."""
    rng = np.random.default_rng(seed)
    base = np.array(PR.random_edges(rng, n), dtype=np.int32)
    fixed = tip0_trees(n)
    out = []
    for t in range(T):
        if t == 1 and T > 1:
            out.append(np.array(PR.random_edges(np.random.default_rng(seed + 977), n),
                                dtype=np.int32))      # unrelated
        elif t % 7 == 3:
            out.append(out[t - 2].copy())             # an exact duplicate
        elif t % 5 == 4:
            out.append(random_moves(rng, fixed[(t // 5) % 3], int(rng.integers(0, 3))))
        elif t % 11 == 6:
            out.append(fixed[(t // 11) % 3])
        else:
            out.append(random_moves(rng, base, int(rng.integers(0, 4))))
    return np.stack(out).astype(np.int32)


def random_postorder(rng, ops):
    """The same ops in another valid order: a random op whose children are made comes next."""
    ops = [tuple(int(v) for v in op) for op in ops]
    n = len(ops) + 2
    user = {c: i for i, (p, l, r) in enumerate(ops) for c in (l, r)}  # child -> its op
    waits = [int(l >= n) + int(r >= n) for p, l, r in ops]
    ready = [i for i, w in enumerate(waits) if w == 0]
    out = []
    while ready:
        p, l, r = ops[ready.pop(int(rng.integers(len(ready))))]
        out.append((p, l, r) if rng.integers(2) else (p, r, l))
        if p in user:
            waits[user[p]] -= 1
            if waits[user[p]] == 0:
                ready.append(user[p])
    assert len(out) == len(ops)
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def as_ops(rng, edges):
    """(ops, root) of an edge list: a random root edge, shuffled internal node numbers, a random
    valid op order."""
    n = (len(edges) + 3) // 2
    ops, root, _ = PR.edges_schedule(edges, n, int(rng.integers(len(edges))))
    name = np.arange(2 * n - 2)
    name[n:] = n + rng.permutation(n - 2)
    ops, root = name[ops].reshape(-1, 3), name[root]
    if rng.integers(2):
        root = root[::-1]
    return random_postorder(rng, ops), root.astype(np.int32)


def as_joins(rng, edges):
    """(joins, root) of an edge list, by its own random ops: op m's parent becomes n + m."""
    ops, root = as_ops(rng, edges)
    n = len(ops) + 2
    name = np.arange(2 * n - 2)
    name[ops[:, 0]] = n + np.arange(n - 2)
    return name[ops[:, 1:]].astype(np.int32), name[root].astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(n, T, seed=0):
    """dict(edges, ops, joins: the three encodings of one tree set; ref_edges, ref_ops,
    ref_joins: the reference's results on each)."""
    rng = np.random.default_rng(10007 * n + 31 * T + seed)
    edges = edge_set(n, T, 10007 * n + 31 * T + seed + 1)
    o = [as_ops(rng, e) for e in edges]
    j = [as_joins(rng, e) for e in edges]
    ops = (np.stack([x[0] for x in o]).astype(np.int32).reshape(T, n - 2, 3),
           np.stack([x[1] for x in o]).astype(np.int32))
    joins = (np.stack([x[0] for x in j]).astype(np.int32).reshape(T, n - 2, 2),
             np.stack([x[1] for x in j]).astype(np.int32))
    out = dict(n=n, T=T, edges=edges, ops=ops, joins=joins)
    out["ref_edges"] = TR.compare("edges", list(edges))
    out["ref_ops"] = TR.compare("ops", list(zip(*ops)))
    out["ref_joins"] = TR.compare("joins", list(zip(*joins)))
    return out
