"""DESIGN 4.27 in plain Python, on a path independent of the library's: splits are Python ints
(bit i = tip i), taken from the tip sets of a ``tree.Tree``'s nodes; U is ``sorted(set(...))``;
RF is a set symmetric difference; the majority-rule tree is built directly.

The rule.  T trees over the same n tips 0..n-1, internal nodes n..2n-3.  The split of an edge is
the set of tips on the side of the edge that does not hold tip 0; with 1 or n - 1 tips (a pendant
edge) it is trivial and has no id; a binary tree has exactly n - 3 others.  U: the distinct
non-trivial splits of all trees in ascending order as integers; the id of a split is its index in
U; count[u] the number of trees that hold split u; RF(a, b) = 2 (n - 3) - 2 |ids(a) & ids(b)|.
Each tree's 2n - 3 edges stand in its form's own order: for ops [n-2][3] (and joins [n-2][2], op
m = (n + m, joins[m])) edges 2i = (left_i, parent_i), 2i + 1 = (right_i, parent_i), then the root
edge; for an edge list [2n-3][2] the list's own.
"""
import numpy as np

from phylo_utils_amd.tree import Node, Tree


def form_edges(form, tree):
    """[(child end, parent end)] * (2n-3) of one tree in its form's edge order."""
    if form == "edges":
        return [(int(a), int(b)) for a, b in np.asarray(tree).reshape(-1, 2)]
    arr, root = tree
    arr = np.asarray(arr)
    n = len(arr) + 2
    out = []
    for m, row in enumerate(arr):
        p, l, r = (n + m, row[0], row[1]) if form == "joins" else row
        out += [(int(l), int(p)), (int(r), int(p))]
    return out + [(int(root[0]), int(root[1]))]


def to_tree(form, tree):
    """(tree.Tree whose leaves are labelled by their tip number, {node id: Node}): rooted on the
    form's last edge for ops and joins, on edge 0 for an edge list."""
    edges = form_edges(form, tree)
    adj = {}
    for a, b in edges:
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)
    n = (len(edges) + 3) // 2
    ra, rb = edges[0] if form == "edges" else edges[-1]
    seed = Node()
    made = {}
    stack = [(ra, rb, seed), (rb, ra, seed)]
    while stack:
        v, came, par = stack.pop()
        made[v] = par.add(Node(str(v) if v < n else None))
        for x in adj[v]:
            if x != came:
                stack.append((x, v, made[v]))
    return Tree(seed), made


def node_tipsets(tree):
    """{Node: int bitset of the leaves below it} of every non-seed node; leaves are labelled by
    tip number."""
    below = {}
    for node in tree.seed_node.postorder():
        if node.is_leaf():
            below[node] = 1 << int(node.label)
        else:
            s = 0
            for c in node.children:
                s |= below[c]
            below[node] = s
    del below[tree.seed_node]
    return below


def canonical(s, n):
    """The side without tip 0, or None for a trivial split."""
    if s & 1:
        s = ((1 << n) - 1) & ~s
    return s if 1 < bin(s).count("1") < n - 1 else None


def edge_splits(form, tree):
    """Per edge, in the form's order: the canonical split (int) or None on a pendant edge."""
    edges = form_edges(form, tree)
    n = (len(edges) + 3) // 2
    t, made = to_tree(form, tree)
    below = node_tipsets(t)
    out = []
    for a, b in edges:
        # the edge's lower end in the rooted copy: the one whose parent is the other, or -- on
        # the edge the copy is rooted on, both below the seed -- either
        na, nb = made[a], made[b]
        low = nb if nb.parent is na else na
        out.append(canonical(below[low], n))
    return out


def compare(form, trees):
    """dict(n, U [ints ascending], count, edge_ids [T][2n-3], rf [T][T]) of a tree set."""
    per = [edge_splits(form, t) for t in trees]
    n = (len(per[0]) + 3) // 2
    U = sorted(set(s for p in per for s in p if s is not None))
    index = {s: i for i, s in enumerate(U)}
    ids = [frozenset(index[s] for s in p if s is not None) for p in per]
    for a in ids:
        assert len(a) == n - 3
    count = [sum(1 for a in ids if u in a) for u in range(len(U))]
    rf = [[len(a ^ b) for b in ids] for a in ids]
    edge_ids = [[-1 if s is None else index[s] for s in p] for p in per]
    return dict(n=n, U=U, count=count, edge_ids=edge_ids, rf=rf)


def bits_of(U, n):
    """uint64 [len(U)][ceil(n / 64)] of int bitsets."""
    nw = (n + 63) // 64
    return np.array([[(s >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(nw)] for s in U],
                    dtype=np.uint64).reshape(len(U), nw)


def tree_splits(tree, names):
    """The non-trivial canonical splits (ints over the rows of `names`) of any ``tree.Tree``,
    polytomies allowed, from its nodes' tip sets."""
    row = {str(x): i for i, x in enumerate(names)}
    n = len(row)
    below, out = {}, set()
    for node in tree.seed_node.postorder():
        below[node] = (1 << row[node.label]) if node.is_leaf() else 0
        for c in node.children:
            below[node] |= below[c]
        s = canonical(below[node], n)
        if s is not None and node is not tree.seed_node:
            out.add(s)
    return out


def label(x):
    return "%d" % round(100 * float(x))


def majority_rule(U, count, T, n, names, threshold=0.5):
    """The consensus tree, built directly: the kept splits, largest first, each hung below the
    smallest kept split that contains it (else the seed); then every tip below the smallest kept
    split that holds it."""
    keep = [(s, c) for s, c in zip(U, count) if (c == T if threshold >= 1.0 else c > threshold * T)]
    keep.sort(key=lambda sc: -bin(sc[0]).count("1"))
    seed = Node()
    nodes = []  # (split, Node), largest first
    for s, c in keep:
        host = seed
        for s2, nd in nodes:  # the last match is the smallest superset
            if s & s2 == s:
                host = nd
        nodes.append((s, host.add(Node(label(c / float(T))))))
    for i in range(n):
        host = seed
        for s2, nd in nodes:
            if (s2 >> i) & 1:
                host = nd
        host.add(Node(str(names[i])))
    return Tree(seed)
