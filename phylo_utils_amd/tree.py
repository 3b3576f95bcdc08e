"""Trees and the flattened post-order schedule (no dendropy).

Mirrors the parts of ``phylo_utils/traversal.py`` and ``phylo_utils/utils.py``
the likelihood path uses:

* ``parse_newick`` -- a small Newick reader (labels, ``:lengths``, quoted labels,
  comments ``[...]`` skipped).
* ``deroot`` / ``resolve_polytomies`` -- ``deepcopy_tree`` (``utils.py:114-118``):
  a bifurcating seed loses one internal child (the second child if it is
  internal, else the first), whose edge length moves to its sister; nodes with
  more than two children keep the first child and hang the rest below new
  zero-length nodes.
* ``Traversal`` (``traversal.py:6-35``): non-seed nodes indexed in post-order
  (leaves included), ``names`` {leaf label: index}, ``root_edge`` = the seed's
  two children, ``brlens`` keyed by the sorted index pair with the seed's
  children joined by ``max`` of their lengths (``utils.py:202-213``), and
  ``postorder_traversal`` int32 [N-2][3] of (parent, child1, child2)
  (``utils.py:127-134``), and ``optimising_traversal`` int32 [3N-5][5]
  (``utils.py:137-188``, ``traversal.py:29,34-35``).
"""
from __future__ import annotations

import numpy as np


class Node(object):
    __slots__ = ("children", "parent", "length", "label")

    def __init__(self, label=None, length=None):
        self.children = []
        self.parent = None
        self.length = length
        self.label = label

    def add(self, child):
        child.parent = self
        self.children.append(child)
        return child

    def is_leaf(self):
        return not self.children

    @property
    def edge_length(self):
        return 0.0 if self.length is None else self.length

    def postorder(self):
        """Iterative post-order (deep caterpillars exceed Python's recursion limit)."""
        out, stack = [], [(self, False)]
        while stack:
            n, done = stack.pop()
            if done or not n.children:
                out.append(n)
                continue
            stack.append((n, True))
            for c in reversed(n.children):
                stack.append((c, False))
        return out

    def leaves(self):
        return [n for n in self.postorder() if n.is_leaf()]


class Tree(object):
    def __init__(self, seed):
        self.seed_node = seed

    def postorder_node_iter(self):
        return iter(self.seed_node.postorder())

    def leaf_nodes(self):
        return self.seed_node.leaves()

    def copy(self):
        return Tree(_copy(self.seed_node))

    def as_newick(self):
        return _write(self.seed_node) + ";"

    def deroot(self):
        """Collapse a basal bifurcation into a trifurcation (dendropy deroot semantics)."""
        seed = self.seed_node
        if len(seed.children) != 2:
            return self
        a, b = seed.children
        if len(b.children) >= 2:
            keep, drop = a, b
        elif len(a.children) >= 2:
            keep, drop = b, a
        else:
            return self
        keep.length = keep.edge_length + drop.edge_length
        pos = seed.children.index(drop)
        for c in drop.children:
            c.parent = seed
        seed.children[pos:pos + 1] = drop.children
        return self

    def resolve_polytomies(self):
        """Binary everywhere: first child stays, the others go below new 0-length nodes."""
        for n in self.seed_node.postorder():
            while len(n.children) > 2:
                rest = n.children[1:]
                n.children = n.children[:1]
                new = n.add(Node(length=0.0))
                for c in rest:
                    new.add(c)
                n = new
        return self


def _copy(node):
    new = Node(node.label, node.length)
    stack = [(node, new)]
    while stack:
        src, dst = stack.pop()
        for c in src.children:
            d = dst.add(Node(c.label, c.length))
            stack.append((c, d))
    return new


def _write(node):
    def lab(n):
        s = ""
        if n.label is not None:
            s = n.label if all(ch not in n.label for ch in " (),:;[]'") else \
                "'" + n.label.replace("'", "''") + "'"
        if n.length is not None and n is not node:
            s += ":" + repr(float(n.length))
        return s

    # iterative writer
    parts = {}
    for n in node.postorder():
        if n.children:
            parts[id(n)] = "(" + ",".join(parts.pop(id(c)) for c in n.children) + ")" + lab(n)
        else:
            parts[id(n)] = lab(n)
    return parts[id(node)]


def parse_newick(text):
    """Newick string -> Tree (rooted as written)."""
    s = text.strip()
    i, n = 0, len(s)
    root = Node()
    cur = root
    stack = []
    expect_child = True

    def read_label(i):
        if i < n and s[i] == "'":
            j = i + 1
            buf = []
            while j < n:
                if s[j] == "'":
                    if j + 1 < n and s[j + 1] == "'":
                        buf.append("'")
                        j += 2
                        continue
                    break
                buf.append(s[j])
                j += 1
            return "".join(buf), j + 1
        j = i
        while j < n and s[j] not in "(),:;[":
            j += 1
        lab = s[i:j].strip()
        return (lab if lab else None), j

    def read_length(i):
        j = i
        while j < n and s[j] not in "(),;[":
            j += 1
        return float(s[i:j]), j

    started = False
    while i < n:
        ch = s[i]
        if ch.isspace():
            i += 1
        elif ch == "[":
            j = s.find("]", i)
            if j < 0:
                raise ValueError("unterminated comment in newick")
            i = j + 1
        elif ch == "(":
            if not started:
                started = True
                stack.append(root)
                cur = root
            else:
                child = cur.add(Node())
                stack.append(child)
                cur = child
            expect_child = True
            i += 1
        elif ch == ",":
            if not stack:
                raise ValueError("unbalanced ',' in newick")
            cur = stack[-1]
            expect_child = True
            i += 1
        elif ch == ")":
            if not stack:
                raise ValueError("unbalanced ')' in newick")
            cur = stack.pop()
            expect_child = False
            i += 1
            lab, i = read_label(i)
            cur.label = lab if lab is not None else cur.label
        elif ch == ":":
            i += 1
            cur.length, i = read_length(i)
        elif ch == ";":
            break
        else:
            if not started:  # single leaf tree
                started = True
            lab, i = read_label(i)
            if expect_child and stack:
                cur = stack[-1].add(Node(lab))
            else:
                cur.label = lab
            expect_child = False
    if stack:
        raise ValueError("unbalanced parentheses in newick")
    return Tree(root)


def prepare_tree(tree):
    """deepcopy_tree (utils.py:114-118): copy, deroot, resolve polytomies."""
    if isinstance(tree, str):
        tree = parse_newick(tree)
    return tree.copy().deroot().resolve_polytomies()


class BranchLengths(dict):
    """Length lookup by unordered node-index pair (utils.py:191-199)."""

    def __getitem__(self, key):
        val = self.get(key)
        if val is None:
            val = self.get(tuple(key)[::-1])
        if val is None:
            raise KeyError(key)
        return val


def optimising_traversal(seed, node_dict):
    """get_optimising_traversal (utils.py:137-188): 3N-5 rows of 5 node indices.

    Row 0 is (-1, -1, -1, LEFT, RIGHT): optimise the root edge.  Then, depth first from
    LEFT and from RIGHT, every other node NOD with parent PAR, sibling SIB and
    grandparent GPA (the other root-edge end when PAR is LEFT or RIGHT) adds
    (PAR, SIB, GPA, NOD, PAR) -- re-orient PAR's partials towards NOD from SIB and GPA,
    then optimise edge (NOD, PAR) -- and, after its children, an internal NOD adds
    (NOD, CH1, CH2, -1, -1), restoring its post-order partials.  Iterative (a
    1000-taxon caterpillar is deeper than Python's recursion limit).
    """
    left, right = seed.children
    rows = [(-1, -1, -1, node_dict[left], node_dict[right])]
    for start in (left, right):
        stack = [(start, False)]
        while stack:
            node, done = stack.pop()
            nod = node_dict[node]
            if done:
                ch1, ch2 = node.children
                rows.append((nod, node_dict[ch1], node_dict[ch2], -1, -1))
                continue
            if node is not left and node is not right:
                par = node.parent
                gpa = right if par is left else (left if par is right else par.parent)
                sib = next(c for c in par.children if c is not node)  # utils.get_sibling
                rows.append((node_dict[par], node_dict[sib], node_dict[gpa], nod,
                             node_dict[par]))
            if node.children:
                ch1, ch2 = node.children
                stack.append((node, True))
                stack.append((ch2, False))
                stack.append((ch1, False))
    return np.array(rows, dtype=np.int32).reshape(-1, 5)


class Traversal(object):
    """Node indexing + post-order schedule for the engine (traversal.py:6-35)."""

    def __init__(self, tree):
        seed = tree.seed_node
        order = [n for n in seed.postorder() if n is not seed]
        self.node_dict = {n: i for i, n in enumerate(order)}
        self.names = {}
        for n in order:
            if n.is_leaf():
                if n.label is None:
                    raise ValueError("unlabelled leaf in tree")
                if n.label in self.names:
                    raise ValueError("duplicate leaf label %r" % n.label)
                self.names[n.label] = self.node_dict[n]
        if len(seed.children) != 2:
            raise ValueError("seed node must have two children after resolution")
        self.n_nodes = len(order)
        self.root_edge = tuple(self.node_dict[c] for c in seed.children)
        self.brlens = BranchLengths()
        for n in order:
            if n.parent is seed:
                nb = [c for c in seed.children if c is not n][0]
                length = max(c.edge_length for c in seed.children)
            else:
                nb = n.parent
                length = n.edge_length
            self.brlens[tuple(sorted((self.node_dict[n], self.node_dict[nb])))] = length
        ops = [(self.node_dict[n], self.node_dict[n.children[0]], self.node_dict[n.children[1]])
               for n in order if n.children]
        self.postorder_traversal = np.array(ops, dtype=np.int32).reshape(-1, 3)
        self.optimising_traversal = optimising_traversal(seed, self.node_dict)

    def op_lengths(self):
        """[n_ops][2] lengths of (parent, child1), (parent, child2) for pu_set_schedule."""
        return np.array([[self.brlens[(p, a)], self.brlens[(p, b)]]
                         for p, a, b in self.postorder_traversal], dtype=np.float64).reshape(-1, 2)

    def root_length(self):
        return float(self.brlens[self.root_edge])


# ---------------------------------------------------------------- nearest-neighbour interchange
# Host helpers of the NNI search (phylo_utils_amd.nni).  Nodes are named by their
# Traversal index on prepare_tree(tree), an internal edge by (NOD, PAR) as the optimising
# traversal's rows name it: NOD the child end, PAR its parent -- the root edge by (LEFT, RIGHT).
# The quartet around the edge is (x0, x1 | x2, x3): NOD's two children, then NOD's sibling and
# grandparent side (on the root edge: RIGHT's two children).  Arrangement 1 is (x0, x2 | x1, x3),
# arrangement 2 is (x0, x3 | x1, x2).

def internal_edges(tree):
    """The internal edges [(NOD, PAR)] of `tree`, in optimising-traversal order: the rows whose
    two ends both have children (the edges pu_nni_sweep scores; N - 3 of them)."""
    tr = Traversal(prepare_tree(tree))
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    return [(int(r[3]), int(r[4])) for r in tr.optimising_traversal
            if r[3] >= 0 and int(r[3]) in internal and int(r[4]) in internal]


def apply_nni_moves(tree, moves):
    """prepare_tree(tree) with every move (nod, par, which, length) applied: `which` 1 exchanges
    x1 with x2, 2 exchanges x0 with x2 (the module comment above), every subtree keeping its own
    edge length; `length`, when not None, replaces the central edge's.  The moves' edges must not
    share an end node (all are taken on the node numbering of the tree as given)."""
    t = prepare_tree(tree)
    tr = Traversal(t)
    node = {i: n for n, i in tr.node_dict.items()}
    left, right = t.seed_node.children
    ends = set()
    for nod, par, which, length in moves:
        if which not in (1, 2):
            raise ValueError("which must be 1 or 2, got %r" % (which,))
        if nod not in node or par not in node:
            raise ValueError("no node %r or %r in the tree" % (nod, par))
        if nod in ends or par in ends:
            raise ValueError("moves share node %d or %d" % (nod, par))
        ends.update((nod, par))
        n, p = node[nod], node[par]
        if n.is_leaf() or p.is_leaf():
            raise ValueError("edge (%d, %d) is not internal" % (nod, par))
        root_edge = (n is left and p is right) or (n is right and p is left)
        if root_edge:
            x2 = p.children[0]
        elif n.parent is p:
            x2 = next(c for c in p.children if c is not n)
        else:
            raise ValueError("(%d, %d): no edge with child end %d" % (nod, par, nod))
        mine = n.children[2 - which]
        i, j = n.children.index(mine), p.children.index(x2)
        n.children[i], p.children[j] = x2, mine
        x2.parent, mine.parent = n, p
        n.label = None  # a support label belonged to the split that is gone
        if root_edge:
            p.label = None
        if length is not None:
            if root_edge:  # the root edge's length is the larger of its two halves
                left.length, right.length = float(length), 0.0
            else:
                n.length = float(length)
    return t


def apply_nni(tree, nod, par, which, length=None):
    """A new Tree: the nearest-neighbour interchange `which` (1 or 2) at internal edge
    (nod, par) of `tree`; every length is kept, the central one replaced by `length` if given."""
    return apply_nni_moves(tree, [(nod, par, which, length)])


def select_moves(candidates):
    """The round's moves from candidates [dict(nod, par, which, gain, ...)]: by descending gain,
    ties by the sorted (nod, par) pair, taken greedily, skipping every candidate whose edge shares
    an end node with an edge already taken."""
    order = sorted(candidates, key=lambda m: (-m["gain"], tuple(sorted((m["nod"], m["par"])))))
    taken, used = [], set()
    for m in order:
        if m["nod"] in used or m["par"] in used:
            continue
        taken.append(m)
        used.update((m["nod"], m["par"]))
    return taken


def with_lengths(tree, brlens):
    """A copy of the prepared `tree` whose edge lengths are `brlens` (Traversal.brlens, keyed by
    node-index pairs); the root edge's length goes to the seed's first child."""
    t = tree.copy()
    tr = Traversal(t)
    bl = BranchLengths(brlens)
    left, right = t.seed_node.children
    for n, i in tr.node_dict.items():
        if n.parent is t.seed_node:
            n.length = float(bl[tr.root_edge]) if n is left else 0.0
        else:
            n.length = float(bl[(i, tr.node_dict[n.parent])])
    return t


# ---------------------------------------------------------------- subtree pruning and regrafting
# Host helpers of the SPR search (phylo_utils_amd.spr).  Nodes are named by their
# Traversal index on prepare_tree(tree), the tree is taken as unrooted: the two ends of the root
# edge are ordinary internal nodes joined by an edge, the seed is not a node.  A prune candidate
# is a directed edge (n, o): the subtree on n's side is cut, o -- internal, with other neighbours
# x and y -- is dissolved and x, y are joined by one edge of length len(x, o) + len(y, o), which
# leaves the rest tree R; R must keep at least two edges (x and y are not both leaves).  A move
# (n, o, u, v) regrafts the subtree at the midpoint of R's edge (u, v) on its pendant length
# len(n, o); (u, v) = (x, y) is the merged edge, distance 0, an edge sharing a node with it has
# distance 1 (the NNI topologies), and so on outward.

def _neighbours(tr):
    """{node: {neighbour: length}} of the unrooted tree of a Traversal."""
    adj = {i: {} for i in range(tr.n_nodes)}
    for (a, b), t in tr.brlens.items():
        adj[a][b] = float(t)
        adj[b][a] = float(t)
    return adj


def _spr_ends(adj, n, o):
    """(x, y) of candidate (n, o), or None where it is none."""
    if o not in adj.get(n, ()) or len(adj[o]) != 3:
        return None
    x, y = [z for z in adj[o] if z != n]
    if len(adj[x]) == 1 and len(adj[y]) == 1:
        return None
    return x, y


def spr_candidates(tree):
    """The prune candidates [(n, o)] of `tree` in optimising-traversal order: both directions
    of every edge (NOD, PAR) -- (NOD, PAR), then (PAR, NOD) -- wherever the dissolved end is
    internal and the rest tree keeps at least two edges."""
    tr = Traversal(prepare_tree(tree))
    adj = _neighbours(tr)
    out = []
    for row in tr.optimising_traversal:
        nod, par = int(row[3]), int(row[4])
        if nod < 0:
            continue
        for n, o in ((nod, par), (par, nod)):
            if _spr_ends(adj, n, o) is not None:
                out.append((n, o))
    return out


def spr_rows(traversal, radius=None):
    """The rows of one scoring pass (pu_spr_sweep) over `traversal`: (rows int32 [R][5] = the
    optimising traversal, inner_off int64 [R + 1], inner_rows int32 [I][6] = (x0, x1, x2, A, B,
    S), inner_len [I][4] = (len1, len2, t, l), moves int32 [I][5] = (n, o, u, v, distance)).

    While the walk stands on edge (NOD, PAR) every node's vector points at that edge, so for the
    candidates (NOD, PAR) and (PAR, NOD) every vector of R points at the merged edge: its two
    ends score distance 0 as they are.  From there an iterative depth-first search of R (a
    1000-taxon caterpillar is deeper than Python's recursion limit) re-orients a node u towards
    a far neighbour v from its other far neighbour and its near one (an update row, A = -1),
    scores edge (v, u) (a scoring row, x0 = -1: A = v, B = u, S = n), descends into v, does the
    same for the other far neighbour, and on the way out restores u from its two far neighbours
    (an update row).  `radius`: only edges of distance <= radius (None: every edge of R).  An
    update row has u = v = distance = -1 in `moves`."""
    tr = traversal
    adj = _neighbours(tr)
    rows = np.ascontiguousarray(tr.optimising_traversal, dtype=np.int32).reshape(-1, 5)
    off, inner, lens, moves = [0], [], [], []
    limit = None if radius is None else int(radius)

    def update(n, o, u, a, la, b, lb):
        inner.append((u, a, b, -1, -1, -1))
        lens.append((la, lb, 0.0, 0.0))
        moves.append((n, o, -1, -1, -1))

    def score(n, o, a, b, t, l, dist):
        inner.append((-1, -1, -1, a, b, n))
        lens.append((0.0, 0.0, t, l))
        moves.append((n, o, a, b, dist))

    for row in rows:
        nod, par = int(row[3]), int(row[4])
        for n, o in (((nod, par), (par, nod)) if nod >= 0 else ()):
            ends = _spr_ends(adj, n, o)
            if ends is None:
                continue
            x, y = ends
            l, merged = adj[n][o], adj[o][x] + adj[o][y]
            score(n, o, x, y, merged, l, 0)
            if limit is not None and limit < 1:
                continue
            for start, other in ((x, y), (y, x)):
                # (u, near, length to near, far neighbours, distance of u's far edges, stage)
                stack = [[start, other, merged, [z for z in adj[start] if z != o], 1, 0]]
                while stack:
                    top = stack[-1]
                    u, near, t_near, far, dist, stage = top
                    if len(far) != 2 or stage == 2:  # a leaf of R, or both sides done
                        if len(far) == 2:
                            update(n, o, u, far[0], adj[u][far[0]], far[1], adj[u][far[1]])
                        stack.pop()
                        continue
                    v, w = far[stage], far[1 - stage]
                    top[5] = stage + 1
                    update(n, o, u, w, adj[u][w], near, t_near)
                    score(n, o, v, u, adj[u][v], l, dist)
                    if limit is None or dist < limit:
                        stack.append([v, u, adj[u][v], [z for z in adj[v] if z != u], dist + 1, 0])
        off.append(len(inner))
    return (rows, np.array(off, dtype=np.int64),
            np.array(inner, dtype=np.int32).reshape(-1, 6),
            np.array(lens, dtype=np.float64).reshape(-1, 4),
            np.array(moves, dtype=np.int32).reshape(-1, 5))


def apply_spr(tree, n, o, u, v):
    """A new Tree: the subtree on n's side of edge (n, o) of prepare_tree(tree) cut out, the
    dissolved o's other neighbours x, y joined by one edge of length len(x, o) + len(y, o), edge
    (u, v) of the rest tree -- (x, y), in either order, names the merged edge -- split into two
    halves at a new node, and the subtree hung from that node at its old length len(n, o).  All
    other lengths are kept.  The result is rooted on the pendant edge; internal labels are
    dropped (a support label belongs to a split of the old tree)."""
    tr = Traversal(prepare_tree(tree))
    adj = _neighbours(tr)
    n, o, u, v = int(n), int(o), int(u), int(v)
    ends = _spr_ends(adj, n, o) if n in adj else None
    if ends is None:
        raise ValueError("(%d, %d) is no prune candidate: an edge whose end %d is internal, with "
                         "at least two edges left" % (n, o, o))
    x, y = ends
    l = adj[n][o]
    merged = adj[o][x] + adj[o][y]
    for z in (x, y):
        del adj[z][o]
    adj[o] = {n: l}
    adj[x][y] = adj[y][x] = merged
    side, todo = {n}, [n]  # n's subtree: what is reached from n without passing o
    while todo:
        for z in adj[todo.pop()]:
            if z != o and z not in side:
                side.add(z)
                todo.append(z)
    if u not in adj or v not in adj.get(u, ()) or o in (u, v) or u in side or v in side:
        raise ValueError("(%d, %d) is no edge of the rest tree of (%d, %d)" % (u, v, n, o))
    t = adj[u].pop(v)
    del adj[v][u]
    for z in (u, v):
        adj[o][z] = adj[z][o] = 0.5 * t
    label = {i: node.label for node, i in tr.node_dict.items() if node.is_leaf()}
    seed = Node()
    stack = []
    for child, parent, length in ((n, o, l), (o, n, 0.0)):
        stack.append((child, parent, seed.add(Node(label.get(child), length))))
    while stack:
        i, came, node = stack.pop()
        for z in sorted(adj[i]):
            if z != came:
                stack.append((z, i, node.add(Node(label.get(z), adj[i][z]))))
    return Tree(seed)
