"""Sets of trees on the CPU: the plain-Python rule (tests/treeset_reference.py) against the
older Robinson-Foulds helper, the host-side consensus builder of phylo_utils_amd.treeset on
hand-made split tables, and every refusal pu_treeset_compare makes before it touches a device."""
import numpy as np
import pytest

import nj_reference as NR
import parsimony_reference as PR
import treeset_cases as C
import treeset_reference as TR
from phylo_utils_amd import _native as N
from phylo_utils_amd import treeset
from phylo_utils_amd.parsimony import edges_to_tree


@pytest.mark.parametrize("n", [4, 5, 9, 40])
def test_reference_rf_equals_the_bipartition_helper(n):
    rng = np.random.default_rng(n)
    names = ["t%02d" % i for i in range(n)]
    trees = [np.array(PR.random_edges(rng, n), dtype=np.int32) for _ in range(3)]
    trees += [C.random_moves(rng, trees[0], k) for k in (1, 2, 3)]
    rf = TR.compare("edges", trees)["rf"]
    built = [edges_to_tree(e, names) for e in trees]
    for a in range(len(trees)):
        for b in range(len(trees)):
            assert rf[a][b] == NR.robinson_foulds(built[a], built[b])
    if n > 4:
        assert max(max(row) for row in rf) > 0


@pytest.mark.parametrize("n,T", [(3, 2), (4, 3), (9, 5), (70, 4)])
def test_three_forms_of_a_tree_have_the_same_reference_splits(n, T):
    case = C.case(n, T, seed=1)
    e, o, j = (case["ref_" + f] for f in ("edges", "ops", "joins"))
    assert e["U"] == o["U"] == j["U"] and e["count"] == o["count"] == j["count"]
    assert e["rf"] == o["rf"] == j["rf"]
    names = [str(i) for i in range(n)]
    for t in range(T):
        want = set(s for s in TR.edge_splits("edges", case["edges"][t]) if s is not None)
        assert len(want) == n - 3
        for form, tree in (("ops", (case["ops"][0][t], case["ops"][1][t])),
                           ("joins", (case["joins"][0][t], case["joins"][1][t]))):
            assert TR.tree_splits(TR.to_tree(form, tree)[0], names) == want
            got = TR.edge_splits(form, tree)
            assert set(s for s in got if s is not None) == want
            assert sum(s is None for s in got) == n


def table(n, T, splits, names=None):
    """A TreeSetResult of hand-made splits [(tips, count)], in ascending order."""
    rows = sorted((sum(1 << i for i in tips), c) for tips, c in splits)
    return treeset.TreeSetResult(n, T, TR.bits_of([s for s, _ in rows], n),
                                 [c for _, c in rows], names=names)


def clades(tree):
    """{frozenset of leaf labels: label} of the internal non-seed nodes."""
    below, out = {}, {}
    for node in tree.seed_node.postorder():
        below[node] = frozenset([node.label]) if node.is_leaf() else \
            frozenset().union(*(below[c] for c in node.children))
        if node.children and node is not tree.seed_node:
            out[below[node]] = node.label
    return out


def test_consensus_five_taxa_known_answer():
    names = list("abcde")
    # 10 trees: {d, e} in 9, {c, d, e} in 6, {b, c} in 4 (conflicts with the second)
    r = table(5, 10, [((3, 4), 9), ((2, 3, 4), 6), ((1, 2), 4)], names)
    t = treeset.consensus(r)
    assert clades(t) == {frozenset("de"): "90", frozenset("cde"): "60"}
    assert t.as_newick() in ("(a,b,(c,(d,e)90)60);",)
    assert all(x.length is None for x in t.seed_node.postorder())
    assert np.array_equal(treeset.split_frequencies(r), [0.4, 0.9, 0.6])
    assert clades(treeset.consensus(r, 0.6)) == {frozenset("de"): "90"}  # 6 of 10 is not > 0.6


def test_consensus_of_nothing_above_threshold_is_the_star():
    r = table(6, 4, [((1, 2), 2), ((3, 4), 2), ((2, 3), 1)])
    t = treeset.consensus(r)
    assert clades(t) == {} and len(t.seed_node.children) == 6
    assert sorted(x.label for x in t.leaf_nodes()) == [str(i) for i in range(6)]
    empty = treeset.TreeSetResult(3, 2, np.zeros((0, 1), dtype=np.uint64), [])
    assert len(treeset.consensus(empty).seed_node.children) == 3


def test_strict_consensus_and_thresholds():
    r = table(7, 8, [((5, 6), 8), ((4, 5, 6), 7), ((1, 2), 8), ((1, 2, 3), 5)])
    assert clades(treeset.consensus(r, 1.0)) == {frozenset("56"): "100", frozenset("12"): "100"}
    assert clades(treeset.consensus(r, 0.5)) == {frozenset("56"): "100", frozenset("456"): "88",
                                                 frozenset("12"): "100", frozenset("123"): "62"}
    for bad in (0.49, 1.01, -1.0):
        with pytest.raises(ValueError):
            treeset.consensus(r, bad)
    # the direct builder of the reference gives the same trees
    U = [int(b[0]) for b in r.bits]
    for th in (0.5, 0.7, 1.0):
        a = treeset.consensus(r, th)
        b = TR.majority_rule(U, list(r.count), 8, 7, [str(i) for i in range(7)], th)
        assert clades(a) == clades(b)


def test_consensus_across_the_word_boundary():
    n = 70
    r = table(n, 3, [(tuple(range(60, 68)), 3), (tuple(range(63, 66)), 2), ((1, 69), 2)])
    c = clades(treeset.consensus(r))
    assert c[frozenset(str(i) for i in range(60, 68))] == "100"
    assert c[frozenset(str(i) for i in range(63, 66))] == "67"
    assert c[frozenset(["1", "69"])] == "67" and len(c) == 3


def test_topology_classes_on_edge_ids():
    r = treeset.TreeSetResult(5, 4, TR.bits_of([6, 12, 24], 5), [3, 2, 3])
    r.edge_ids = np.array([[-1, 0, -1, 1, -1, -1, -1], [1, -1, -1, -1, 0, -1, -1],
                           [-1, -1, 2, -1, -1, 0, -1], [-1, 2, -1, -1, -1, -1, 0]], dtype=np.int32)
    assert list(treeset.topology_classes(r)) == [0, 0, 2, 2]


def call(n, T, form, trees, roots, n_rows, ids=True, U=True):
    E = min(max(2 * n - 3, 1), 64)
    out = np.zeros((min(max(T, 1), 4), E), dtype=np.int32)  # a refused call writes nothing
    nu = np.zeros(1, dtype=np.int64)
    rc = N.lib().pu_treeset_compare(0, n, T, form, N.ptr(trees), N.ptr(roots), n_rows,
                                    N.ptr(out) if ids else None, N.ptr(nu) if U else None,
                                    None, None, None)
    return rc, N.last_error()


def test_refusals_before_any_device():
    n = 6
    ops, root = PR.caterpillar_schedule(n)
    ops, roots = ops[None].copy(), root[None].copy()
    edges = np.array(PR.schedule_edges(ops[0], root), dtype=np.int32)[None]
    joins = np.ascontiguousarray(ops[:, :, 1:])
    bad = N.PU_E_ARG
    assert call(n, 1, 0, None, roots, 0)[0] == bad
    assert call(n, 1, 0, ops, roots, 0, ids=False)[0] == bad
    assert call(n, 1, 0, ops, roots, 0, U=False)[0] == bad
    assert call(n, 1, 0, ops, None, 0)[0] == bad          # ops without roots
    assert call(n, 1, 1, joins, None, 0)[0] == bad        # joins without roots
    assert call(2, 1, 0, ops, roots, 0)[0] == bad
    assert call(8193, 1, 0, ops, roots, 0)[0] == bad      # PU_NJ_MAX_N = 8192
    assert call(n, 0, 0, ops, roots, 0)[0] == bad
    # T (n - 3) >= 2^31: 262241 * 8189 = 2^31 + 7901 is the first T refused at n = 8192, and
    # 2^30 * 2 = 2^31 at n = 5.  (A set just below the limit is valid and would be converted:
    # gigabytes of host memory, so it is not called here.)
    for big_n, big_T in ((8192, 262241), (5, 1 << 30), (8192, 2147483647)):
        assert big_T * (big_n - 3) >= 2 ** 31
        rc, msg = call(big_n, big_T, 0, ops, roots, 0)
        assert rc == bad and "2^31" in msg, msg
    assert 262240 * 8189 < 2 ** 31
    assert call(n, 1, 0, ops, roots, -1)[0] == bad
    assert call(n, 1, 0, ops, roots, 2)[0] == bad
    assert call(n, 1, 3, ops, roots, 0)[0] == bad and "form" in N.last_error()
    assert call(n, 1, -1, ops, roots, 0)[0] == bad
    # trees that are no binary trees over tips 0..n-1; the message names the tree
    two = np.concatenate([ops, ops])
    two_roots = np.concatenate([roots, roots])
    two[1, 2, 1] = two[1, 1, 1]                            # a child used twice
    rc, msg = call(n, 2, 0, two, two_roots, 0)
    assert rc == bad and "tree 1" in msg
    late = ops.copy()
    late[0, [0, 1]] = late[0, [1, 0]]                      # a child before it is made
    rc, msg = call(n, 1, 0, late, roots, 0)
    assert rc == bad and "tree 0" in msg
    rc, msg = call(n, 1, 0, ops, np.array([[0, 1]], dtype=np.int32), 0)
    assert rc == bad and "root edge" in msg
    j2 = joins.copy()
    j2[0, 1, 0] = 2 * n                                    # a cluster that does not exist
    rc, msg = call(n, 1, 1, j2, roots, 0)
    assert rc == bad and "tree 0" in msg
    e2 = np.concatenate([edges, edges, edges])
    e2[2, 3] = e2[2, 4]                                    # a tip on two edges
    rc, msg = call(n, 3, 2, e2, None, 0)
    assert rc == bad and "tree 2" in msg
    e3 = edges.copy()
    e3[0, 0, 0] = 2 * n - 2                                # a node out of range
    assert call(n, 1, 2, e3, None, 0)[0] == bad


def test_python_layer_refusals():
    with pytest.raises(ValueError):
        treeset.compare([])
    with pytest.raises(ValueError):
        treeset.compare(np.zeros((2, 8, 2), dtype=np.int32))   # 2n - 3 is odd
    with pytest.raises(ValueError):
        treeset.compare((np.zeros((2, 4, 3), np.int32), np.zeros((2, 2), np.int32)), form="joins")
    with pytest.raises(ValueError):
        treeset.compare(np.zeros((1, 9, 2), dtype=np.int32), form="trees")


def test_lists_of_edge_lists_and_their_op_lists():
    """A Python list of edge lists -- two, four or five of them too, the lengths of a (joins,
    roots) pair and of an nj_joins tuple -- is an edge batch; the host conversion of an edge
    batch to op lists keeps every tree's splits."""
    rng = np.random.default_rng(3)
    for n in (3, 4, 9, 70):
        trees = [np.array(PR.random_edges(rng, n), dtype=np.int32) for _ in range(5)]
        for k in (1, 2, 4, 5):
            form, a, roots, _, _ = treeset._batch(trees[:k], None, None)
            assert form == "edges" and roots is None and np.array_equal(a, np.stack(trees[:k]))
        ops, roots = treeset._edges_as_ops(np.stack(trees))
        assert ops.shape == (5, n - 2, 3) and roots.shape == (5, 2)
        assert TR.compare("ops", list(zip(ops, roots)))["U"] == TR.compare("edges", trees)["U"]
        assert TR.compare("ops", list(zip(ops, roots)))["rf"] == TR.compare("edges", trees)["rf"]
    pair = (np.zeros((2, 7, 2), np.int32), np.zeros((2, 2), np.int32))
    assert treeset._batch(pair, None, None)[0] == "joins"
    bad = np.stack([np.array(PR.random_edges(rng, 6), dtype=np.int32)])
    bad[0, 2] = bad[0, 3]
    with pytest.raises(ValueError):
        treeset._edges_as_ops(bad)
