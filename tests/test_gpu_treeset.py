"""Sets of trees on the device (pu_treeset.hip) against the plain-Python restatement
of the rule (tests/treeset_reference.py): every comparison is exact."""
import numpy as np
import pytest

import nj_reference as NR
import parsimony_reference as PR
import treeset_cases as C
import treeset_reference as TR
from phylo_utils_amd import _native as N
from phylo_utils_amd import bootstrap, nj, treeset

pytestmark = pytest.mark.gpu

# the RF tile is 16 trees wide: T = 1, 2 below it, 16 on it, 17 and 33 above one and two tiles
SHAPES = [(n, T) for n in (3, 4, 5, 63, 64, 65, 129, 200) for T in (1, 2, 17, 33)]
SHAPES += [(128, 17), (65, 16), (5, 16)]


def arg(case, form):
    return case["edges"] if form == "edges" else case[form]


def check(case, form, r):
    ref, n, T = case["ref_" + form], case["n"], case["T"]
    assert (r.n, r.n_trees, r.n_unique) == (n, T, len(ref["U"]))
    assert r.bits.dtype == np.uint64 and r.bits.shape == (len(ref["U"]), (n + 63) // 64)
    assert np.array_equal(r.bits, TR.bits_of(ref["U"], n))
    assert np.array_equal(r.count, np.array(ref["count"], dtype=np.int32))
    assert np.array_equal(r.edge_ids, np.array(ref["edge_ids"], dtype=np.int32).reshape(T, 2 * n - 3))
    assert np.array_equal(r.rf, np.array(ref["rf"], dtype=np.int32).reshape(T, T))


@pytest.mark.parametrize("n,T", SHAPES)
def test_three_forms_against_the_reference(n, T):
    """U, bits, count, RF and each form's edge ids in its own edge order equal the reference's;
    the forms -- other root edges, node numbers and op orders -- agree with each other."""
    case = C.case(n, T)
    refs = [case["ref_" + f] for f in ("edges", "ops", "joins")]
    for other in refs[1:]:  # the reference itself sees one tree set in three encodings
        assert other["U"] == refs[0]["U"] and other["rf"] == refs[0]["rf"]
    if n > 4 and T > 2:
        rf = np.array(refs[0]["rf"])
        assert rf.max() > 0 and (rf[np.triu_indices(T, 1)] == 0).any()
    for form in ("edges", "ops", "joins"):
        r = treeset.compare(arg(case, form), form=form)
        check(case, form, r)
        assert np.array_equal(r.rf, r.rf.T) and not r.rf.diagonal().any()
        assert r.form == form and r.edges.shape == (T, 2 * n - 3, 2)


def test_two_hundred_taxa_three_hundred_trees():
    case = C.case(200, 300)
    check(case, "edges", treeset.compare(case["edges"]))
    check(case, "joins", treeset.compare(case["joins"], form="joins"))


def test_reencodings_of_one_tree_are_at_distance_zero():
    case = C.case(65, 17)
    rng = np.random.default_rng(5)
    e = case["edges"][0]
    enc = [C.as_ops(rng, e) for _ in range(6)]
    ops = (np.stack([x[0] for x in enc]), np.stack([x[1] for x in enc]))
    r = treeset.compare(ops)
    assert not r.rf.any() and r.n_unique == 62 and (r.count == 6).all()
    assert (treeset.topology_classes(r) == 0).all()


@pytest.mark.parametrize("n", [5, 70])
def test_tip_zero_in_a_cherry_on_the_root_edge_and_deep(n):
    """Tip 0 as a child of the first op, as an end of the root edge, and in the middle of a
    caterpillar: the complemented clusters."""
    cat, root = PR.caterpillar_schedule(n)
    flip = (2 * n - 3) - (np.arange(2 * n - 2) - n)  # reverse the internal numbering
    name = np.concatenate([np.arange(n)[::-1], flip[n:]])
    on_root = (name[cat].astype(np.int32), name[root].astype(np.int32))  # root edge (.., tip 0)
    assert 0 in on_root[1]
    mid = np.arange(2 * n - 2)
    mid[0], mid[n // 2] = n // 2, 0
    deep = (mid[cat].astype(np.int32), mid[root].astype(np.int32))
    trees = [(cat, root), on_root, deep]
    ops = (np.stack([t[0] for t in trees]), np.stack([t[1] for t in trees]))
    ref = TR.compare("ops", trees)
    r = treeset.compare(ops)
    assert np.array_equal(r.bits, TR.bits_of(ref["U"], n))
    assert np.array_equal(r.edge_ids, np.array(ref["edge_ids"], dtype=np.int32))
    assert np.array_equal(r.rf, np.array(ref["rf"], dtype=np.int32))


@pytest.mark.parametrize("n,T", [(65, 33), (4, 17), (3, 2)])
def test_row_counts(n, T):
    case = C.case(n, T)
    full = treeset.compare(case["edges"])
    for k in (0, 1, T):
        r = treeset.compare(case["edges"], rows=k)
        if k == 0:
            assert r.rf is None
        else:
            assert r.rf.shape == (k, T) and np.array_equal(r.rf, full.rf[:k])
        assert np.array_equal(r.edge_ids, full.edge_ids) and np.array_equal(r.bits, full.bits)


def test_nullable_outputs_change_no_other():
    case = C.case(129, 17)
    ops, roots = case["ops"]
    n, T = case["n"], case["T"]
    E, ns, nw = 2 * n - 3, n - 3, (n + 63) // 64

    def call(want_bits, want_count, want_rf):
        ids = np.full((T, E), -7, dtype=np.int32)
        U = np.zeros(1, dtype=np.int64)
        bits = np.zeros((T * ns, nw), dtype=np.uint64) if want_bits else None
        count = np.zeros(T * ns, dtype=np.int32) if want_count else None
        rf = np.full((T, T), -7, dtype=np.int32) if want_rf else None
        N.check(N.lib().pu_treeset_compare(0, n, T, 0, N.ptr(ops), N.ptr(roots), T, N.ptr(ids),
                                           N.ptr(U), N.ptr(bits), N.ptr(count), N.ptr(rf)))
        return ids, int(U[0]), bits, count, rf

    full = call(True, True, True)
    ref = case["ref_ops"]
    assert full[1] == len(ref["U"]) and np.array_equal(full[4], np.array(ref["rf"]))
    for mask in ((False, False, False), (True, False, False), (False, True, False),
                 (False, False, True)):
        got = call(*mask)
        assert np.array_equal(got[0], full[0]) and got[1] == full[1]
        for i in (2, 3, 4):
            if got[i] is not None:
                assert np.array_equal(got[i], full[i])


@pytest.mark.parametrize("n", [12, 70])
def test_support_equals_split_support_on_nj_replicates(n):
    """The edges of an NJ tree labelled from 25 NJ replicates (random matrices: the reference's
    own and copies of it with every entry moved by up to a fifth, so that some splits survive):
    bit for bit what pu_split_support gives for the cluster below each edge."""
    R = 25
    D = NR.random_matrix(40 + n, n)
    rng = np.random.default_rng(n)
    ref = NR.nj(D, gaps=False)
    reps = []
    for r in range(R):
        up = np.triu(D * (1.0 + (0.2 * r / R) * rng.uniform(-1.0, 1.0, (n, n))), 1)
        reps.append(NR.nj(up + up.T, gaps=False))
    joins = np.stack([x["joins"] for x in reps]).astype(np.int32)
    roots = np.stack([x["root"] for x in reps]).astype(np.int32)
    rj, rr = ref["joins"].astype(np.int32), ref["root"].astype(np.int32)
    want, n_ok = bootstrap.split_support((rj, rr), (joins, roots))
    assert n_ok == R and want.min() >= 1.0 / R  # replicate 0 is the reference's own matrix
    got, tree = treeset.support((rj, rr), (joins, roots), form="joins")
    assert tree is None and got.shape == (2 * n - 3,)
    X = n + n - 3  # the last cluster: the root edge's other end carries the root edge's split
    below = [int(c) for c in rj.reshape(-1)] + [int(rr[0]) if rr[1] == X else int(rr[1])]
    seen = []
    for e, c in enumerate(below):
        if c < n:
            assert np.isnan(got[e])
        else:
            assert got[e] == want[c - n]  # bit for bit
            seen.append(c - n)
    assert sorted(seen) == list(range(n - 3))
    # the same values on a Tree of the reference, from the same replicates
    names = ["t%d" % i for i in range(n)]
    t = nj.joins_to_tree(names, rj, ref["lens"], rr, ref["root_len"], 1e-8)
    got_t, labelled = treeset.support(t, (joins, roots), names=names)
    assert sorted(got_t[~np.isnan(got_t)]) == sorted(want)
    labels = sorted(int(x.label) for x in labelled.seed_node.postorder()
                    if x.children and x.label is not None)
    assert len(labels) >= n - 3 and set(labels) == set(round(100 * s) for s in want)


def labelled_splits(tree, names):
    """{canonical split: label} of the internal nodes of a tree that carry a non-trivial one."""
    row = {str(x): i for i, x in enumerate(names)}
    below, out = {}, {}
    for node in tree.seed_node.postorder():
        below[node] = (1 << row[node.label]) if node.is_leaf() else 0
        for c in node.children:
            below[node] |= below[c]
        s = TR.canonical(below[node], len(row))
        if s is not None and node.children and node is not tree.seed_node:
            out[s] = node.label
    return out


@pytest.mark.parametrize("n,T,threshold", [(65, 33, 0.5), (65, 33, 0.8), (65, 33, 1.0),
                                           (5, 17, 0.5), (3, 2, 0.5)])
def test_consensus_of_a_device_result(n, T, threshold):
    case = C.case(n, T)
    ref = case["ref_edges"]
    r = treeset.compare(case["edges"], rows=0)
    names = [str(i) for i in range(n)]
    got = treeset.consensus(r, threshold)
    want = TR.majority_rule(ref["U"], ref["count"], T, n, names, threshold)
    assert NR.robinson_foulds(got, want) == 0
    assert labelled_splits(got, names) == labelled_splits(want, names)
    assert sorted(x.label for x in got.leaf_nodes()) == sorted(names)
    assert np.array_equal(treeset.split_frequencies(r), np.array(ref["count"]) / float(T))


@pytest.mark.parametrize("n,T", [(64, 33), (5, 17), (3, 2)])
def test_topology_classes_group_by_zero_distance(n, T):
    case = C.case(n, T)
    r = treeset.compare(case["joins"], form="joins")
    want = [min(b for b in range(T) if r.rf[a, b] == 0) for a in range(T)]
    got = treeset.topology_classes(r)
    assert list(got) == want
    if n > 4:
        assert 1 < len(set(got)) < T  # duplicates and different trees both


def test_profile_times():
    case = C.case(63, 17)
    treeset.profile(True)
    try:
        treeset.compare(case["edges"])
        ms = treeset.kernel_ms()
    finally:
        treeset.profile(False)
    assert len(ms) == 3 and all(np.isfinite(x) and x >= 0.0 for x in ms)
    with pytest.raises(N.PhyloHipError):
        treeset.kernel_ms()


def big_case(n, T, seed):
    """Random trees and copies of them a few SPR moves apart, as an edge batch and as ops, with
    the reference's result on the edge batch."""
    rng = np.random.default_rng(seed)
    base = C.random_tree(rng, n)
    if n > 4096:  # the host side of a larger case takes seconds: one move, no more
        edges = [C.random_moves(rng, base, 1) for _ in range(T - 2)]
    else:
        edges = [C.random_moves(rng, base, int(rng.integers(0, 4))) for _ in range(T - 2)]
    edges += [edges[0].copy(), C.random_tree(rng, n)]
    enc = [C.as_ops(rng, e) for e in edges]
    ops = (np.stack([x[0] for x in enc]).astype(np.int32), np.stack([x[1] for x in enc]))
    return np.stack(edges), ops, TR.compare("edges", edges)


@pytest.mark.parametrize("n,T", [(256, 17), (1300, 18), (4100, 3)])
def test_the_other_paths_of_the_kernels(n, T, monkeypatch):
    """n = 1300: one tree's clusters do not fit the LDS of a workgroup, so they stay in memory
    with one thread per word (21 words: a workgroup of 64), and the 32 id lists of an RF tile do
    not fit either and are read from memory.  n = 4100: 65 words, a workgroup of 128.  n = 256:
    the last size of four words; with several trees per workgroup (PU_TREESET_GROUP, the mapping
    measured against the one kept) sixteen trees' clusters no longer fit, eight do.  Both RF
    kernels, the one kept and the one measured against it, give the reference's matrix."""
    edges, ops, ref = big_case(n, T, n + T)
    want_rf = np.array(ref["rf"], dtype=np.int32)
    for kernel in ("lane", "wave"):
        if kernel == "wave":
            monkeypatch.setenv("PU_TREESET_RF", "wave")
        r = treeset.compare(edges)
        assert np.array_equal(r.bits, TR.bits_of(ref["U"], n))
        assert np.array_equal(r.count, np.array(ref["count"], dtype=np.int32))
        assert np.array_equal(r.edge_ids, np.array(ref["edge_ids"], dtype=np.int32))
        assert np.array_equal(r.rf, want_rf)
        assert np.array_equal(treeset.compare(ops, rows=3).rf, want_rf[:3])
    monkeypatch.delenv("PU_TREESET_RF")
    monkeypatch.setenv("PU_TREESET_GROUP", "64")
    assert np.array_equal(treeset.compare(edges, rows=0).bits, TR.bits_of(ref["U"], n))


@pytest.mark.parametrize("n,T", [(5, 17), (64, 33), (65, 33), (129, 17), (200, 33)])
def test_several_trees_per_workgroup(n, T, monkeypatch):
    """The split kernel's other mapping: 64, 32 and 16 trees per workgroup, the last workgroup
    partly filled."""
    case = C.case(n, T)
    monkeypatch.setenv("PU_TREESET_GROUP", "64")
    check(case, "edges", treeset.compare(case["edges"]))


def test_wave_per_pair_kernel_on_the_tile_edges(monkeypatch):
    case = C.case(65, 33)
    monkeypatch.setenv("PU_TREESET_RF", "wave")
    check(case, "edges", treeset.compare(case["edges"]))
