"""The tree-set calls through TreeModel: rf_distance, map_support, the topology
classes of set_parsimony_tree's replicates and the replicate trees of bootstrap_nj."""
import numpy as np
import pytest

import treeset_reference as TR
from phylo_utils_amd import TreeModel, parsimony, treeset
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem

pytestmark = pytest.mark.gpu


def model(n=12, sites=300, seed=5):
    m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    rm = GammaRateModel(4, 0.7)
    tree, names, st = make_problem(n, sites, m, rm.rates, seed=seed)
    # the alignment's rows in another order than the sorted names
    order = np.random.default_rng(seed).permutation(n)
    aln = [(names[i], "".join("ACGT"[x] for x in st[i])) for i in order]
    tm = TreeModel()
    tm.set_alignment(aln, A.DNA)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    return tm, tree, [names[i] for i in order]


def labelled(tree, names):
    """{canonical split: label} of the labelled internal nodes of a tree."""
    row = {str(x): i for i, x in enumerate(names)}
    below, out = {}, {}
    for node in tree.seed_node.postorder():
        below[node] = (1 << row[node.label]) if node.is_leaf() else 0
        for c in node.children:
            below[node] |= below[c]
        s = TR.canonical(below[node], len(row))
        if s is not None and node.children and node is not tree.seed_node and \
                node.label is not None:
            assert out.setdefault(s, node.label) == node.label
    return out


def test_rf_distance():
    tm, tree, names = model()
    tm.set_tree(tree)
    other = "((t0,t3),(t1,(t2,t4)),((t5,t6),((t7,t8),(t9,(t10,t11)))));"
    assert sorted(names) == sorted("t%d" % i for i in range(12))
    want = treeset.rf_distances([tree, other, tree.as_newick()], names)
    assert tm.rf_distance(other) == int(want[0, 1]) > 0
    assert tm.rf_distance(tree.as_newick()) == 0 == int(want[0, 2])
    assert isinstance(tm.rf_distance(other), int)


def test_map_support_equals_the_bootstrap_support():
    """The NJ tree labelled from its own replicates through the split table carries, split by
    split, the labels bootstrap_nj gave it, and the same values."""
    tm, _, names = model()
    R = 30
    tree, support, n_ok, reps = tm.bootstrap_nj(R, seed=2, return_replicates=True)
    assert n_ok == R and len(tm.bootstrap_nj(R, seed=2)) == 3
    assert names == sorted(tm.names, key=tm.names.get)
    values, copy = tm.map_support(reps)
    n = len(names)
    assert values.shape == (2 * n - 3,) and np.isnan(values).sum() == n
    assert sorted(values[~np.isnan(values)]) == sorted(support)
    assert labelled(copy, names) == labelled(tree, names) and len(labelled(copy, names)) == n - 3
    assert 0.0 < support.min() < 1.0 or len(set(support)) > 1  # the labels differ between splits
    # the model's tree is untouched, the copy has its lengths
    assert copy is not tm.tree and all(x.length is not None for x in copy.leaf_nodes())
    # the same from Newick strings and from edge lists of other trees
    nwk = [tree.as_newick()] * 3 + ["((t0,t3),(t1,(t2,t4)),((t5,t6),((t7,t8),(t9,(t10,t11)))));"]
    v2, _ = tm.map_support(nwk)
    assert set(np.round(v2[~np.isnan(v2)] * 4)) <= {3.0, 4.0} and (v2[~np.isnan(v2)] >= 0.75).all()
    edges, _, _ = parsimony.stepwise_addition(tm._coded_alignment(), n_rep=6, seed=1)
    v3, c3 = tm.map_support(edges)
    by_hand = treeset.compare(edges, rows=0)
    held = {tuple(b): c for b, c in zip(by_hand.bits, by_hand.count)}
    want = {s: held.get(tuple(TR.bits_of([s], n)[0]), 0) / 6.0 for s in labelled(copy, names)}
    assert sorted(v3[~np.isnan(v3)]) == sorted(want.values())
    assert labelled(c3, names) == {s: "%d" % round(100 * v) for s, v in want.items()}


def test_parsimony_replicates_topology_classes():
    tm, _, names = model(n=14, sites=60, seed=9)
    out3 = tm.set_parsimony_tree(n_rep=12, seed=3, spr_rounds=0)
    assert len(out3) == 3
    tree, length, lengths, classes = tm.set_parsimony_tree(n_rep=12, seed=3, spr_rounds=0,
                                                           return_classes=True)
    assert length == out3[1] and np.array_equal(lengths, out3[2])
    assert tree.as_newick() == out3[0].as_newick()
    # the grouping of the refined edge lists themselves
    aln = tm._coded_alignment()
    w = parsimony.integer_weights(tm.siteweights, aln[0].shape[1])
    edges, _, _ = parsimony.stepwise_addition(aln, n_rep=12, seed=3, weights=w)
    edges, _, _ = parsimony.spr_search(aln, edges, weights=w, max_rounds=0)
    rf = TR.compare("edges", list(edges))["rf"]
    want = [min(b for b in range(12) if rf[a][b] == 0) for a in range(12)]
    assert list(classes) == want and classes.shape == (12,)
