"""Tree sets with branch lengths on the device (pu_treedist.hip) against the
plain-Python restatement of the rule (tests/treedist_reference.py): every comparison is exact,
``==`` on the integers and bit for bit on the doubles."""
import numpy as np
import pytest

import parsimony_reference as PR
import treedist_cases as DC
import treedist_reference as D
import treeset_cases as C
from phylo_utils_amd import _native as N
from phylo_utils_amd import treeset

pytestmark = pytest.mark.gpu

ALL = ("wrf", "kf", "path", "wpath")

# n = 3, 4, 5: no split, one, two.  64 / 65: the bitset word boundary, and 2016 / 2080 pairs on
# either side of the 2048-pair segment.  130: three words, five segments.  257 / 258: the last n
# whose 32 keyed vectors and id lists of a weighted tile fit the LDS and the first that does not
# (32 (20 n - 36) bytes against 160 KiB).  T = 1, 2, 33, 65 are off the 16-tree tiles.
SHAPES = [(3, 2), (4, 1), (5, 65), (64, 2), (65, 33), (130, 3), (257, 2), (258, 2)]


def run(case, form, rows=None):
    return treeset.distances(DC.arg(case, form), ALL, lengths=case["len_" + form], rows=rows,
                             form=form, squared=True)


def check(got, ref, rows=None):
    for key, raw in (("wrf", "wrf"), ("kf", "kf2"), ("wpath", "wpath2")):
        want = np.asarray(ref[raw], dtype=np.float64)[:rows]
        assert got[key].dtype == np.float64 and got[key].shape == want.shape
        assert np.array_equal(DC.bits(got[key]), DC.bits(want)), key
    want = np.array(ref["path2"], dtype=np.uint64)[:rows]
    assert got["path"].dtype == np.uint64 and np.array_equal(got["path"], want)


@pytest.mark.parametrize("n,T", SHAPES)
def test_three_forms_against_the_reference(n, T):
    """wRF, KF2, Path2 and WPath2 of the same trees in the three forms equal the reference's, and
    so do the split and tip length sums."""
    case = DC.case(n, T)
    ref = case["ref"]
    for form in ("edges", "ops", "joins"):
        got = run(case, form)
        check(got, ref)
        for key in ALL:
            assert np.array_equal(got[key], got[key].T) and not got[key].diagonal().any()
        r, split_mean, tip_mean = treeset.split_lengths(DC.arg(case, form),
                                                        lengths=case["len_" + form], form=form)
        assert r.n_unique == len(ref["U"])
        count = np.array(ref["count"], dtype=np.float64)
        assert np.array_equal(DC.bits(split_mean), DC.bits(np.array(ref["split_sum"]) / count))
        assert np.array_equal(DC.bits(tip_mean), DC.bits(np.array(ref["tip_sum"]) / float(T)))
    if n > 4 and T > 2:
        assert np.array(ref["wrf"])[np.triu_indices(T, 1)].min() > 0.0


def test_square_roots_on_the_host():
    case = DC.case(64, 2)
    got = treeset.distances(case["edges"], ALL, lengths=case["len_edges"])
    ref = case["ref"]
    assert np.array_equal(got["wrf"], np.array(ref["wrf"]))
    assert np.array_equal(got["kf"], np.sqrt(np.array(ref["kf2"])))
    assert np.array_equal(got["path"], np.sqrt(np.array(ref["path2"], dtype=np.float64)))
    assert np.array_equal(got["wpath"], np.sqrt(np.array(ref["wpath2"])))
    one = treeset.distances(case["edges"], "kf", lengths=case["len_edges"])
    assert isinstance(one, np.ndarray) and np.array_equal(one, got["kf"])


@pytest.mark.parametrize("n,T", [(5, 65), (64, 2)])
def test_row_counts(n, T):
    case = DC.case(n, T)
    for k in (0, 1, T):
        got = run(case, "edges", rows=k)
        for key in ALL:
            assert got[key].shape == (k, T)
        check(got, case["ref"], rows=k)


def test_nullable_outputs_change_no_other():
    case = DC.case(65, 33)
    ops, roots = case["ops"]
    n, T = 65, 33
    L = np.ascontiguousarray(case["len_ops"])

    def call(mask):
        f = [np.full((T, T), -7.0) if m else None for m in mask[:2]]
        p = np.full((T, T), 7, dtype=np.uint64) if mask[2] else None
        w = np.full((T, T), -7.0) if mask[3] else None
        U = np.zeros(1, dtype=np.int64) if mask[4] else None
        s = np.full(T * (n - 3), -7.0) if mask[5] else None
        t = np.full(n, -7.0) if mask[6] else None
        N.check(N.lib().pu_treedist(0, n, T, 0, N.ptr(ops), N.ptr(roots), N.ptr(L), T, N.ptr(f[0]),
                                    N.ptr(f[1]), N.ptr(p), N.ptr(w), N.ptr(U), N.ptr(s), N.ptr(t)))
        return [f[0], f[1], p, w, U, s, t]

    full = call([True] * 7)
    u = int(full[4][0])
    assert u == len(case["ref"]["U"]) and (full[5][u:] == -7.0).all()
    assert np.array_equal(DC.bits(full[5][:u]), DC.bits(case["ref"]["split_sum"]))
    for i in range(7):
        got = call([j == i for j in range(7)])
        assert np.array_equal(got[i], full[i])
    call([False] * 7)


def test_identical_trees_are_at_distance_zero():
    case = DC.case(65, 33)
    T = 17
    edges = np.stack([case["edges"][0]] * T)
    L = np.stack([case["len_edges"][0]] * T)
    got = treeset.distances(edges, ALL, lengths=L, squared=True)
    for key in ALL:
        assert got[key].shape == (T, T) and not got[key].any()


def test_caterpillars_without_a_shared_split():
    """Caterpillars over tip orders that share no non-trivial split: every split key is held by
    one tree of a pair alone."""
    n = 9
    cat, root = PR.caterpillar_schedule(n)
    order = [np.arange(n), np.array([0, 2, 4, 6, 8, 1, 3, 5, 7]), np.array([0, 3, 6, 1, 4, 7, 2, 5, 8])]
    trees = []
    for o in order:
        name = np.concatenate([o, np.arange(n, 2 * n - 2)])
        trees.append((name[cat].astype(np.int32), name[root].astype(np.int32)))
    rng = np.random.default_rng(3)
    L = DC.random_lengths(rng, (3, 2 * n - 3))
    ops = (np.stack([t[0] for t in trees]), np.stack([t[1] for t in trees]))
    rf = treeset.compare(ops).rf
    assert (rf[np.triu_indices(3, 1)] == 2 * (n - 3)).all()
    ref = D.distances("ops", trees, L)
    check(treeset.distances(ops, ALL, lengths=L, squared=True), ref)


def test_one_topology_with_other_lengths():
    """RF = 0 and wRF > 0; re-encodings of one tree with the same lengths are at 0."""
    case = DC.case(65, 33)
    rng = np.random.default_rng(11)
    e = case["edges"][0]
    enc = [C.as_ops(rng, e) for _ in range(4)]
    ops = (np.stack([x[0] for x in enc]), np.stack([x[1] for x in enc]))
    same = np.stack([DC.carry("edges", e, case["len_edges"][0], "ops", x) for x in enc])
    got = treeset.distances(ops, ALL, lengths=same, squared=True)
    assert not treeset.compare(ops).rf.any()
    for key in ALL:
        assert not got[key].any()
    other = DC.random_lengths(rng, same.shape)
    got = treeset.distances(ops, ALL, lengths=other, squared=True)
    assert got["wrf"][np.triu_indices(4, 1)].min() > 0.0 and not got["path"].any()
    check(got, D.distances("ops", enc, other))


def test_unit_lengths_give_the_rf_matrix():
    case = DC.case(65, 33)
    ones = np.ones_like(case["len_edges"])
    got = treeset.distances(case["edges"], ("wrf", "kf"), lengths=ones, squared=True)
    rf = treeset.compare(case["edges"]).rf
    assert np.array_equal(got["wrf"], rf.astype(np.float64))
    assert np.array_equal(got["kf"], rf.astype(np.float64))


def test_compare_is_unchanged_by_a_distance_call():
    case = DC.case(130, 3)
    before = treeset.compare(case["edges"])
    run(case, "edges")
    treeset.split_lengths(case["edges"], lengths=case["len_edges"])
    after = treeset.compare(case["edges"])
    for key in ("edge_ids", "bits", "count", "rf"):
        assert np.array_equal(getattr(before, key), getattr(after, key))


def test_consensus_with_mean_lengths():
    case = DC.case(65, 33)
    ref = case["ref"]
    r, split_mean, tip_mean = treeset.split_lengths(case["edges"], lengths=case["len_edges"])
    plain = treeset.consensus(r)
    cons = treeset.consensus(r, lengths=(split_mean, tip_mean))
    strip = treeset.consensus(r, lengths=(split_mean, tip_mean))
    for node in strip.seed_node.postorder():
        node.length = None
    assert strip.as_newick() == plain.as_newick()
    want = {s: x / c for s, x, c in zip(ref["U"], ref["split_sum"], ref["count"])}
    below, seen = {}, 0
    for node in cons.seed_node.postorder():
        below[node] = (1 << int(node.label)) if node.is_leaf() else 0
        for c in node.children:
            below[node] |= below[c]
        if node is cons.seed_node:
            assert node.length is None
        elif node.is_leaf():
            assert node.length == ref["tip_sum"][int(node.label)] / 33.0
        else:
            assert node.length == want[below[node]]
            seen += 1
    assert seen == sum(1 for c in ref["count"] if c > 16.5) > 0


def test_bootstrap_replicates_end_to_end():
    """The replicates of TreeModel.bootstrap_nj carry no lengths: with every length 1 their
    weighted RF is their RF, and the consensus carries the unit means."""
    from test_gpu_treeset_model import model
    tm, _, names = model()
    tree, support, n_ok, reps = tm.bootstrap_nj(12, seed=4, return_replicates=True)
    assert n_ok == 12
    joins, roots = reps
    n = joins.shape[1] + 2
    ones = np.ones((12, 2 * n - 3))
    got = treeset.distances(reps, ("wrf", "path"), names=names, lengths=ones, form="joins")
    r, split_mean, tip_mean = treeset.split_lengths(reps, names=names, lengths=ones, form="joins")
    assert np.array_equal(got["wrf"], treeset.compare(reps, form="joins").rf.astype(np.float64))
    assert (got["path"][got["wrf"] > 0] > 0).all()
    assert (split_mean == 1.0).all() and (tip_mean == 1.0).all()
    cons = treeset.consensus(r, lengths=(split_mean, tip_mean))
    assert all(x.length == 1.0 for x in cons.seed_node.postorder() if x is not cons.seed_node)
    # the model's tree (the NJ tree with its lengths) against itself and against the consensus
    for metric in ALL:
        assert tm.tree_distance(tree.as_newick(), metric) == 0.0
    d = treeset.distances([tree, cons], "kf", names)
    assert tm.tree_distance(cons, "kf") == d[0, 1] > 0.0


def test_profile_times():
    case = DC.case(64, 2)
    treeset.distance_profile(True)
    try:
        run(case, "edges")
        ms = treeset.distance_kernel_ms()
    finally:
        treeset.distance_profile(False)
    assert len(ms) == 5 and all(np.isfinite(x) and x >= 0.0 for x in ms)
    with pytest.raises(N.PhyloHipError):
        treeset.distance_kernel_ms()
