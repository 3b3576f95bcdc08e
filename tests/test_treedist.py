"""The tree-distance rule without a device: the restatement against its own second
statement, the metric axioms, every refusal, and ``consensus`` with and without lengths."""
import math

import numpy as np
import pytest

import treedist_cases as DC
import treedist_reference as D
import treeset_cases as C
import treeset_reference as TR
from phylo_utils_amd import _native as N
from phylo_utils_amd import treeset

U53 = 2.0 ** -53


@pytest.mark.parametrize("n,T", [(3, 2), (4, 3), (5, 4), (9, 5), (33, 4), (66, 3)])
def test_the_two_statements_agree(n, T):
    """Integers exactly.  fp64 within the bound of the arithmetic, u = 2^-53, to first order with
    a factor 2 for the higher orders (every count here is far below 1/u):
    * a serial sum of m non-negative terms is within (m - 1) u of its exact sum, relatively;
    * p has at most e path edges, so |p - exact| <= (e - 1) u p, and fsum's own rounding adds u;
    * wRF: 2n - 3 + (n - 3) keys at the most, each term |la - lb| rounded once (u), summed
      serially: (keys) u wRF;
    * KF2: each term has two more roundings (the difference, the square): (keys + 2) u KF2;
    * WPath2: d = pa - pb carries |pa| ea u + |pb| eb u + u |d|, so d^2 is within
      2 |d| (pa ea + pb eb) u + 3 u d^2; the segmented sum adds at most (2048 + segments) u."""
    case = DC.case(n, T)
    trees, L = DC.trees_of(case, "edges"), case["len_edges"]
    ref = case["ref"]
    keyed = [D.check_keyed("edges", t, x) for t, x in zip(trees, L)]
    paths = [D.check_paths("edges", t, x) for t, x in zip(trees, L)]
    own = [D.paths("edges", t, x) for t, x in zip(trees, L)]
    n_keys = 3 * n - 6
    for t in range(T):
        assert own[t][0] == paths[t][0]
        for e, p, q in zip(own[t][0], own[t][1], paths[t][1]):
            assert abs(p - q) <= 2 * e * U53 * q
    for a in range(T):
        for b in range(T):
            w, q = D.check_weighted(keyed[a], keyed[b])
            assert abs(ref["wrf"][a][b] - w) <= 2 * n_keys * U53 * w
            assert abs(ref["kf2"][a][b] - q) <= 2 * (n_keys + 2) * U53 * q
            assert ref["path2"][a][b] == sum((x - y) ** 2 for x, y in zip(paths[a][0], paths[b][0]))
            terms, slack = [], 0.0
            for ea, pa, eb, pb in zip(paths[a][0], paths[a][1], paths[b][0], paths[b][1]):
                d = pa - pb
                terms.append(d * d)
                slack += 2 * abs(d) * (pa * ea + pb * eb) * U53 + 3 * U53 * d * d
            exact = math.fsum(terms)
            m = len(terms)
            bound = 2 * (slack + (min(m, D.SEGMENT) + m // D.SEGMENT + 1) * U53 * exact)
            assert abs(ref["wpath2"][a][b] - exact) <= bound


@pytest.mark.parametrize("n,T", [(5, 4), (33, 4), (66, 3)])
def test_metric_axioms(n, T):
    case = DC.case(n, T)
    ref = case["ref"]
    for key in ("wrf", "kf2", "path2", "wpath2"):
        m = ref[key]
        for a in range(T):
            assert m[a][a] == 0
            for b in range(T):
                assert m[a][b] == m[b][a]
    # all lengths 1: wRF is RF
    trees = DC.trees_of(case, "edges")
    ones = np.ones((T, 2 * n - 3))
    unit = D.distances("edges", trees, ones, want=("wrf",))
    assert unit["wrf"] == [[float(x) for x in row] for row in case["ref_edges"]["rf"]]
    # one topology under other node numbers, root edges and op orders: Path2 = 0
    rng = np.random.default_rng(n)
    enc = [C.as_ops(rng, trees[0]) for _ in range(3)]
    same = D.distances("ops", enc, np.ones((3, 2 * n - 3)), want=("path2",))
    assert not np.array(same["path2"]).any()


def test_three_tips():
    """No split, three pendant keys, e = 2 for every pair."""
    case = DC.case(3, 2)
    e, p = D.paths("edges", case["edges"][0], case["len_edges"][0])
    assert e == [2, 2, 2] and case["ref"]["U"] == [] and case["ref"]["split_sum"] == []


def test_the_reference_keeps_the_segment_rule():
    """2080 pairs: one full segment and 32 more; a plain serial sum differs."""
    case = DC.case(65, 33)
    trees, L = DC.trees_of(case, "edges"), case["len_edges"]
    pa = D.paths("edges", trees[0], L[0])[1]
    pb = D.paths("edges", trees[1], L[1])[1]
    sq = [(x - y) * (x - y) for x, y in zip(pa, pb)]
    assert len(sq) == 2080
    head = tail = 0.0
    for v in sq[:2048]:
        head += v
    for v in sq[2048:]:
        tail += v
    assert D.wpath2_pair(pa, pb) == case["ref"]["wpath2"][0][1] == head + tail


NEWICKS = ["((a:1,b:2):0.5,(c:1,d:1):0.25,e:3);", "((a:1,c:2):0.5,(b:1,d:1):0.25,e:3);"]


def refused(fn, *args, **kw):
    with pytest.raises((ValueError, N.PhyloHipError)) as info:
        fn(*args, **kw)
    return str(info.value)


def test_python_refusals_need_no_device():
    case = DC.case(5, 4)
    e, L = case["edges"], case["len_edges"]
    assert "metric" in refused(treeset.distances, e, "rf", lengths=L)
    assert "metric" in refused(treeset.distances, e, (), lengths=L)
    assert "lengths" in refused(treeset.distances, e, "wrf")
    assert "lengths" in refused(treeset.distances, e, "wrf", lengths=L[:, :-1])
    assert "own lengths" in refused(treeset.distances, NEWICKS, "wrf", lengths=L[:2])
    for bad in (-1.0, np.nan, np.inf):
        x = L.copy()
        x[2, 3] = bad
        assert "tree 2 edge 3" in refused(treeset.distances, e, "kf", lengths=x)
        assert "tree 2 edge 3" in refused(treeset.split_lengths, e, lengths=x)
    assert "rows" in refused(treeset.distances, e, "wrf", lengths=L, rows=5)
    assert "rows" in refused(treeset.distances, e, "wrf", lengths=L, rows=-1)
    msg = refused(treeset.distances, [NEWICKS[0], "((a:1,c):0.5,(b:1,d:1):0.25,e:3);"], "wrf")
    assert "tree 1" in msg and "'c'" in msg and "no length" in msg
    msg = refused(treeset.distances, [NEWICKS[0], "((a:1,c:1),(b:1,d:1):0.25,e:3);"], "wrf")
    assert "tree 1" in msg and "internal" in msg


def test_entry_point_refusals_come_before_any_device():
    """pu_treedist with device = -1: an argument that is refused is refused first; only a call
    that passes every check gets as far as the device number."""
    case = DC.case(5, 4)
    ops, roots = case["ops"]
    L = np.ascontiguousarray(case["len_ops"])
    n, T = 5, 4
    out = np.zeros((T, T))

    def call(n=n, T=T, form=0, trees=ops, roots=roots, lengths=L, rows=T):
        rc = N.lib().pu_treedist(-1, n, T, form, N.ptr(trees), N.ptr(roots), N.ptr(lengths), rows,
                                 N.ptr(out), None, None, None, None, None, None)
        return rc, N.last_error() if hasattr(N, "last_error") else ""

    def message(**kw):
        with pytest.raises(N.PhyloHipError) as info:
            N.check(call(**kw)[0])
        return str(info.value)

    assert "lengths" in message(lengths=None)
    assert "n_rows" in message(rows=T + 1)
    assert "n_rows" in message(rows=-1)
    assert "form" in message(form=3)
    assert "null" in message(trees=None)
    assert "root" in message(roots=None)
    assert "n = 2" in message(n=2)
    assert "n_trees" in message(T=0)
    for bad in (-0.5, np.nan, -np.inf, np.inf):
        x = L.copy()
        x[1, 6] = bad
        assert "tree 1 edge 6" in message(lengths=x)
    twice = ops.copy()
    twice[3, 1, 1] = twice[3, 0, 1]  # a child used twice
    assert "tree 3" in message(trees=twice)
    assert "device" in message().lower()  # everything else passed


def test_consensus_without_lengths_is_unchanged():
    """``consensus(result)`` and ``consensus(result, lengths=None)`` write what they wrote before
    lengths existed: the reference's majority-rule tree, label for label, with no length."""
    for n, T in ((65, 33), (5, 17), (9, 5)):
        case = C.case(n, T)
        ref = case["ref_edges"]
        r = treeset.TreeSetResult(n, T, TR.bits_of(ref["U"], n), ref["count"])
        a, b = treeset.consensus(r), treeset.consensus(r, 0.5, None, None)
        assert a.as_newick() == b.as_newick() and ":" not in a.as_newick()
        U = len(ref["U"])
        split_mean, tip_mean = np.arange(1.0, U + 1.0), np.arange(1.0, n + 1.0) / 4.0
        c = treeset.consensus(r, lengths=(split_mean, tip_mean))
        for node in c.seed_node.postorder():
            if node is not c.seed_node:
                assert node.length is not None
                if node.is_leaf():
                    assert node.length == tip_mean[int(node.label)]
            node.length = None
        assert c.as_newick() == a.as_newick()
    with pytest.raises(ValueError):
        treeset.consensus(r, lengths=(split_mean[:-1], tip_mean))


def test_newick_lengths_in_op_order():
    """Tree and Newick input brings its own lengths into the ops form's edge order."""
    names = list("abcde")
    form, a, roots, _, pairs, L, n = treeset._batch_with_lengths(NEWICKS, names, None, None)
    assert form == "ops" and n == 5 and L.shape == (2, 7)
    ref = D.distances("ops", list(zip(a, roots)), L)
    # by hand: pendant keys a..e, splits {a,b}|.. and {c,d}|.. against {a,c}, {b,d}
    assert ref["wrf"][0][1] == 0 + 1 + 1 + 0 + 0 + 0.5 + 0.25 + 0.5 + 0.25
    assert ref["kf2"][0][1] == 1 + 1 + 2 * 0.25 + 2 * 0.0625
    assert ref["path2"][0][1] == sum((x - y) ** 2 for x, y in zip(
        [2, 4, 4, 3, 4, 4, 3, 2, 3, 3], [4, 2, 4, 3, 4, 2, 3, 4, 3, 3]))
