"""Parsimony SPR on the device (pu_parsimony.hip) against the numpy restatement
(tests/parsimony_spr_reference.py), whose score of a move is brute force: the move applied and
the new tree scored from scratch.  Every result is an integer and every comparison is exact
equality -- the score matrix with its sentinel, the lengths, the search's edges, rounds and
moves, chunking, the argument refusals and the way through TreeModel."""
import functools

import numpy as np
import pytest

import parsimony_reference as PR
import parsimony_spr_reference as SR
from phylo_utils_amd import _native as N
from phylo_utils_amd import parsimony
from test_gpu_parsimony import model, names_of

pytestmark = pytest.mark.gpu

# (shape, P, weights, radius): every pattern count -- 1; a wave less one, a wave, one more; a
# tile less one, a tile, one more; three tiles -- every radius and every kind of weights
COMBOS = (("random", 1, "none", 0), ("caterpillar", 63, "big", 1), ("balanced", 64, "ones", 2),
          ("random", 65, "big", 3), ("caterpillar", 255, "none", 0), ("balanced", 256, "big", 0),
          ("random", 257, "big", 2), ("balanced", 600, "big", 0), ("caterpillar", 600, "none", 1))


@functools.lru_cache(maxsize=None)
def alignment(n, P, K):
    """(codes, table, sets) with the full-set gap code and partial ambiguities; at K = 32 the 32
    codes are states 3 .. 31 (the top mask bit among them), the full set and two subsets."""
    rng = np.random.default_rng(11 * n + 17 * P + K)
    if K < 32:
        codes, table = PR.random_alignment(rng, n, P, K, ambiguity=0.1)
    else:
        table = np.zeros((32, 32))
        table[np.arange(29), np.arange(3, 32)] = 1.0
        table[29] = 1.0
        table[30, [0, 31]] = 1.0
        table[31, [1, 2, 30, 31]] = 1.0
        base = rng.integers(25, 29, size=P)  # states 28 .. 31
        codes = np.where(rng.random((n, P)) < 0.35, rng.integers(20, 29, size=(n, P)), base[None])
        codes = np.where(rng.random((n, P)) < 0.1, rng.integers(29, 32, size=(n, P)), codes)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
    codes.setflags(write=False)
    return codes, table, PR.tip_sets(codes, table)


@functools.lru_cache(maxsize=None)
def weights(kind, n, P):
    """None; all ones; integers with zeros and values near 2^40."""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(P, dtype=np.int64)
    w = np.random.default_rng(P + n).integers(0, 6, size=P).astype(np.int64)
    w[P // 2] = 2 ** 40 - 1
    if P > 2:
        w[0], w[-1] = 0, 2 ** 40 + 3
    return w


@functools.lru_cache(maxsize=None)
def tree(n, shape):
    """An edge list int32 [2n-3][2]: a schedule of parsimony_reference as its edges, or a random
    tree after one SPR move (so that the edge ids are in no creation order)."""
    if shape == "caterpillar":
        edges = PR.schedule_edges(*PR.caterpillar_schedule(n))
    elif shape == "balanced":
        edges = PR.schedule_edges(*PR.balanced_schedule(n))
    else:
        edges = PR.random_edges(np.random.default_rng(n), n)
        for d in SR.valid_directions(edges)[::-1]:
            tg = SR.targets(edges, d)
            if tg:
                edges = SR.apply_spr_edges(edges, d, max(tg))
                break
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    edges.setflags(write=False)
    return edges


@functools.lru_cache(maxsize=None)
def expected(n, shape, P, K, kind, radius, brute=True):
    """(L, object matrix [2E][E]) by brute force; by the rule's formula (itself held to brute
    force in test_parsimony_spr.py) only for the 40-taxon caterpillar, where brute force would
    take most of a minute."""
    S = alignment(n, P, K)[2]
    fn = SR.brute_scores if brute else SR.formula_scores
    L, sc = fn(tree(n, shape), S, weights(kind, n, P), radius)
    return L, SR.score_matrix(tree(n, shape), sc)


def same(scores, want):
    return scores.dtype == np.uint64 and scores.shape == want.shape and \
        np.array_equal(scores.astype(object), want)


@pytest.mark.parametrize("K", [2, 4, 20, 32])
@pytest.mark.parametrize("n", [3, 4, 5, 6, 9, 17])
def test_spr_scores(n, K):
    for shape, P, kind, radius in COMBOS:
        codes, table, _ = alignment(n, P, K)
        aln = (codes, table, names_of(n))
        w = weights(kind, n, P)
        edges = tree(n, shape)
        L, want = expected(n, shape, P, K, kind, radius)
        gotL, got = parsimony.spr_scores(aln, edges, weights=w, radius=radius)
        assert isinstance(gotL, int) and gotL == L, (shape, P, kind, radius)
        assert same(got, want), (shape, P, kind, radius)
        assert gotL == parsimony.fitch_lengths(aln, PR.edges_schedule(edges, n)[:2], weights=w)
        # the sentinel sits exactly on what is no (valid direction, target) pair
        for d in range(2 * len(edges)):
            tg = SR.targets(edges, d, radius)
            assert set(np.flatnonzero(got[d] != parsimony.SENTINEL)) == set(tg), (d, radius)
        if n == 4:  # pruning a pair of tips leaves two tips: a valid direction without a target
            assert any(not SR.targets(edges, d, radius) for d in SR.valid_directions(edges))


@pytest.mark.parametrize("K", [4, 20])
def test_spr_scores_batch(K):
    """Three different trees in one call are three single calls."""
    n, P = 9, 257
    codes, table, _ = alignment(n, P, K)
    aln = (codes, table, names_of(n))
    w = weights("big", n, P)
    batch = np.stack([tree(n, s) for s in ("random", "caterpillar", "balanced")])
    for radius in (None, 2):
        L, sc = parsimony.spr_scores(aln, batch, weights=w, radius=radius)
        assert L.dtype == np.uint64 and sc.shape == (3, 30, 15)
        for t, shape in enumerate(("random", "caterpillar", "balanced")):
            eL, want = expected(n, shape, P, K, "big", radius or 0)
            oneL, one = parsimony.spr_scores(aln, batch[t], weights=w, radius=radius)
            assert int(L[t]) == oneL == eL
            assert np.array_equal(sc[t], one) and same(one, want)


def test_spr_scores_deep_walk(monkeypatch):
    """A 40-taxon caterpillar: walks 37 arriving sets deep, in LDS and (PU_PARS_LDS) in the
    workspace."""
    n, P, K = 40, 65, 4
    codes, table, _ = alignment(n, P, K)
    aln = (codes, table, names_of(n))
    w = weights("big", n, P)
    L, want = expected(n, "caterpillar", P, K, "big", 0, False)
    monkeypatch.delenv("PU_PARS_LDS", raising=False)
    gotL, got = parsimony.spr_scores(aln, tree(n, "caterpillar"), weights=w)
    assert gotL == L and same(got, want)
    monkeypatch.setenv("PU_PARS_LDS", "1")
    againL, again = parsimony.spr_scores(aln, tree(n, "caterpillar"), weights=w)
    assert againL == L and np.array_equal(again, got)


@functools.lru_cache(maxsize=None)
def search_case(n, K=4):
    """Stepwise-addition starts (a batch of 4) and the restatement's search from each."""
    codes, table, w, orders = PR.stepwise_case(n, K)
    S = PR.tip_sets(codes, table)
    starts = np.stack([PR.stepwise(S, o, w)["edges"] for o in orders[2:6]])
    return codes, table, w, S, starts, [SR.search(e, S, w, max_rounds=50) for e in starts]


def all_outputs(n, K):
    P = 600
    codes, table, _ = alignment(n, P, K)
    aln = (codes, table, names_of(n))
    w = weights("big", n, P)
    batch = np.stack([tree(n, s) for s in ("random", "caterpillar", "balanced")])
    sc, st, sw, _, starts, _ = search_case(n)
    out = list(parsimony.spr_scores(aln, batch, weights=w)) \
        + list(parsimony.spr_scores(aln, batch, radius=2))
    for res in (parsimony.spr_search(aln, batch, weights=w, max_rounds=3, return_moves=True),
                parsimony.spr_search((sc, st, names_of(n)), starts, weights=sw)):
        out += list(res[:3]) + [np.concatenate(m) for m in res[3:]]
    return out


@pytest.mark.parametrize("n,K", [(17, 4), (17, 20)])
def test_chunking_changes_nothing(n, K, monkeypatch):
    """PU_PARS_CHUNK=1 (one tree per chunk), a small PU_PARS_WS (direction and pattern chunks,
    and one row of workspace stack per launch) and PU_PARS_LDS (the arriving sets in the
    workspace, not in LDS) are read at each call and change no bit."""
    for name in ("PU_PARS_CHUNK", "PU_PARS_WS", "PU_PARS_LDS"):
        monkeypatch.delenv(name, raising=False)
    plain = all_outputs(n, K)
    for chunk, ws, lds in (("1", None, None), (None, "4096", None), (None, None, "1"),
                           ("1", "4096", "1"), ("2", "20000", "1")):
        for name, v in (("PU_PARS_CHUNK", chunk), ("PU_PARS_WS", ws), ("PU_PARS_LDS", lds)):
            if v:
                monkeypatch.setenv(name, v)
            else:
                monkeypatch.delenv(name, raising=False)
        got = all_outputs(n, K)
        assert len(got) == len(plain)
        assert all(np.array_equal(a, b) for a, b in zip(plain, got)), (chunk, ws, lds)


@pytest.mark.parametrize("n", [9, 17])
def test_spr_search(n):
    codes, table, w, S, starts, ref = search_case(n)
    aln = (codes, table, names_of(n))
    dev_starts = parsimony.stepwise_addition(aln, orders=PR.stepwise_case(n, 4)[3][2:6],
                                             weights=w)[0]
    assert np.array_equal(dev_starts, starts)
    assert any(r["rounds"] > 0 for r in ref)
    edges, lengths, rounds, moves = parsimony.spr_search(aln, starts, weights=w, max_rounds=50,
                                                         return_moves=True)
    assert edges.shape == starts.shape and lengths.dtype == np.uint64
    for t, want in enumerate(ref):
        assert np.array_equal(edges[t], want["edges"]), t
        assert int(lengths[t]) == want["length"] and int(rounds[t]) == want["rounds"] < 50, t
        assert [tuple(int(v) for v in m) for m in moves[t]] == want["moves"], t
        # each reported length is the device's own length of the tree after that move
        cur = starts[t]
        for d, f, L in moves[t]:
            cur = parsimony.apply_spr_edges(cur, int(d), int(f))
            assert parsimony.fitch_lengths(aln, PR.edges_schedule(cur, n)[:2], weights=w) == int(L)
        assert np.array_equal(cur, edges[t])
        assert int(lengths[t]) <= PR.lengths(starts[t], S, w)
    # without a limit and without the moves: the same trees; one tree alone: its row
    e0, l0, r0 = parsimony.spr_search(aln, starts, weights=w)
    assert np.array_equal(e0, edges) and np.array_equal(l0, lengths) and np.array_equal(r0, rounds)
    t = int(np.argmax(rounds))
    one = parsimony.spr_search(aln, starts[t], weights=w)
    assert np.array_equal(one[0], edges[t]) and one[1:] == (int(lengths[t]), int(rounds[t]))
    # max_rounds = 1 stops after one round
    e1, l1, r1, m1 = parsimony.spr_search(aln, starts, weights=w, max_rounds=1, return_moves=True)
    for i, want in enumerate(ref):
        assert int(r1[i]) == min(1, want["rounds"])
        assert [tuple(int(v) for v in m) for m in m1[i]] == want["moves"][:1]
        assert int(l1[i]) == (want["moves"][0][2] if want["moves"] else want["length"])
    # a local optimum: 0 rounds, edges unchanged
    e2, l2, r2 = parsimony.spr_search(aln, edges, weights=w)
    assert np.array_equal(e2, edges) and np.array_equal(l2, lengths) and not r2.any()
    # a radius: the restatement's search under the same radius
    er, lr, rr = parsimony.spr_search(aln, starts[t], weights=w, radius=2)
    want = SR.search(starts[t], S, w, radius=2)
    assert np.array_equal(er, want["edges"]) and (lr, rr) == (want["length"], want["rounds"])


def test_three_taxa_have_no_move():
    codes, table, S = alignment(3, 65, 4)
    aln = (codes, table, names_of(3))
    edges = tree(3, "caterpillar")
    L, sc = parsimony.spr_scores(aln, edges)
    assert L == PR.lengths(edges, S) and sc.shape == (6, 3) and (sc == parsimony.SENTINEL).all()
    e, l, r = parsimony.spr_search(aln, edges)
    assert np.array_equal(e, edges) and (l, r) == (L, 0)


def test_treemodel_spr_refinement():
    tm = model()
    codes, table, names = tm._coded_alignment()
    plain_tree, plain_len, plain_all = tm.set_parsimony_tree(n_rep=5, seed=3)
    newick = plain_tree.as_newick()
    tree_spr, length, all_lengths = tm.set_parsimony_tree(n_rep=5, seed=3, spr_rounds=0)
    assert length <= plain_len and all(int(a) <= int(b) for a, b in zip(all_lengths, plain_all))
    assert tm.parsimony_length() == length == int(min(all_lengths))
    # the restatement: every replicate refined, the shortest kept, ties to the lowest replicate
    w = np.asarray(tm.siteweights).astype(np.int64)
    S = PR.tip_sets(codes, table)
    runs = [SR.search(PR.stepwise(S, o, w)["edges"], S, w)
            for o in parsimony.random_orders(len(names), 5, 3)]
    assert [int(x) for x in all_lengths] == [r["length"] for r in runs]
    best = runs[[r["length"] for r in runs].index(length)]
    assert np.array_equal(parsimony.tree_schedule(tree_spr, names)[0], parsimony.tree_schedule(
        parsimony.edges_to_tree(best["edges"], names), names)[0])
    # one round at radius 1 lies between the two
    _, one, _ = tm.set_parsimony_tree(n_rep=5, seed=3, spr_rounds=1, spr_radius=1)
    assert length <= one <= plain_len
    # the default call is what it was
    again, again_len, _ = tm.set_parsimony_tree(n_rep=5, seed=3)
    assert again.as_newick() == newick and again_len == plain_len


def test_refusals_leave_the_device_usable():
    n, P, K = 5, 65, 4
    codes, table, S = alignment(n, P, K)
    names = names_of(n)
    aln = (codes, table, names)
    good = tree(n, "random")

    def bad(g, j, v):
        e = good.copy()
        e[g, j] = v
        return e

    bad_codes = codes.copy()
    bad_codes[2, 7] = len(table)
    zero_row = table.copy()
    zero_row[K + 1] = 0.0
    neg = np.ones(P, dtype=np.int64)
    neg[3] = -1
    (g0, j0), (g1, j1) = np.argwhere(good < n)[:2]
    two_trees = bad(g0, j0, int(good[g1, j1]))  # one tip on two edges, another on none
    cycle = np.array([[0, 5], [1, 5], [2, 6], [6, 7], [7, 6], [3, 7], [4, 5]], dtype=np.int32)
    moves = np.zeros((1, 1, 3), dtype=np.uint64)
    lens, rounds = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)

    def raw_search(edges, radius, max_rounds, mv):
        e = np.ascontiguousarray(edges, dtype=np.int32).copy()
        N.check(N.lib().pu_parsimony_spr(0, n, P, table.shape[0], K, N.ptr(codes), N.ptr(table),
                                         None, 1, N.ptr(e), radius, max_rounds, N.ptr(lens),
                                         N.ptr(rounds), N.ptr(mv)), None, "pu_parsimony_spr")

    calls = []
    for fn in (parsimony.spr_scores, parsimony.spr_search):
        calls += [
            # what pu_fitch_lengths refuses
            lambda fn=fn: fn((codes[:2], table, names[:2]), np.zeros((1, 2), np.int32)),
            lambda fn=fn: fn((codes[:, :0], table, names), good),
            lambda fn=fn: fn((bad_codes, table, names), good),
            lambda fn=fn: fn((codes, zero_row, names), good),
            lambda fn=fn: fn((np.zeros_like(codes), np.ones((1, 33)), names), good),
            lambda fn=fn: fn(aln, good, weights=neg),
            # edge lists that are no binary tree over the rows
            lambda fn=fn: fn(aln, bad(2, 1, 2 * n - 2)),
            lambda fn=fn: fn(aln, bad(2, 1, -1)),
            lambda fn=fn: fn(aln, bad(3, 0, int(good[3, 1]))),  # a loop edge
            lambda fn=fn: fn(aln, two_trees),
            lambda fn=fn: fn(aln, cycle),
            lambda fn=fn: fn(aln, np.stack([good, two_trees])),
            lambda fn=fn: fn(aln, good, radius=-1),
        ]
    calls += [
        lambda: parsimony.spr_search(aln, good, max_rounds=-1),
        lambda: raw_search(good, 0, 0, moves),  # moves_out without max_rounds
        lambda: raw_search(good, -1, 1, moves),
    ]
    want = SR.score_matrix(good, SR.brute_scores(good, S)[1])
    for i, call in enumerate(calls):
        with pytest.raises(N.PhyloHipError) as err:
            call()
        assert "(-1)" in str(err.value), (i, str(err.value))
        assert same(parsimony.spr_scores(aln, good)[1], want), i
    with pytest.raises(ValueError):
        parsimony.spr_search(aln, good, return_moves=True)  # needs max_rounds > 0
    raw_search(good, 0, 1, moves)  # the same call with its rows is fine
