"""DESIGN 4.26 on the host: the rule's score formula against brute force (every neighbour tree
scored from scratch), the move on edge lists, the count of directions, the radius and the
search's fixed point (tests/parsimony_spr_reference.py), and the package's apply_spr_edges."""
import functools

import numpy as np
import pytest

import parsimony_reference as PR
import parsimony_spr_reference as SR
from phylo_utils_amd import parsimony

TAXA = (4, 5, 6, 9)


@functools.lru_cache(maxsize=None)
def case(n, K):
    """(edges, sets, integer weights with zeros) with ambiguity codes."""
    rng = np.random.default_rng(100 * K + n)
    codes, table = PR.random_alignment(rng, n, 41, K, ambiguity=0.15)
    w = rng.integers(0, 5, size=41).astype(np.int64)
    return PR.random_edges(rng, n), PR.tip_sets(codes, table), w


@pytest.mark.parametrize("K", [4, 20])
@pytest.mark.parametrize("n", TAXA)
def test_formula_is_brute_force(n, K):
    edges, S, w = case(n, K)
    for ww in (w, None):
        for radius in (0, 1, 2):
            assert SR.formula_scores(edges, S, ww, radius) == SR.brute_scores(edges, S, ww, radius)
    # the formula on a tree after a move, too (edge ids no longer in creation order)
    d = SR.valid_directions(edges)[-1]
    for f in SR.targets(edges, d):
        moved = SR.apply_spr_edges(edges, d, f)
        assert SR.formula_scores(moved, S, w) == SR.brute_scores(moved, S, w)
        break


def test_formula_is_brute_force_on_a_deep_walk():
    """A 17-taxon caterpillar, the shape whose 40-taxon form the device test holds to the formula:
    walks 14 arriving sets deep."""
    n = 17
    rng = np.random.default_rng(n)
    codes, table = PR.random_alignment(rng, n, 29, 4, ambiguity=0.15)
    S = PR.tip_sets(codes, table)
    w = rng.integers(0, 5, size=29).astype(np.int64)
    edges = PR.schedule_edges(*PR.caterpillar_schedule(n))
    for radius in (0, 3):
        assert SR.formula_scores(edges, S, w, radius) == SR.brute_scores(edges, S, w, radius)


@pytest.mark.parametrize("n", (3,) + TAXA)
def test_directions_and_moves(n):
    rng = np.random.default_rng(n)
    edges = PR.random_edges(rng, n)
    names = ["t%d" % i for i in range(n)]
    valid = SR.valid_directions(edges)
    assert len(valid) == 3 * n - 6
    base = SR.splits(edges)
    n_moves = 0
    for d in range(2 * len(edges)):
        tg = SR.targets(edges, d) if d in valid else {}
        m = SR.direction(edges, d)
        if m is not None:  # every edge of T' but the merged one, none of them vacant
            assert set(tg) == set(SR.rest_tree(edges, d)) - {m["ea"]}
            assert not {m["e"], m["eb"]} & set(tg)
        for f in range(len(edges)):
            if f not in tg:
                if m is None or f in (m["e"], m["ea"], m["eb"]):
                    with pytest.raises(ValueError):
                        parsimony.apply_spr_edges(edges, d, f)
                continue
            moved = SR.apply_spr_edges(edges, d, f)
            assert np.array_equal(parsimony.apply_spr_edges(edges, d, f), moved)
            # edges_to_tree refuses what is no connected binary tree over the tips
            tree = parsimony.edges_to_tree(moved, names)
            assert len(parsimony.tree_schedule(tree, names)[0]) == n - 2
            assert tuple(moved[m["e"]]) == tuple(int(v) for v in edges[m["e"]])
            assert len(SR.splits(moved)) == n - 3
            n_moves += 1
    if n == 3:
        assert n_moves == 0 and base == frozenset()


@pytest.mark.parametrize("n", TAXA)
def test_radius_one_is_nni(n):
    edges = PR.random_edges(np.random.default_rng(50 + n), n)
    got = set()
    for d in SR.valid_directions(edges):
        tg = SR.targets(edges, d, 1)
        assert all(k == 1 for k in tg.values())
        assert tg == {f: k for f, k in SR.targets(edges, d).items() if k == 1}
        got |= {SR.splits(SR.apply_spr_edges(edges, d, f)) for f in tg}
    want = SR.nni_neighbours(edges)
    assert len(want) == 2 * (n - 3) == len(set(want))
    assert got == set(want) and SR.splits(edges) not in got


@pytest.mark.parametrize("n,K", [(6, 4), (9, 4), (9, 20)])
def test_search_ends_on_a_local_optimum(n, K):
    edges, S, w = case(n, K)
    start = PR.lengths(edges, S, w)
    res = SR.search(edges, S, w)
    assert res["length"] == PR.lengths(res["edges"], S, w) <= start
    assert [m[2] for m in res["moves"]] == sorted({m[2] for m in res["moves"]}, reverse=True)
    L, sc = SR.brute_scores(res["edges"], S, w)
    assert L == res["length"] and min(sc.values()) >= L
    # the formula drives the same search, and max_rounds cuts it
    assert SR.search(edges, S, w, scores=SR.formula_scores)["moves"] == res["moves"]
    if res["rounds"]:
        one = SR.search(edges, S, w, max_rounds=1)
        assert one["rounds"] == 1 and one["moves"] == res["moves"][:1]
        t = edges
        for d, f, L in res["moves"]:
            t = SR.apply_spr_edges(t, d, f)
            assert PR.lengths(t, S, w) == L
        assert np.array_equal(t, res["edges"])
