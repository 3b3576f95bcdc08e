"""Fitch parsimony without a device: the numpy restatement of the rule
(tests/parsimony_reference.py) against Sankoff's dynamic programme, the insertion identity, the
invariants of stepwise addition and the conditions the shared fixtures must meet to catch a wrong
tie rule, and the host pieces of phylo_utils_amd.parsimony and of the CLI."""
import functools

import numpy as np
import pytest

import parsimony_reference as PR
from phylo_utils_amd import parsimony, phy
from phylo_utils_amd.tree import Traversal, parse_newick, prepare_tree


def case(seed, n, P, K):
    rng = np.random.default_rng(seed)
    codes, table = PR.random_alignment(rng, n, P, K, ambiguity=0.15)
    w = rng.integers(0, 5, size=P).astype(np.int64)
    return rng, codes, table, w


@pytest.mark.parametrize("K", [2, 4, 20])
def test_fitch_equals_sankoff(K):
    for n in range(3, 13):
        rng, codes, table, w = case(17 * K + n, n, 29, K)
        assert (codes[:, 0] == K).all()  # an all-gap column
        assert (codes > K).any()  # ambiguity codes
        S = PR.tip_sets(codes, table)
        allowed = table[codes] > 0
        for _ in range(3):
            edges = PR.random_edges(rng, n)
            for weights in (None, w):
                assert PR.lengths(edges, S, weights) == PR.sankoff_length(edges, allowed, weights)


def test_length_does_not_depend_on_the_root_edge():
    rng, codes, table, w = case(5, 11, 41, 4)
    S = PR.tip_sets(codes, table)
    edges = PR.random_edges(rng, 11)
    ch = [PR.pattern_changes(edges, S, e) for e in range(len(edges))]
    assert all(np.array_equal(c, ch[0]) for c in ch)
    assert len({PR.lengths(edges, S, w, e) for e in range(len(edges))}) == 1


@pytest.mark.parametrize("K", [4, 20])
def test_insertion_identity(K):
    """insertion_lengths(T, x)[e] is the length of T with x attached on e, scored from scratch
    (by Fitch and by Sankoff)."""
    for n in (4, 5, 9):
        rng, codes, table, w = case(31 * K + n, n, 33, K)
        S = PR.tip_sets(codes, table)
        allowed = table[codes] > 0
        edges = PR.random_edges(rng, n - 1)  # over rows 0..n-2; row n-1 is the query
        edges = [(u if u < n - 1 else u + 1, v if v < n - 1 else v + 1) for u, v in edges]
        got = PR.insertion_lengths(edges, S, [S[n - 1]], w)[0]
        for e in range(len(edges)):
            built = PR.attach(edges, e, n - 1, 2 * n - 3)
            assert got[e] == PR.lengths(built, S, w) == PR.sankoff_length(built, allowed, w)


@functools.lru_cache(maxsize=None)
def stepwise_runs(n):
    codes, table, w, orders = PR.stepwise_case(n)
    S = PR.tip_sets(codes, table)
    return S, w, orders, [PR.stepwise(S, o, w) for o in orders]


@pytest.mark.parametrize("n", PR.STEP_TAXA)
def test_stepwise_invariants(n):
    S, w, orders, runs = stepwise_runs(n)
    for o, r in zip(orders, runs):
        edges = r["edges"]
        assert edges.shape == (2 * n - 3, 2)
        deg = np.bincount(edges.ravel(), minlength=2 * n - 2)
        assert np.array_equal(deg, [1] * n + [3] * (n - 2))
        parsimony.edges_to_tree(edges, ["t%d" % i for i in range(n)])  # connected: no error
        steps = r["step_lengths"]
        assert len(steps) == n - 2 and all(a <= b for a, b in zip(steps, steps[1:]))
        assert steps[-1] == r["length"] == PR.lengths(edges, S, w)
        assert tuple(edges[0]) [0] == o[0]


def test_fixtures_can_catch_a_wrong_tie_rule():
    tied = chosen_not_first = 0
    for n in PR.STEP_TAXA:
        for r in stepwise_runs(n)[3]:
            tied += sum(t >= 2 for t in r["tied"])
            chosen_not_first += sum(c != 0 for c in r["chosen"])
    assert tied >= 1 and chosen_not_first >= 1
    # the rule itself: among tied edges the lowest id wins
    S, w, orders, runs = stepwise_runs(5)
    for o, r in zip(orders, runs):
        edges = [(int(o[0]), 5), (int(o[1]), 5), (int(o[2]), 5)]
        for k, e in zip(range(3, 5), r["chosen"]):
            cand = PR.insertion_lengths(edges, S, [S[o[k]]], w)[0]
            assert e == min(i for i, c in enumerate(cand) if c == min(cand))
            edges = PR.attach(edges, e, int(o[k]), 5 + k - 2)


def test_state_masks():
    table = np.array([[1, 0, 0, 0], [0, 0.5, 0, 0], [1, 1, 1, 1], [0, 1, 0, 1]], dtype=float)
    m = parsimony.state_masks(table)
    assert m.dtype == np.uint8 and m.tolist() == [1, 2, 15, 10]
    assert np.array_equal(m, PR.masks_of(table))
    wide = parsimony.state_masks(np.eye(20))
    assert wide.dtype == np.uint32 and wide[19] == 1 << 19
    with pytest.raises(ValueError):
        parsimony.state_masks(np.array([[1.0, 0.0], [0.0, 0.0]]))
    with pytest.raises(ValueError):
        parsimony.state_masks(np.eye(33))


def test_random_orders_are_deterministic():
    a, b = parsimony.random_orders(17, 5, 3), parsimony.random_orders(17, 5, 3)
    assert a.dtype == np.int32 and a.shape == (5, 17) and np.array_equal(a, b)
    assert all(sorted(r) == list(range(17)) for r in a)
    assert len({tuple(r) for r in a}) == 5
    assert not np.array_equal(a, parsimony.random_orders(17, 5, 4))
    rng = np.random.default_rng(3)
    assert np.array_equal(a[0], rng.permutation(17)) and np.array_equal(a[1], rng.permutation(17))
    # a longer batch starts with the shorter one
    assert np.array_equal(parsimony.random_orders(17, 7, 3)[:5], a)


def test_edges_to_tree_newick_round_trip():
    n = 9
    rng = np.random.default_rng(2)
    edges = PR.random_edges(rng, n)
    names = ["t%d" % i for i in range(n)]
    lens = np.arange(1, 2 * n - 2) / 8.0
    tree = parsimony.edges_to_tree(edges, names, lens)
    assert len(tree.seed_node.children) == 3
    again = parse_newick(tree.as_newick())
    assert again.as_newick() == tree.as_newick()
    # the same splits and lengths as the edge list
    tr = Traversal(prepare_tree(again))
    assert sorted(tr.names) == sorted(names) and tr.n_nodes == 2 * n - 2
    assert sorted(tr.brlens.values()) == sorted(lens.tolist())
    ops, root, pairs = parsimony.tree_schedule(again, names)
    S = PR.tip_sets(*PR.random_alignment(rng, n, 21, 4))
    assert PR.lengths(PR.schedule_edges(ops, root), S) == PR.lengths(edges, S)
    with pytest.raises(ValueError):
        parsimony.edges_to_tree(edges[:-1], names)
    with pytest.raises(ValueError):
        parsimony.tree_schedule(again, names[:-1] + ["other"])


def test_integral_weights_only():
    assert parsimony.integer_weights(None, 3) is None
    w = parsimony.integer_weights(np.array([1.0, 0.0, 7.0]), 3)
    assert w.dtype == np.int64 and w.tolist() == [1, 0, 7]
    with pytest.raises(ValueError):
        parsimony.integer_weights(np.array([1.0, 0.5, 7.0]), 3)
    with pytest.raises(ValueError):
        parsimony.integer_weights(np.array([1.0, np.nan, 7.0]), 3)
    with pytest.raises(ValueError):
        parsimony.integer_weights(np.array([1, 2]), 3)


def test_cli_argument_exclusions(tmp_path):
    aln, tree = tmp_path / "a.fasta", tmp_path / "t.nwk"
    aln.write_text(">a\nAC\n>b\nAC\n>c\nAG\n")
    tree.write_text("(a,b,c);\n")
    base = ["-s", str(aln), "-m", "JC"]
    phy.validate_args(phy.parse_cli(base + ["--parsimony"]))
    assert phy.parse_cli(base + ["--parsimony"]).parsimony == 1
    assert phy.parse_cli(base + ["--parsimony", "7"]).parsimony == 7
    phy.validate_args(phy.parse_cli(base + ["-t", str(tree), "--parsimony-score"]))
    for extra in (["-t", str(tree), "--parsimony"], ["--nj", "nj", "--parsimony", "2"],
                  ["--parsimony", "--distances"], ["--parsimony", "0"]):
        with pytest.raises(ValueError):
            phy.validate_args(phy.parse_cli(base + extra))
        assert phy.main(base + extra) == 1
    with pytest.raises(ValueError):  # no tree at all
        phy.validate_args(phy.parse_cli(base + ["--parsimony-score"]))
