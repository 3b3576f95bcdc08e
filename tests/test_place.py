"""Phylogenetic placement on the CPU: the restatement the device tests compare
against (tests/place_reference.py) pinned to the oracle's lnL of the joined (N+1)-taxon tree,
the host helpers of phylo_utils_amd.place, and the planted queries the device test relies on."""
import json
import re

import numpy as np
import pytest

import place_reference as R

from phylo_utils_amd import place as PL
from phylo_utils_amd.tree import Traversal, parse_newick, prepare_tree

_CACHE = {}


def restated(orc, case):
    if case not in _CACHE:
        _CACHE[case] = R.Restated(orc, R.problem(case))
    return _CACHE[case]


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_against_the_joined_tree(case, oracle_mod):
    """lnl_at(q, e, l) equals tree_lnl of the attached tree to 1e-11 |lnL|: every edge of the
    small cases, 6 sampled edges of the caterpillar; every query (the first, a noisy one and
    the all-gap one of the 65-query case); at the lower bound, 0.07 and 1.3."""
    r = restated(oracle_mod, case)
    E, Q = len(r.edges), len(r.z)
    edges = range(E) if E <= 25 else [0, 1, 2, E // 2, E - 2, E - 1]
    queries = range(Q) if Q <= 9 else [0, 7, Q - 1]
    worst = 0.0
    for k in edges:
        for q in queries:
            for l in (R.LO, 0.07, 1.3):
                a, b = r.lnl_at(q, k, l), r.joined_lnl(q, k, l)
                worst = max(worst, abs(a - b) / abs(b))
    print("%s: restatement vs joined tree, worst %.2e" % (case, worst))
    assert worst <= 1e-11


def _is_binary(tree):
    return all(len(n.children) in (0, 2) for n in tree.seed_node.postorder())


@pytest.mark.parametrize("newick", ["(t0:0.1,t1:0.2,(t2:0.15,t3:0.3):0.25);",
                                    "((a:0.1,b:0.2):0.05,(c:0.3,(d:0.1,e:0.2):0.07):0.11);"])
def test_attach(newick):
    base = prepare_tree(newick)
    tr = Traversal(base)
    total = sum(tr.brlens.values())
    for row in tr.optimising_traversal:
        if row[3] < 0:
            continue
        for edge in ((int(row[3]), int(row[4])), (int(row[4]), int(row[3]))):
            t = PL.attach(newick, edge, "query", 0.4)
            assert _is_binary(t)
            tr2 = Traversal(prepare_tree(t))
            assert sorted(tr2.names) == sorted(list(tr.names) + ["query"])
            assert tr2.n_nodes == tr.n_nodes + 2
            assert abs(sum(tr2.brlens.values()) - total - 0.4) <= 1e-15
            q = tr2.names["query"]
            (pend,) = [v for (a, b), v in tr2.brlens.items() if q in (a, b)]
            assert pend == 0.4
            # the two halves of the split edge meet at the query's neighbour
            x = next(a + b - q for (a, b) in tr2.brlens if q in (a, b))
            halves = sorted(v for (a, b), v in tr2.brlens.items() if x in (a, b) and q not in (a, b))
            assert halves == [0.5 * tr.brlens[edge], 0.5 * tr.brlens[edge]]
            back = Traversal(prepare_tree(parse_newick(t.as_newick())))
            assert sorted(back.brlens.values()) == sorted(tr2.brlens.values())
            assert back.names.keys() == tr2.names.keys()
    with pytest.raises(ValueError):
        PL.attach(newick, (0, 10 ** 6), "query", 0.1)
    with pytest.raises(ValueError):
        PL.attach(newick, tuple(int(v) for v in tr.optimising_traversal[0][3:]),
                  next(iter(tr.names)), 0.1)


def _result(tree, rng, Q=3, keep=4):
    tr = Traversal(tree)
    edges = np.array([(r[3], r[4]) for r in tr.optimising_traversal if r[3] >= 0], dtype=np.int32)
    lengths = np.array([tr.brlens[int(a), int(b)] for a, b in edges])
    placements = []
    for _ in range(Q):
        rows = []
        for e in rng.choice(len(edges), keep, replace=False):
            rows.append(dict(edge=tuple(int(v) for v in edges[e]), edge_num=int(e),
                             lnl=float(-1000 - 5 * rng.random()), pendant=float(rng.random()),
                             distal=0.5 * float(lengths[e]), iters=3))
        rows.sort(key=lambda r: (-r["lnl"], r["edge_num"]))
        for r, w in zip(rows, PL.weight_ratios([r["lnl"] for r in rows])):
            r["lwr"] = float(w)
        placements.append(rows)
    return dict(names=["q%d" % k for k in range(Q)], edges=edges, lengths=lengths,
                placements=placements)


@pytest.mark.parametrize("newick", ["(t0:0.1,t1:0.2,(t2:0.15,t3:0.3):0.25);",
                                    "(((a:0.1,b:0.2):0.05,(c:0.3,(d:0.1,e:0.2):0.07):0.11):0.2,f:0.3);",
                                    "(f:0.3,((a:0.1,b:0.2):0.05,(c:0.3,(d:0.1,e:0.2):0.07):0.11):0.2);"])
def test_write_jplace(newick, tmp_path):
    tree = prepare_tree(newick)
    res = _result(tree, np.random.default_rng(3))
    path = tmp_path / "out.jplace"
    PL.write_jplace(str(path), tree, res)
    doc = json.loads(path.read_text())
    assert doc["version"] == 3 and doc["fields"] == PL.JPLACE_FIELDS
    nums = [int(v) for v in re.findall(r"\{(\d+)\}", doc["tree"])]
    assert sorted(nums) == list(range(len(res["edges"])))
    # the tree string, edge numbers taken out, is the same unrooted tree with the same lengths
    plain = Traversal(prepare_tree(re.sub(r"\{\d+\}", "", doc["tree"])))
    tr = Traversal(tree)
    assert plain.names.keys() == tr.names.keys()
    assert np.allclose(sorted(plain.brlens.values()), sorted(tr.brlens.values()), rtol=0,
                       atol=1e-15)
    # every number stands behind the length of its own edge
    by_num = {int(k): float(v) for v, k in re.findall(r":([0-9.eE+-]+)\{(\d+)\}", doc["tree"])}
    assert [by_num[k] for k in range(len(res["edges"]))] == res["lengths"].tolist()
    for entry, rows in zip(doc["placements"], res["placements"]):
        assert abs(sum(p[2] for p in entry["p"]) - 1.0) <= 1e-12
        assert [p[0] for p in entry["p"]] == [r["edge_num"] for r in rows]
        assert all(p[3] == 0.5 * res["lengths"][p[0]] for p in entry["p"])
    assert [e["n"] for e in doc["placements"]] == [[n] for n in res["names"]]


def test_candidate_selection_is_deterministic_under_ties():
    scores = np.array([[-5.0, -1.0], [-3.0, -1.0], [-3.0, -2.0], [-3.0, -1.0], [-9.0, -np.inf]])
    assert PL.select_candidates(scores, 3) == [[1, 2, 3], [0, 1, 3]]
    assert PL.select_candidates(scores, 1) == [[1], [0]]
    assert PL.select_candidates(scores, 99) == [[1, 2, 3, 0, 4], [0, 1, 3, 2, 4]]
    assert PL.select_candidates(scores[::-1].copy(), 2) == [[1, 2], [1, 3]]
    w = PL.weight_ratios([-1000.0, -1001.0, -1e6])
    assert abs(w.sum() - 1) <= 1e-15 and w[0] > w[1] > w[2] == 0.0


def decided(r, prob, q, l0=0.1):
    """(best edge number, its pendant optimum, gap to the runner-up over |lnL|) of query q over
    every edge, each at its Brent optimum."""
    opt = [r.optimum(q, k, l0) for k in range(len(r.edges))]
    lnl = np.array([o[1] for o in opt])
    order = np.argsort(-lnl, kind="stable")
    return int(order[0]), opt[order[0]][0], (lnl[order[0]] - lnl[order[1]]) / abs(lnl[order[0]])


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_planted_queries_are_decided(case, oracle_mod):
    """Every tip copy and simulated sister the device test checks: the best restated edge is
    the planted one by more than 1e-6 |lnL| over the runner-up, and a tip copy's pendant
    optimum is the lower bound."""
    r = restated(oracle_mod, case)
    prob = r.prob
    assert prob["planted"]
    for q, edge in sorted(prob["planted"].items()):
        best, pend, gap = decided(r, prob, q)
        print("%s: query %d (%s) best edge %s planted %s pendant %.3g gap %.2e" % (
            case, q, prob["kinds"][q], tuple(r.edges[best]), edge, pend, gap))
        assert tuple(int(v) for v in r.edges[best]) == edge
        assert gap > 1e-6
        if prob["kinds"][q].startswith("copy"):
            assert pend == R.LO
