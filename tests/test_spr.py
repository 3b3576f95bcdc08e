"""Subtree pruning and regrafting on the host: the CPU restatement of the regraft
score (tests/spr_reference.py) against the oracle's lnL of the rearranged tree, ``apply_spr``,
and the rows ``spr_rows`` hands to pu_spr_sweep, replayed with the oracle's ``clv``."""
import numpy as np
import pytest

import spr_reference as R

from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem
from phylo_utils_amd.tree import (Node, Traversal, Tree, apply_spr, prepare_tree, spr_candidates,
                                  spr_rows, with_lengths)


def _problem(kind, n_taxa, seed=4):
    m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if kind == "dna" else SM.LG()
    rm = GammaRateModel(4, 0.5 if kind == "dna" else 0.8)
    tree, names, st = make_problem(n_taxa, 40, m, rm.rates, seed=seed)
    K = len(m.freqs)
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, size=40).astype(np.float64)
    return dict(tree=tree, names=names, codes=st.astype(np.uint8), table=np.eye(K), model=m,
                rm=rm, compact=True, weights=w)


@pytest.fixture(scope="module", params=["dna-7", "dna-12", "protein-7", "protein-12"])
def restated(request, oracle_mod):
    kind, n = request.param.split("-")
    ref = R.Restated(oracle_mod, _problem(kind, int(n)))
    return request.param, ref, ref.all_moves()


def test_score_is_the_oracle_lnl_of_the_rearranged_tree(restated):
    """Every move of the 7- and 12-taxon trees under GTR+G4 and LG+G4: the restatement's score
    is oracle.tree_lnl of apply_spr's tree (pulley principle) at 1e-11 relative, the tolerance
    of tests/test_place.py for the same argument.  Measured: worst 7.7e-14 (protein-12), 5.2e-16 (dna-12)."""
    case, ref, moves = restated
    n_taxa = len(ref.prob["names"])
    per = {}
    worst = 0.0
    for (n, o, u, v), (d, score) in moves.items():
        want = ref.moved_lnl(n, o, u, v)
        worst = max(worst, abs(score - want) / abs(want))
        per[n, o] = per.get((n, o), 0) + 1
    print("%s: %d moves, worst relative error %.2e" % (case, len(moves), worst))
    assert worst <= 1e-11
    # 2(N - k) - 3 moves per candidate, k the leaves on n's side
    tr = ref.tr
    for (n, o), count in per.items():
        side, todo = {n}, [n]
        while todo:
            for z in ref.adj[todo.pop()]:
                if z != o and z not in side:
                    side.add(z)
                    todo.append(z)
        k = sum(1 for z in side if len(ref.adj[z]) == 1)
        assert count == 2 * (n_taxa - k) - 3, (n, o)
    assert sorted(per) == sorted(spr_candidates(ref.prob["tree"]))
    # the root edge's ends take part like any node
    left, right = (int(z) for z in tr.root_edge)
    assert any(o in (left, right) for _, o in per)
    assert any(u in (left, right) or v in (left, right) for _, _, u, v in moves)
    assert any({u, v} == {left, right} for _, _, u, v in moves)


def _lengths(tree):
    """{split (the side without the smallest leaf): edge length} of every edge, tip edges too."""
    t = prepare_tree(tree)
    tr = Traversal(t)
    leaves = frozenset(n.label for n in t.leaf_nodes())
    first = min(leaves)
    below = {}
    for n in t.seed_node.postorder():
        below[n] = frozenset([n.label]) if n.is_leaf() else \
            frozenset().union(*(below[c] for c in n.children))
    out = {}
    for n, i in tr.node_dict.items():
        nb = n.parent if n.parent is not t.seed_node else \
            next(c for c in t.seed_node.children if c is not n)
        s = below[n]
        out[leaves - s if first in s else s] = float(tr.brlens[i, tr.node_dict[nb]])
    return out


def test_apply_spr_builds_the_defined_tree(restated):
    case, ref, moves = restated
    tree = ref.tree
    base = _lengths(tree)
    names = sorted(ref.prob["names"])
    for (n, o, u, v), (d, _) in moves.items():
        new = apply_spr(tree, n, o, u, v)
        t = prepare_tree(new)
        assert sorted(x.label for x in t.leaf_nodes()) == names
        assert all(len(x.children) in (0, 2) for x in t.seed_node.postorder())
        got = _lengths(new)
        assert len(got) == len(base) == 2 * len(names) - 3
        R_, x, y, merged, l, _ = ref.rest(n, o)
        # the lengths of the definition: two halves of t, the pendant l, the merged edge (unless
        # it is the one split), everything else as it was
        vals = sorted(got.values())
        want = sorted(base.values())
        for gone in (ref.adj[o][x], ref.adj[o][y], ref.adj[n][o]) + \
                (() if {u, v} == {x, y} else (R_[u][v],)):
            want.remove(gone)
        want += [0.5 * R_[u][v]] * 2 + [l] + ([] if {u, v} == {x, y} else [merged])
        assert np.allclose(vals, sorted(want), rtol=0, atol=1e-15), (n, o, u, v)
        if d == 0:
            assert R.splits(new) == R.splits(tree)
        elif d >= 2:
            assert R.splits(new) != R.splits(tree)
    # a move followed by its inverse restores the topology (and moves the attachment point only)
    far = [k for k, (d, _) in moves.items() if d >= 2][:25]
    for n, o, u, v in far:
        moved = prepare_tree(apply_spr(tree, n, o, u, v))
        side, todo = {n}, [n]
        while todo:
            for z in ref.adj[todo.pop()]:
                if z != o and z not in side:
                    side.add(z)
                    todo.append(z)
        tr0 = ref.tr
        name = {i: s for s, i in tr0.names.items()}
        sub = frozenset(name[z] for z in side if z in name)
        x, y = [z for z in ref.adj[o] if z != n]

        def leafset(a, b):  # the leaves on a's side of edge (a, b) of the old tree
            s, td = {a}, [a]
            while td:
                for z in ref.adj[td.pop()]:
                    if z != b and z not in s:
                        s.add(z)
                        td.append(z)
            return frozenset(name[z] for z in s if z in name)

        back = _find_move(moved, sub, leafset(x, o), leafset(y, o))
        assert back is not None, (n, o, u, v)
        assert R.splits(apply_spr(moved, *back)) == R.splits(tree)
    with pytest.raises(ValueError):
        apply_spr(tree, 0, 1, 2, 3) if 1 not in ref.adj[0] else apply_spr(tree, 0, 0, 1, 2)
    n, o, u, v = next(iter(moves))
    with pytest.raises(ValueError, match="rest tree"):
        apply_spr(tree, n, o, n, o)


def _find_move(tree, sub, side_x, side_y):
    """The move on `tree` that cuts the subtree with leaves `sub` and regrafts it on the edge
    that separates side_x from the rest (leaf sets of the old tree, `sub` aside); side_y is that
    rest."""
    tr = Traversal(prepare_tree(tree))
    adj = {i: set() for i in range(tr.n_nodes)}
    for a, b in tr.brlens:
        adj[a].add(b)
        adj[b].add(a)
    name = {i: s for s, i in tr.names.items()}

    def leaves(a, b):
        s, td = {a}, [a]
        while td:
            for z in adj[td.pop()]:
                if z != b and z not in s:
                    s.add(z)
                    td.append(z)
        return frozenset(name[z] for z in s if z in name)

    for n in adj:
        for o in adj[n]:
            if leaves(n, o) != sub:
                continue
            for u in adj:
                for v in adj[u]:
                    if o not in (u, v) and leaves(u, v) - sub == side_x:
                        return n, o, u, v
    return None


def test_rows_replayed_on_the_host(restated):
    """The outer and inner rows with a host-side update (oracle.clv): after each candidate's
    rows every node's partial is bitwise what it was before them, and the (A, B, S, t, l) of
    every scoring row are those the restatement derives from R on its own."""
    case, ref, moves = restated
    orc, tr, e = ref.orc, ref.tr, ref.e
    st = R.state(orc, ref.tips, tr, e, ref.prob["weights"])
    P, S = st["partials"], st["scale"]
    rows, off, inner, lens, table = spr_rows(tr)
    assert len(off) == len(rows) + 1 and off[-1] == len(inner) == len(lens) == len(table)

    def update(p, a, la, b, lb):
        cml = np.zeros(S[p].shape)
        P[p] = orc.clv(ref.pm(la), ref.pm(lb), P[a], P[b], S[a], S[b], cml)
        S[p] = cml

    # as pu_spr_sweep does before its walk: every internal node rewritten by the update function
    # itself (the state above comes from the oracle's compiled traversal)
    for p, a, b in tr.postorder_traversal:
        update(int(p), int(a), tr.brlens[p, a], int(b), tr.brlens[p, b])
    seen = {}
    worst = 0.0
    for r, row in enumerate(rows):
        if row[0] >= 0:
            p, a, b = (int(z) for z in row[:3])
            update(p, a, tr.brlens[p, a], b, tr.brlens[p, b])
        lo, hi = int(off[r]), int(off[r + 1])
        if row[3] < 0:
            assert lo == hi
            continue
        i = lo
        while i < hi:  # one candidate at a time
            j = i
            while j < hi and tuple(table[j][:2]) == tuple(table[i][:2]):
                j += 1
            before = (P.copy(), S.copy())
            for k in range(i, j):
                x, ln, mv = inner[k], lens[k], table[k]
                if x[0] >= 0:
                    assert x[3] < 0 and mv[2] == mv[3] == mv[4] == -1
                    update(int(x[0]), int(x[1]), ln[0], int(x[2]), ln[1])
                    continue
                a, b, s = (int(z) for z in x[3:])
                n, o, u, v, d = (int(z) for z in mv)
                assert (a, b, s) == (u, v, n) and x[0] < 0
                got = R.score_from(orc, e, ref.prob["weights"], P[a], S[a], P[b], S[b], P[s],
                                   S[s], ln[2], ln[3])
                dist, want = moves[R.key(n, o, u, v)]
                A_, sA, B_, sB, S_, sS, t, l = ref.ends(n, o, u, v)
                assert (ln[2], ln[3]) == (t, l) and d == dist
                # the same vectors up to the order of the two factors of a product
                assert np.allclose(P[a], A_, rtol=1e-13, atol=0) and np.array_equal(S[a], sA)
                assert np.allclose(P[b], B_, rtol=1e-13, atol=0) and np.array_equal(S[b], sB)
                assert np.allclose(P[s], S_, rtol=1e-13, atol=0) and np.array_equal(S[s], sS)
                worst = max(worst, abs(got - want) / abs(want))
                assert R.key(n, o, u, v) not in seen
                seen[R.key(n, o, u, v)] = got
            assert np.array_equal(P, before[0]) and np.array_equal(S, before[1]), table[i][:2]
            i = j
    assert set(seen) == set(moves)
    assert worst <= 1e-13
    # a radius-r row set scores exactly the moves of distance <= r
    for radius in (0, 1, 2, 3):
        _, off_r, inner_r, _, table_r = spr_rows(tr, radius)
        got = set(R.key(*m[:4]) for m, x in zip(table_r, inner_r) if x[3] >= 0)
        assert got == set(k for k, (d, _) in moves.items() if d <= radius), radius
        assert all(m[4] <= radius for m in table_r)


def test_caterpillar_of_1000_taxa_builds_without_recursion():
    rng = np.random.default_rng(0)
    cur = Node("t0", 0.2)
    for i in range(1, 999):
        p = Node(None, float(rng.uniform(0.05, 0.3)))
        p.add(cur)
        p.add(Node("t%d" % i, float(rng.uniform(0.05, 0.3))))
        cur = p
    root = Node()
    root.add(cur)
    root.add(Node("t999", 0.2))
    tr = Traversal(prepare_tree(Tree(root)))
    rows, off, inner, lens, moves = spr_rows(tr, radius=2)
    assert len(rows) == 3 * 1000 - 5 and off[-1] == len(inner) > 2 * 1000
    assert moves[:, 4].max() == 2
    # one deep candidate of the full walk: the subtree of one leaf, every other edge scored
    t = apply_spr(Tree(root), tr.names["t0"], int(tr.postorder_traversal[0][0]),
                  tr.names["t999"], int(tr.root_edge[0]) if tr.names["t999"] == tr.root_edge[1]
                  else int(tr.root_edge[1]))
    assert len(t.leaf_nodes()) == 1000


def test_search_precondition(oracle_mod):
    """The fixture of the device search test (tests/test_gpu_spr.py, tests/test_cli_spr.py) on
    the reference alone: at the start tree's lengths after one oracle.optimise_sweep, the
    restatement's scores rank a move back to G's topology within the top KEEP pruned subtrees,
    the move that made the start tree has distance >= 3, and no single NNI undoes it (the start
    tree differs from G in more than one split)."""
    from phylo_utils_amd.spr import rank_moves
    sp = R.search_problem()
    assert sp["move"][4] >= 3
    assert len(R.splits(sp["G"]) ^ R.splits(sp["start"])) > 2
    states = R.simulated_on_host(sp)
    names = sorted(states, key=lambda s: int(s[1:]))
    prob = dict(tree=sp["start"], names=names,
                codes=np.array([states[n] for n in names], dtype=np.uint8), table=np.eye(4),
                model=sp["model"], rm=sp["rm"], weights=np.ones(R.SEARCH_SITES))
    ref = R.Restated(oracle_mod, prob)
    tr, e = ref.tr, ref.e
    lens, _ = oracle_mod.optimise_sweep(ref.tips, tr.postorder_traversal, tr.op_lengths(),
                                        tr.root_edge, tr.root_length(), e["evecs"], e["evals"],
                                        e["ivecs"], e["freqs"], e["rates"], e["weights"],
                                        tr.optimising_traversal, tr.n_nodes)
    ref = R.Restated(oracle_mod, dict(prob, tree=with_lengths(sp["start"], lens)))
    moves = ref.all_moves()
    keys = list(moves)
    table = [k + (moves[k][0],) for k in keys]
    trial = rank_moves(table, [moves[k][1] for k in keys], R.KEEP)
    want = R.splits(sp["G"])
    hits = [i for i, m in enumerate(trial) if R.splits(apply_spr(ref.tree, *m[:4])) == want]
    print("seed %d: the move back to G ranks %s of %d trial moves" % (sp["seed"], hits, len(trial)))
    assert hits
