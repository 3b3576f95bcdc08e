"""NNI on the device: the quartet kernel (pu_quartet_derivs) and the scoring pass
(pu_nni_sweep) against the CPU restatement (tests/nni_reference.py, composed from the oracle),
against the existing edge path and against real trees, then the search.  Tolerances are those of
tests/test_gpu_edges.py for the same quantities."""
import ctypes

import numpy as np
import pytest

import nni_reference as R
import twostate as T
import walk_errors as W
from test_cli import _write_case

from phylo_utils_amd import TreeModel, phy
from phylo_utils_amd import _native as N
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem, simulate_states
from phylo_utils_amd.tree import (Node, Tree, apply_nni, apply_nni_moves, internal_edges,
                                  prepare_tree)

pytestmark = pytest.mark.gpu

GTR = lambda: SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
rates_of = lambda C, a=0.5: GammaRateModel(C, a) if C > 1 else UniformRateModel()


def _close(x, y, rtol):
    assert abs(x - y) <= rtol * max(1.0, abs(y)), (x, y, abs(x - y))


def _tm(tree, names, codes, table, m, rm, compact=True, keep=True):
    tm = TreeModel(device=0, keep_partials=keep, compact_tips=compact)
    if compact:
        tm.set_alignment_codes(codes, table, names)
    else:
        tm.set_alignment_partials(np.asarray(table)[codes], names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    return tm


def _setup(kind, n_taxa, n_sites, C, seed, compact=True, keep=True):
    """(tm, tree, eigen dict, tips {node: [S][K]})."""
    rm = rates_of(C, 0.8 if kind == "protein" else 0.5)
    if kind == "binary":
        m = T.TwoState(0.3)
        tree, names, codes, table, _ = T.binary_problem(n_taxa, n_sites, 0.3, rm.rates, seed=seed)
    else:
        m = GTR() if kind == "dna" else SM.LG()
        tree, names, st = make_problem(n_taxa, n_sites, m, rm.rates, seed=seed)
        codes, table = st.astype(np.uint8), np.eye(len(m.freqs))
    tm = _tm(tree, names, codes, table, m, rm, compact, keep)
    tr = tm.traversal
    tips = {tr.names[n]: np.asarray(table)[codes[i]] for i, n in enumerate(names)}
    return tm, tree, R.eigen(m, rm), tips


def _node_sets(tr):
    """Three quartets of nodes: four internal, two tips + two internal, one tip + three."""
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    tips = sorted(tr.names.values())
    return [(inner[0], inner[-1], inner[2], inner[1]), (tips[0], inner[1], tips[3], inner[-2]),
            (inner[3], tips[1], inner[0], inner[-1])]


LENS = (0.07, 0.21, 0.13, 0.4, 0.09)
CASES = {
    "dna-coded-14x700-C4": ("dna", 14, 700, 4, True),
    "dna-dense-S97-C1": ("dna", 8, 97, 1, False),
    "dna-S65-C3": ("dna", 8, 65, 3, True),
    "binary-C8-S130": ("binary", 9, 130, 8, True),
    "binary-C25-S70": ("binary", 8, 70, 25, True),  # the LDS limit of K = 2
    "protein-C4-S97": ("protein", 8, 97, 4, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_quartet_derivs_vs_restatement(oracle_mod, case):
    kind, n_taxa, n_sites, C, compact = CASES[case]
    tm, tree, e, tips = _setup(kind, n_taxa, n_sites, C, seed=2, compact=compact)
    st = R.state(oracle_mod, tips, tm.traversal, e)
    P, S = st["partials"], st["scale"]
    lnl0 = tm.likelihood()
    worst = 0.0
    for nodes in _node_sets(tm.traversal):
        for t in (None, (1e-6, 0.05, 3.0)):
            got = tm.quartet_derivatives(nodes, LENS, t)
            ref = R.quartet_derivs(oracle_mod, P, S, nodes, LENS, t, e)
            for k in range(3):
                for j in range(3):
                    worst = max(worst, abs(got[k, j] - ref[k, j]) / max(1.0, abs(ref[k, j])))
                    _close(got[k, j], ref[k, j], 1e-10)
    print("%s: max error relative to max(1, |v|) %.2e" % (case, worst))
    assert tm.likelihood() == lnl0  # nothing in the context changed


def _caterpillar(n, rng):
    cur = Node("t0", 0.2)
    for i in range(1, n - 1):
        p = Node(None, rng.uniform(0.05, 0.3))
        p.add(cur)
        p.add(Node("t%d" % i, rng.uniform(0.05, 0.3)))
        cur = p
    root = Node()
    root.add(cur)
    root.add(Node("t%d" % (n - 1), 0.2))
    return Tree(root)


def test_quartet_derivs_on_rescaled_nodes(oracle_mod):
    """A 150-taxon caterpillar: the deep nodes carry non-zero scalers (asserted on the device's
    own partials), which enter L and R and the category mix."""
    rng = np.random.default_rng(5)
    m, rm = GTR(), rates_of(4)
    tree = _caterpillar(150, rng)
    sts = simulate_states(rng, tree, m, rm.rates, 130)
    names = sorted(sts)
    codes = np.array([sts[n] for n in names], dtype=np.uint8)
    tm = _tm(tree, names, codes, np.eye(4), m, rm)
    tr = tm.traversal
    e = R.eigen(m, rm)
    tips = {tr.names[n]: np.eye(4)[codes[i]] for i, n in enumerate(names)}
    st = R.state(oracle_mod, tips, tr, e)
    P, S = st["partials"], st["scale"]
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    nodes = (inner[-2], inner[-3], inner[-5], inner[len(inner) // 2])  # (inner[-1]: two tips)
    assert any((tm.node_partials(v)[1] != 0).any() for v in nodes)
    assert all((S[v] != 0).any() for v in nodes[:3])
    for t in (None, (1e-6, 0.05, 3.0)):
        got = tm.quartet_derivatives(nodes, LENS, t)
        ref = R.quartet_derivs(oracle_mod, P, S, nodes, LENS, t, e)
        for k in range(3):
            for j in range(3):
                _close(got[k, j], ref[k, j], 1e-10)


def _walk_internal_edges(tm):
    """Apply the optimising traversal's update rows on the device and yield, at every internal
    edge, (nod, par, quartet nodes, lens[5])."""
    tr = tm.traversal
    child = {int(p): (int(a), int(b)) for p, a, b in tr.postorder_traversal}
    for row in tr.optimising_traversal:
        if row[0] >= 0:
            p, x, y = (int(v) for v in row[:3])
            tm.update_partials([row[:3]], [[tr.brlens[p, x], tr.brlens[p, y]]])
        nod, par = int(row[3]), int(row[4])
        if nod < 0 or nod not in child or par not in child:
            continue
        nodes = child[nod] + ((int(row[1]), int(row[2])) if row[0] >= 0 else child[par])
        lens = [tr.brlens[nodes[0], nod], tr.brlens[nodes[1], nod], tr.brlens[nodes[2], par],
                tr.brlens[nodes[3], par], tr.brlens[nod, par]]
        yield nod, par, nodes, lens


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_arrangement_0_is_the_existing_edge_path(kind):
    tm, tree, e, tips = _setup(kind, 11, 500, 4, seed=9)
    n = 0
    for nod, par, nodes, lens in _walk_internal_edges(tm):
        got = tm.quartet_derivatives(nodes, lens)[0]
        ref = tm.edge_derivatives(nod, par)
        for j in range(3):
            _close(got[j], ref[j], 1e-11)
        n += 1
    assert n == 11 - 3


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_arrangements_1_and_2_are_real_trees(oracle_mod, kind):
    tm, tree, e, tips = _setup(kind, 11, 500, 4, seed=9)
    m, rm = tm.substitution_model, tm.rate_model
    names = sorted(tm.names, key=tm.names.get)
    codes, table = tm._codes
    byname = {n: np.asarray(table)[codes[tm.names[n]]] for n in names}
    lnl0 = tm.likelihood()
    for nod, par, nodes, lens in _walk_internal_edges(tm):
        got = tm.quartet_derivatives(nodes, lens)
        _close(got[0, 0], lnl0, 1e-11)
        for k in (1, 2):
            moved = apply_nni(tree, nod, par, k)
            fresh = _tm(moved, names, codes, table, m, rm)
            _close(got[k, 0], fresh.likelihood(), 1e-11)
            tr2 = fresh.traversal
            ref = R.state(oracle_mod, {tr2.names[n]: v for n, v in byname.items()}, tr2, e)["lnl"]
            _close(got[k, 0], ref, 1e-9)


def _branch_lengths(tm):
    bl = np.empty((len(tm.traversal.postorder_traversal), 2))
    rl = ctypes.c_double()
    N.check(N.lib().pu_get_branch_lengths(tm._ctx, N.ptr(bl), ctypes.byref(rl)), tm._ctx)
    return bl, rl.value


@pytest.mark.parametrize("kind,compact", [("dna", True), ("dna", False), ("protein", True)])
def test_nni_sweep_vs_restatement(oracle_mod, kind, compact):
    tm, tree, e, tips = _setup(kind, 10, 600, 4, seed=4, compact=compact)
    lnl0, site0, bl0 = tm.likelihood(), tm.sitewise_patterns().copy(), _branch_lengths(tm)
    quartets, scores = tm.nni_scores(tol=1e-8, max_iter=50)
    assert len(quartets) == 10 - 3
    assert [(int(q[0]), int(q[1])) for q in quartets] == internal_edges(tree)
    assert len(set(tuple(sorted((int(q[0]), int(q[1])))) for q in quartets)) == 10 - 3
    # the context is where a traversal leaves it, bit for bit, and no length moved
    assert tm.likelihood() == lnl0
    assert np.array_equal(tm.sitewise_patterns(), site0)
    bl1 = _branch_lengths(tm)
    assert np.array_equal(bl1[0], bl0[0]) and bl1[1] == bl0[1]
    q2, s2 = tm.nni_scores(tol=1e-8, max_iter=50)
    assert np.array_equal(q2, quartets) and np.array_equal(s2, scores)
    _, rq, rs = R.sweep(oracle_mod, tips, tm.traversal, e, tol=1e-8, max_iter=50)
    assert np.array_equal(rq, quartets)
    for got, ref in zip(scores.reshape(-1, 4), rs.reshape(-1, 2)):
        assert abs(got[0] - ref[0]) <= 1e-6 * max(ref[0], 1e-3), (got, ref)
        _close(got[1], ref[1], 1e-9)
        assert got[3] >= 1
    for s in scores:  # arrangement 0 at its optimum is no worse than the standing tree
        assert s[0, 1] >= lnl0 - 1e-9 * abs(lnl0)


def test_refusals():
    kmax = N.lib().pu_quartet_max_cat(20)
    if kmax < 64:
        rm = GammaRateModel(kmax + 1, 0.8)
        m = SM.LG()
        tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
        tm = _tm(tree, names, st.astype(np.uint8), np.eye(20), m, rm)
        lnl0 = tm.likelihood()
        with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
            tm.nni_scores()
        inner = sorted(set(int(p) for p in tm.traversal.postorder_traversal[:, 0]))
        with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
            tm.quartet_derivatives(inner[:4], LENS)
        assert tm.likelihood() == lnl0
        tm.compute_partials()
        assert tm.likelihood() == lnl0
    tm, tree, e, tips = _setup("dna", 8, 70, 4, seed=1, keep=False)
    for call in (tm.nni_search, tm.nni_scores, lambda: tm.quartet_derivatives((8, 9, 10, 11), LENS)):
        with pytest.raises(ValueError, match="keep_partials"):
            call()
    tm, tree, e, tips = _setup("dna", 8, 70, 4, seed=1)
    inner = sorted(set(int(p) for p in tm.traversal.postorder_traversal[:, 0]))
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*repeated"):
        tm.quartet_derivatives((inner[0], inner[1], inner[0], inner[2]), LENS)
    with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
        tm.quartet_derivatives(inner[:4], (0.1, 0.0, 0.1, 0.1, 0.1))
    with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
        tm.quartet_derivatives((inner[0], inner[1], inner[2], 10 ** 6), LENS)
    with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
        tm.nni_scores(tol=0.0)
    tree, names, st = make_problem(8, 70, GTR(), [1.0], seed=1)
    tm = _tm(tree, names, st.astype(np.uint8), np.eye(4), SM.Unrest(), UniformRateModel())
    for call in (tm.nni_search, tm.nni_scores):
        with pytest.raises(ValueError, match="reversible"):
            call()
    tm, tree, e, tips = _setup("dna", 8, 70, 1, seed=1)
    tm.set_ascertainment_bias_correction()
    for call in (tm.nni_search, tm.nni_scores):
        with pytest.raises(ValueError, match="ascertainment"):
            call()


def _search_problem():
    m, rm = GTR(), rates_of(4)
    tree, names, st = make_problem(9, 1500, m, rm.rates, seed=11)
    edges = internal_edges(tree)
    (a, b) = next((x, y) for i, x in enumerate(edges) for y in edges[i + 1:]
                  if not set(x) & set(y))
    start = apply_nni_moves(tree, [(a[0], a[1], 1, None), (b[0], b[1], 2, None)])
    assert len(R.splits(start) ^ R.splits(tree)) == 4
    return m, rm, tree, start, names, st.astype(np.uint8)


def test_nni_search():
    m, rm, tree, start, names, codes = _search_problem()
    runs = []
    for _ in range(2):
        tm = _tm(start, names, codes, np.eye(4), m, rm)
        lnl_start = tm.optimise_branch_lengths()
        final, lnl, history = tm.nni_search()
        runs.append(final.as_newick())
    assert lnl > lnl_start
    assert history and all(h["after"] > h["before"] for h in history)
    assert 2 * sum(h["fallback"] for h in history) <= len(history)
    assert R.splits(final) == R.splits(tree)  # the generating topology, on 1500 sites
    assert lnl == tm.likelihood()
    quartets, scores = tm.nni_scores()
    assert (scores[:, 1:, 1] - lnl <= 1e-3).all()
    assert runs[0] == runs[1]


def test_cli_nni(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    spec = "HKY{2.0}+G4{0.7}"
    assert phy.main(["-s", fa, "-m", spec, "--nj", "nj"]) == 0
    plain = float(capsys.readouterr().out.split("=")[1])
    out = tmp_path / "final.nwk"
    assert phy.main(["-s", fa, "-m", spec, "--nj", "nj", "--nni", "-o", str(out)]) == 0
    searched = float(capsys.readouterr().out.split("=")[1])
    assert searched >= plain
    assert len(prepare_tree(out.read_text()).leaf_nodes()) == 9
    assert phy.main(["-t", nw, "-s", fa, "-m", spec, "--nni", "2"]) == 0
    assert np.isfinite(float(capsys.readouterr().out.split("=")[1]))


def test_an_error_in_mid_walk_puts_the_context_back():
    """pu_nni_sweep, then pu_branch_support, on rows whose last edge names a PAR that is not
    NOD's neighbour (walk_errors.py): PU_E_ARG from both, and the lnL, sitewise lnL and partials
    are pu_run's again."""
    tm, _, _, _ = _setup(*CASES["dna-S65-C3"][:4], seed=2)
    tm.likelihood()
    bad = W.rows_with_a_bad_last_edge(tm)
    before = W.snapshot(tm)
    n, n_rep = len(tm.names) - 3, 10
    scores, quartets, cnt = np.zeros((n, 3, 4)), np.zeros((n, 6), dtype=np.int32), ctypes.c_int()
    rc = N.lib().pu_nni_sweep(tm._ctx, len(bad), N.ptr(bad), 1e-8, 50, N.ptr(scores),
                              N.ptr(quartets), ctypes.byref(cnt))
    W.assert_refused_and_put_back(tm, before, rc)
    sup = np.zeros((n, 4))
    rc = N.lib().pu_branch_support(tm._ctx, len(bad), N.ptr(bad), 1e-8, 50, 7, 0, n_rep, 0.1,
                                   N.ptr(scores), N.ptr(quartets), N.ptr(sup), None,
                                   ctypes.byref(cnt))
    W.assert_refused_and_put_back(tm, before, rc)
