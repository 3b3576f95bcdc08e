"""Subtree pruning and regrafting on the device: k_regraft through pu_regraft_edge
and pu_spr_sweep against the CPU restatement (tests/spr_reference.py, itself pinned to the
oracle's lnL of the rearranged tree in tests/test_spr.py), against the oracle's lnL of
``apply_spr``'s tree, and against the two-launch device composition pu_update_partials +
pu_edge_lnl; then the search.

Each case makes its device calls once (the `run` fixture); the tests below read what it kept."""
import ctypes

import numpy as np
import pytest

import ancestral_reference as AR
import spr_reference as R
import walk_errors as WE

from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import spr as SPR
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import make_problem
from phylo_utils_amd.tree import Traversal, apply_spr, prepare_tree, spr_rows, with_lengths

pytestmark = pytest.mark.gpu


def _tm(prob, keep=True):
    tm = TreeModel(device=0, keep_partials=keep, compact_tips=prob["compact"])
    if prob["compact"]:
        tm.set_alignment_codes(prob["codes"], prob["table"], prob["names"], prob["weights"])
    else:
        tm.set_alignment_partials(prob["table"][prob["codes"]], prob["names"], prob["weights"])
    tm.set_substitution_model(prob["model"])
    tm.set_rate_model(prob["rm"])
    tm.set_tree(prob["tree"])
    tm.initialise()
    return tm


def _problem(case):
    K = {"binary": 2, "dna": 4, "protein": 20}[R.CASES[case][0]]
    prob = R.problem(case, N.lib().pu_regraft_max_cat(K))
    if R.CASES[case][3] is None:
        assert prob["rm"].ncat == N.lib().pu_regraft_max_cat(K) == 64
    return prob


def _triples(tr):
    """(a, b, s) for pu_regraft_edge on the post-order partials: three internal nodes, then a
    tip as S, as A and as B."""
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    tips = sorted(tr.names.values())
    return [(inner[0], inner[1], inner[2]), (inner[-1], inner[0], tips[0]),
            (tips[1], inner[1], inner[-1]), (inner[2], tips[2], inner[0]),
            (tips[0], tips[1], tips[2])]


@pytest.fixture(scope="module", params=sorted(R.CASES))
def run(request, oracle_mod):
    prob = _problem(request.param)
    ref = R.Restated(oracle_mod, prob)
    tm = _tm(prob)
    before = WE.snapshot(tm)
    single = [(t, SPR.regraft_edge(tm, *t, 0.23, 0.11)) for t in _triples(ref.tr)]
    after_single = WE.snapshot(tm)
    moves, scores = SPR.spr_scores(tm)
    after = WE.snapshot(tm)
    moves2, scores2 = SPR.spr_scores(tm)
    near, near_scores = SPR.spr_scores(tm, radius=2)
    return dict(case=request.param, prob=prob, ref=ref, tm=tm, before=before, single=single,
                after_single=after_single, after=after, moves=moves, scores=scores,
                moves2=moves2, scores2=scores2, near=near, near_scores=near_scores)


def test_regraft_edge_against_the_restatement(run):
    """One launch on three post-order vectors -- internal nodes, and a tip as S, as A and as B
    (tips with ambiguity and gap codes, pattern weights with zeros) -- against the definition
    with transition matrices at 1e-10 relative (DESIGN 4.19's device-versus-restatement
    tolerance).  Measured: at most 4.2e-16 over the seven cases."""
    ref = run["ref"]
    st = R.state(ref.orc, ref.tips, ref.tr, ref.e, run["prob"]["weights"])
    P, S = st["partials"], st["scale"]
    assert (np.asarray(run["prob"]["weights"]) == 0).any()
    assert (run["prob"]["table"].sum(axis=1) > 1).any()
    worst = 0.0
    for (a, b, s), got in run["single"]:
        want = R.score_from(ref.orc, ref.e, run["prob"]["weights"], P[a], S[a], P[b], S[b], P[s],
                            S[s], 0.23, 0.11)
        worst = max(worst, abs(got - want) / abs(want))
    print("%s: pu_regraft_edge worst relative error %.2e" % (run["case"], worst))
    assert worst <= 1e-10


def test_scores_against_the_restatement_and_the_oracle(run):
    """spr_scores(radius=None): the moves are the restatement's, every score is the
    restatement's and -- on the 7- and 12-taxon trees, all of them -- oracle.tree_lnl of
    apply_spr's tree, at 1e-10 relative.  Measured: at most 6.4e-16 against the restatement and
    4.3e-15 against the oracle's lnL (protein-12x130-C1)."""
    ref = run["ref"]
    want = ref.all_moves()
    got = {R.key(*m[:4]): (int(m[4]), s) for m, s in zip(run["moves"], run["scores"])}
    assert len(got) == len(run["moves"]) and set(got) == set(want)
    worst = worst_tree = 0.0
    for k, (d, s) in got.items():
        assert d == want[k][0]
        worst = max(worst, abs(s - want[k][1]) / abs(want[k][1]))
        lnl = ref.moved_lnl(*k)
        worst_tree = max(worst_tree, abs(s - lnl) / abs(lnl))
    print("%s: %d moves, worst relative error %.2e (restatement), %.2e (oracle lnL of the moved "
          "tree)" % (run["case"], len(got), worst, worst_tree))
    assert worst <= 1e-10 and worst_tree <= 1e-10


def test_scores_against_the_device_composition(run):
    """The same number from two launches: pu_update_partials of the dissolved node's slot from
    (A @ t/2, B @ t/2), then pu_edge_lnl(n, o); the rows are replayed one call at a time."""
    tm, lib = run["tm"], N.lib()
    tr = tm.traversal
    rows, off, inner, lens, table = spr_rows(tr)
    adj = {i: {} for i in range(tr.n_nodes)}
    for (a, b), t in tr.brlens.items():
        adj[a][b] = adj[b][a] = float(t)
    tm.likelihood()
    got = {R.key(*m[:4]): s for m, s in zip(run["moves"], run["scores"])}
    worst = 0.0
    lnl = ctypes.c_double()
    for r, row in enumerate(rows):
        if row[0] >= 0:
            p, a, b = (int(z) for z in row[:3])
            tm.update_partials([(p, a, b)], [(adj[p][a], adj[p][b])])
        for i in range(int(off[r]), int(off[r + 1])):
            x, ln, mv = inner[i], lens[i], table[i]
            n, o, u, v = (int(z) for z in mv[:4])
            if x[0] >= 0:
                tm.update_partials([tuple(int(z) for z in x[:3])], [(ln[0], ln[1])])
            else:
                tm.update_partials([(o, u, v)], [(0.5 * ln[2], 0.5 * ln[2])])
                assert lib.pu_edge_lnl(tm._ctx, n, o, ctypes.byref(lnl), None) == 0
                worst = max(worst, abs(got[R.key(n, o, u, v)] - lnl.value) / abs(lnl.value))
            if i + 1 == int(off[r + 1]) or tuple(table[i + 1][:2]) != (n, o):
                # the candidate's rows are over and R's nodes restored: o back to where the
                # walk left it, from its two other neighbours
                x_, y_ = [z for z in adj[o] if z != n]
                tm.update_partials([(o, x_, y_)], [(adj[o][x_], adj[o][y_])])
    tm.compute_partials()
    print("%s: worst relative difference to the two-launch composition %.2e" % (run["case"],
                                                                                 worst))
    assert worst <= 1e-10


def test_state_repeats_and_radius(run):
    b4 = run["before"]
    for af in (run["after_single"], run["after"]):
        assert af["lnl"] == b4["lnl"] and np.array_equal(af["site"], b4["site"])
        for (p0, s0), (p1, s1) in zip(b4["parts"], af["parts"]):
            assert np.array_equal(p0, p1) and np.array_equal(s0, s1)
    assert np.array_equal(run["moves"], run["moves2"])
    assert np.array_equal(run["scores"], run["scores2"])
    full = {R.key(*m[:4]): s for m, s in zip(run["moves"], run["scores"])}
    assert len(run["near"]) < len(run["moves"]) and run["near"][:, 4].max() == 2
    assert sorted(R.key(*m[:4]) for m in run["near"]) == \
        sorted(R.key(*m[:4]) for m in run["moves"] if m[4] <= 2)
    for m, s in zip(run["near"], run["near_scores"]):
        assert s == full[R.key(*m[:4])], m
    # the single call is the sweep's kernel: the merged-edge row of the root edge's first
    # candidate is scored on post-order partials in both
    tm, tr = run["tm"], run["tm"].traversal
    m0 = run["moves"][0]
    n, o, u, v = (int(z) for z in m0[:4])
    assert m0[4] == 0
    t = tr.brlens[o, u] + tr.brlens[o, v]
    one = SPR.regraft_edge(tm, u, v, n, t, tr.brlens[n, o])
    assert abs(one - run["scores"][0]) <= 1e-12 * abs(one)


def test_all_three_vectors_with_scalers(oracle_mod):
    """The 150-taxon caterpillar of tests/test_gpu_place.py (its deep nodes rescale): three
    internal nodes that all carry non-zero scalers at the same patterns, against the restatement."""
    prob = AR.problem("dna-caterpillar-150x130-C4")
    tm = _tm(prob)
    tr = tm.traversal
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    # only the (pattern, category) vectors that fell below the threshold carry a scaler: the
    # three deepest nodes that have any, and patterns at which all three have one
    deep = [v for v in inner if (tm.node_partials(v)[1] != 0).any()]
    assert len(deep) >= 3
    a, b, s = deep[-1], deep[-2], deep[-3]
    parts = [tm.node_partials(v) for v in (a, b, s)]
    for _, sc in parts:
        assert (sc != 0).any()
    joint = (parts[0][1] != 0) & (parts[1][1] != 0) & (parts[2][1] != 0)
    assert joint.any() and (np.asarray(prob["weights"])[joint.any(axis=1)] != 0).any()
    e = R.eigen(prob["model"], prob["rm"])
    want = R.score_from(oracle_mod, e, prob["weights"], parts[0][0], parts[0][1], parts[1][0],
                        parts[1][1], parts[2][0], parts[2][1], 0.3, 0.07)
    got = SPR.regraft_edge(tm, a, b, s, 0.3, 0.07)
    print("caterpillar: nodes %s, %d (pattern, category) with three scalers, down to %.1f, "
          "relative error %.2e" % ((a, b, s), joint.sum(), min(sc.min() for _, sc in parts),
                                   abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-10 * abs(want)


def _sweep_rc(tm, rows, off, inner, lens):
    scores = np.zeros(max(len(inner), 1))
    return N.lib().pu_spr_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(off), N.ptr(inner),
                                N.ptr(lens), N.ptr(scores), None)


def test_refusals_and_an_error_in_mid_sweep():
    lib = N.lib()
    assert lib.pu_regraft_max_cat(3) == N.PU_E_ARG
    assert lib.pu_regraft_max_cat(2) == 64 and lib.pu_regraft_max_cat(4) == 64
    kmax = lib.pu_regraft_max_cat(20)
    assert 4 <= kmax < 64
    prob = _problem("dna-7x67-C1")
    out = ctypes.c_double()

    def calls(tm, t=0.2, l=0.1):
        tr = tm.traversal
        a, b, s = _triples(tr)[0]
        rows, off, inner, lens, _ = spr_rows(tr, 1)
        return (lib.pu_regraft_edge(tm._ctx, a, b, s, t, l, ctypes.byref(out)),
                _sweep_rc(tm, rows, off, inner, lens))

    # more categories than the kernel's LDS holds
    m, rm = SM.LG(), GammaRateModel(kmax + 1, 0.8)
    tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
    big = dict(tree=tree, names=names, codes=st.astype(np.uint8), table=np.eye(20), model=m,
               rm=rm, compact=True, weights=np.ones(70))
    tm = _tm(big)
    lnl0 = tm.likelihood()
    assert calls(tm) == (N.PU_E_ARG,) * 2
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
        SPR.spr_scores(tm)
    assert tm.likelihood() == lnl0
    # partials not kept, host matrices, the ascertainment correction
    assert calls(_tm(prob, keep=False)) == (N.PU_E_STATE,) * 2
    with pytest.raises(ValueError, match="keep_partials"):
        SPR.spr_scores(_tm(prob, keep=False))
    tm = _tm(dict(prob, model=SM.Unrest(), rm=UniformRateModel()))
    assert calls(tm) == (N.PU_E_STATE,) * 2
    with pytest.raises(ValueError, match="reversible"):
        SPR.spr_scores(tm)
    tm = _tm(prob)
    tm.set_ascertainment_bias_correction()
    tm.initialise()
    assert calls(tm) == (N.PU_E_STATE,) * 2
    # arguments: all refused before any launch
    tm = _tm(prob)
    before = WE.snapshot(tm)
    assert calls(tm) == (0, 0)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert calls(tm, t=bad)[0] == N.PU_E_ARG and calls(tm, l=bad)[0] == N.PU_E_ARG
    tr = tm.traversal
    a, b, s = _triples(tr)[0]
    assert lib.pu_regraft_edge(tm._ctx, a, a, s, 0.2, 0.1, ctypes.byref(out)) == N.PU_E_ARG
    assert lib.pu_regraft_edge(tm._ctx, a, b, tr.n_nodes, 0.2, 0.1, ctypes.byref(out)) == \
        N.PU_E_ARG
    assert lib.pu_regraft_edge(tm._ctx, a, b, s, 0.2, 0.1, None) == N.PU_E_ARG
    rows, off, inner, lens, _ = spr_rows(tr)
    mid = len(inner) // 2
    upd = next(i for i in range(mid, len(inner)) if inner[i][0] >= 0)
    sco = next(i for i in range(mid, len(inner)) if inner[i][3] >= 0)
    for col, bad in ((2, 0.0), (3, -1.0), (2, float("nan")), (3, float("inf"))):
        ln = lens.copy()
        ln[sco][col] = bad
        assert _sweep_rc(tm, rows, off, inner, ln) == N.PU_E_ARG
    for col, bad in ((0, 0.0), (1, float("nan"))):
        ln = lens.copy()
        ln[upd][col] = bad
        assert _sweep_rc(tm, rows, off, inner, ln) == N.PU_E_ARG
    for i, col, bad in ((sco, 4, tr.n_nodes), (sco, 5, tr.n_nodes + 3), (upd, 1, -2),
                        (upd, 0, tr.n_nodes)):
        x = inner.copy()
        x[i][col] = bad
        assert _sweep_rc(tm, rows, off, x, lens) == N.PU_E_ARG
    x = inner.copy()
    x[sco][:3] = (x[sco][4], x[upd][1], x[upd][2])  # x0 = B of a scoring row
    ln = lens.copy()
    ln[sco][:2] = 0.1
    assert _sweep_rc(tm, rows, off, x, ln) == N.PU_E_ARG
    down = off.copy()
    down[len(off) // 2] = off[-1] + 1
    assert _sweep_rc(tm, rows, down, inner, lens) == N.PU_E_ARG
    shifted = off.copy()
    shifted[0] = 1
    assert _sweep_rc(tm, rows, shifted, inner, lens) == N.PU_E_ARG
    assert lib.pu_spr_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(off), None, None, None,
                            None) == N.PU_E_ARG
    assert N.last_error(tm._ctx)
    WE.assert_refused_and_put_back(tm, before, N.PU_E_ARG)
    # a bad inner row in the middle of the sweep that only the walk can find: an update of a
    # tip.  By then nodes are re-oriented; the call returns PU_E_ARG with a message and the
    # context is put back
    x = inner.copy()
    x[upd][0] = sorted(tr.names.values())[0]
    WE.assert_refused_and_put_back(tm, before, _sweep_rc(tm, rows, off, x, lens))
    assert "tip" in N.last_error(tm._ctx)
    # and a bad outer row, as the other walks are tested
    WE.assert_refused_and_put_back(tm, before, _sweep_rc(tm, WE.rows_with_a_bad_last_edge(tm),
                                                         off, inner, lens))
    assert np.array_equal(SPR.spr_scores(tm)[1], SPR.spr_scores(tm)[1])


@pytest.fixture(scope="module")
def searched():
    sp = R.search_problem()
    G = Traversal(sp["G"])
    gen = TreeModel(device=0)
    host = R.simulated_on_host(sp)
    names = sorted(host, key=lambda s: int(s[1:]))
    gen.set_alignment_codes(np.zeros((len(names), 1), dtype=np.uint8), np.eye(4), names)
    gen.set_substitution_model(sp["model"])
    gen.set_rate_model(sp["rm"])
    gen.set_tree(sp["G"])
    gen.initialise()
    states = gen.simulate(R.SEARCH_SITES, seed=sp["seed"])
    tm = TreeModel(device=0)
    tm.set_alignment_codes(states, np.eye(4), names)
    tm.set_substitution_model(sp["model"])
    tm.set_rate_model(sp["rm"])
    tm.set_tree(sp["start"])
    tm.initialise()
    tree, lnl, history = tm.spr_search(keep=R.KEEP)
    return dict(sp=sp, tm=tm, tree=tree, lnl=lnl, history=history, states=states, names=names,
                host=host, n_nodes=G.n_nodes)


def test_search_recovers_the_generating_topology(searched):
    """10 taxa x 2000 DNA sites simulated (TreeModel.simulate, seed spr_reference.SEARCH_SEED)
    down a random tree G; the search starts from G with one subtree moved by >= 3 edges, which
    no single NNI undoes, and ends on G's topology.  The precondition holds on the reference
    alone (tests/test_spr.py::test_search_precondition, run on the CPU): at the start tree's
    lengths after oracle.optimise_sweep the CPU restatement ranks the move back to G first of
    the top 5 pruned subtrees, on the alignment the simulator's specification draws -- which
    is the device's, asserted here."""
    sp, history = searched["sp"], searched["history"]
    for i, n in enumerate(searched["names"]):
        assert np.array_equal(searched["states"][i], searched["host"][n]), n
    assert R.splits(sp["start"]) != R.splits(sp["G"])
    assert R.splits(searched["tree"]) == R.splits(sp["G"])
    moved = [h for h in history if h["move"] is not None]
    assert moved and all(h["after"] > h["before"] + 1e-3 for h in moved)
    lnls = [moved[0]["before"]] + [h["after"] for h in moved]
    assert all(b > a for a, b in zip(lnls, lnls[1:]))
    assert all(h["move"][4] >= 1 and 0 <= h["rank"] < R.KEEP and h["tried"] == h["rank"] + 1
               for h in moved)
    print("search: %s" % [(h["move"], round(h["before"], 3), round(h["after"], 3), h["rank"])
                          for h in history])
    # the model is on the returned tree: a fresh likelihood of it is the search's lnL
    tm = searched["tm"]
    assert tm.likelihood() == searched["lnl"]
    fresh = TreeModel(device=0)
    fresh.set_alignment_codes(searched["states"], np.eye(4), searched["names"])
    fresh.set_substitution_model(sp["model"])
    fresh.set_rate_model(sp["rm"])
    fresh.set_tree(searched["tree"])
    fresh.initialise()
    assert abs(fresh.likelihood() - searched["lnl"]) <= 1e-10 * abs(searched["lnl"])
    assert R.splits(with_lengths(tm.tree, tm.traversal.brlens)) == R.splits(sp["G"])
