"""Phylogenetic placement on the device: k_place_table, k_place_prescore and
k_place_newton through pu_place_prescore, pu_place_refine and pu_place_edge against the CPU
restatement (tests/place_reference.py, itself pinned to the oracle's lnL of the joined tree in
tests/test_place.py).

Each case makes its device calls once (the `run` fixture); the tests below read what it kept."""
import ctypes

import numpy as np
import pytest

import place_reference as R

from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import place as PL
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu

L0, TOL, MAX_ITER, KEEP = 0.1, 1e-8, 50, 5
EPS = np.finfo(float).eps


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


def _queries(prob, rows=None):
    q = dict(prob["queries"])
    if rows is not None:
        q["codes"] = np.ascontiguousarray(q["codes"][rows])
        q["names"] = [q["names"][k] for k in rows]
    return q


def _snapshot(tm, node):
    return dict(lnl=tm.likelihood(), site=tm.sitewise_patterns().copy(),
                parts=tm.node_partials(node))


@pytest.fixture(scope="module", params=sorted(R.CASES))
def run(request, oracle_mod):
    prob = R.problem(request.param)
    if request.param == "binary-8x70-Cmax":
        assert prob["rm"].ncat == N.lib().pu_place_max_cat(2)
    ref = R.Restated(oracle_mod, prob)
    tm = _tm(prob)
    q = _queries(prob)
    nod, par = (int(v) for v in ref.edges[0])
    before = _snapshot(tm, nod)
    # the single-edge calls on a fresh traversal: the root edge, at its length and at another
    edge0 = PL.place_edge(tm, q, nod, par, pendant0=L0, max_iter=0)
    edge_nt = PL.place_edge(tm, q, nod, par, pendant0=L0, tol=TOL, max_iter=MAX_ITER)
    edge_t = PL.place_edge(tm, q, nod, par, length=0.37, pendant0=L0, max_iter=0)
    pre = PL.prescore(tm, q, L0)
    after_pre = _snapshot(tm, nod)
    # the candidates: the device's own KEEP best per query, and the root edge for every query
    chosen = PL.select_candidates(pre["scores"], KEEP)
    cand = sorted(set((e, k) for k, es in enumerate(chosen) for e in es) |
                  set((0, k) for k in range(len(chosen))))
    fine = PL.refine(tm, q, cand, len(pre["edges"]), L0, TOL, MAX_ITER)
    after_fine = _snapshot(tm, nod)
    pre2 = PL.prescore(tm, q, L0)
    fine2 = PL.refine(tm, q, cand, len(pre["edges"]), L0, TOL, MAX_ITER)
    return dict(case=request.param, prob=prob, ref=ref, tm=tm, q=q, before=before, pre=pre,
                pre2=pre2, fine=fine, fine2=fine2, after_pre=after_pre, after_fine=after_fine,
                edge0=edge0, edge_nt=edge_nt, edge_t=edge_t, chosen=chosen)


def _site_lnl(run):
    """The tree's lnL under the queries' site map and weights."""
    ref, site = run["ref"], run["before"]["site"]
    return float(np.dot(ref.sw, site[ref.map]))


def test_prescore_against_the_restatement(run):
    ref, got = run["ref"], run["pre"]
    counts = run["tm"].edge_counts()
    assert got["edges"].tolist() == counts["edges"].tolist() == ref.edges.tolist()
    assert np.array_equal(got["lengths"], counts["lengths"])
    assert np.array_equal(got["lengths"], ref.lengths)
    assert len(got["edges"]) == 2 * len(run["prob"]["names"]) - 3
    want = ref.prescore(L0)
    worst = (np.abs(got["scores"] - want) / np.abs(want)).max()
    print("%s: pre-score [%d][%d] worst relative error %.2e" % ((run["case"],) + want.shape +
                                                               (worst,)))
    assert worst <= 1e-10


def test_all_gap_query_scores_the_tree(run):
    kinds = run["prob"]["kinds"]
    if "gap" not in kinds:
        return
    lnl = _site_lnl(run)
    col = run["pre"]["scores"][:, kinds.index("gap")]
    worst = np.abs(col - lnl).max() / abs(lnl)
    print("%s: all-gap query vs the tree's lnL %.2e" % (run["case"], worst))
    assert worst <= 1e-10
    if run["ref"].prob["queries"]["site_pattern"] is None:
        assert abs(lnl - run["before"]["lnl"]) <= 1e-10 * abs(lnl)


def test_refined_lnl_against_the_restatement(run):
    ref, fine = run["ref"], run["fine"]
    worst = 0.0
    for e, k, l, lnl in zip(fine["edge_num"], fine["query"], fine["pendant"], fine["lnl"]):
        assert R.LO <= l <= R.HI
        want = ref.lnl_at(int(k), int(e), float(l))
        worst = max(worst, abs(lnl - want) / abs(want))
    print("%s: %d refined lnL, worst relative error %.2e, Newton steps %d..%d" % (
        run["case"], len(fine["lnl"]), worst, fine["iters"].min(), fine["iters"].max()))
    assert worst <= 1e-10
    assert fine["iters"].max() <= MAX_ITER


def _sample(fine, n=40):
    """Every candidate of the small cases; of the 65-query case every n-th."""
    idx = np.arange(len(fine["lnl"]))
    return idx if len(idx) <= 60 else idx[::len(idx) // n]


def test_refined_lnl_reaches_the_brent_optimum(run):
    ref, fine = run["ref"], run["fine"]
    worst = -np.inf
    for i in _sample(fine):
        e, k = int(fine["edge_num"][i]), int(fine["query"][i])
        _, best = ref.optimum(k, e, L0)
        worst = max(worst, (best - fine["lnl"][i]) / abs(best))
    print("%s: Brent optimum minus refined lnL over |lnL|, worst %.2e" % (run["case"], worst))
    assert worst <= 1e-8


def test_stopping_rule_and_derivatives(run):
    """At l*: the next Newton step would meet the stopping rule, or l* is on a bound with the
    derivative pointing outward.  Only where the surface is flat -- BOTH derivatives below what
    moves lnL by its tolerance, 1e-10 |lnL| per unit length (and per unit length squared): the
    all-gap query, whose lnL does not depend on l, so that d1 / d2 is a quotient of rounding
    errors -- is neither asked.  Every candidate of the small cases is checked; of the 65-query
    case (356 candidates) every eighth (`_sample`), here and in the Brent test, to keep the
    restatement's share of the test within seconds.  derivs_out against
    differences of the restatement: steps H1 = 1e-6 (tests/test_counts.py's) and H2 = 1e-4;
    bound: 3.96e-7 (test_counts.py's) of the value plus the rounding of the differences, 4 eps
    |lnL| / 2 H1 and 16 eps |lnL| / H2^2 (four lnL values of relative error eps each), plus for
    d2 its truncation term, bounded by H2 |d2|."""
    ref, fine = run["ref"], run["fine"]
    worst1 = worst2 = 0.0
    for i in _sample(fine):
        e, k, l = int(fine["edge_num"][i]), int(fine["query"][i]), float(fine["pendant"][i])
        lnl, (d1, d2) = abs(fine["lnl"][i]), fine["derivs"][i]
        flat = 1e-10 * lnl
        assert ((d2 < 0 and abs(d1 / d2) <= TOL * (1 + l)) or (l == R.LO and d1 <= flat) or
                (l == R.HI and d1 >= -flat) or (abs(d1) <= flat and abs(d2) <= flat)), \
            (e, k, l, d1, d2)
        f1, f2 = ref.fd_derivs(k, e, l)
        tol1 = 3.96e-7 * abs(f1) + 4 * EPS * lnl / (2 * R.H1)
        tol2 = (3.96e-7 + R.H2) * abs(f2) + 16 * EPS * lnl / R.H2 ** 2
        worst1, worst2 = max(worst1, abs(d1 - f1) / tol1), max(worst2, abs(d2 - f2) / tol2)
    print("%s: derivatives vs differences, worst error over its bound: d1 %.2e, d2 %.2e" % (
        run["case"], worst1, worst2))
    assert worst1 <= 1 and worst2 <= 1


def test_best_edge_of_the_planted_queries(run):
    """Every planted query tests/test_place.py proved decided: the best refined edge is the
    planted one and a tip copy ends on the lower bound."""
    prob, fine, pre = run["prob"], run["fine"], run["pre"]
    for q, edge in sorted(prob["planted"].items()):
        rows = [i for i in range(len(fine["lnl"])) if fine["query"][i] == q and
                fine["edge_num"][i] in run["chosen"][q]]
        best = max(rows, key=lambda i: (fine["lnl"][i], -fine["edge_num"][i]))
        assert tuple(int(v) for v in pre["edges"][fine["edge_num"][best]]) == edge, (q, edge)
        if prob["kinds"][q].startswith("copy"):
            assert fine["pendant"][best] <= 1e-7


def test_single_edge_call(run):
    pre, fine, ref = run["pre"], run["fine"], run["ref"]
    e0, nt, et = run["edge0"], run["edge_nt"], run["edge_t"]
    Q = len(run["q"]["codes"])
    assert np.array_equal(e0["score"], pre["scores"][0])
    assert np.array_equal(e0["lnl"], e0["score"]) and np.all(e0["pendant"] == L0)
    assert np.array_equal(nt["score"], pre["scores"][0])
    rows = [i for i in range(len(fine["lnl"])) if fine["edge_num"][i] == 0]
    assert [int(fine["query"][i]) for i in rows] == list(range(Q))
    assert np.array_equal(nt["lnl"], fine["lnl"][rows])
    assert np.array_equal(nt["pendant"], fine["pendant"][rows])
    assert np.array_equal(nt["derivs"], fine["derivs"][rows])
    # at another length, against the restatement on the post-order partials
    nod, par = (int(v) for v in ref.edges[0])
    P, S = ref.post
    mid = ref.midpoint(0, 0.37, (P[nod], S[nod], P[par], S[par]))
    for k in (range(Q) if Q <= 9 else (0, 7, Q - 1)):
        want = ref.lnl_at(k, 0, L0, mid)
        assert abs(et["score"][k] - want) <= 1e-10 * abs(want)


def test_repeat_is_bitwise_and_state_unchanged(run):
    assert np.array_equal(run["pre"]["scores"], run["pre2"]["scores"])
    for key in ("pendant", "lnl", "derivs", "iters"):
        assert np.array_equal(run["fine"][key], run["fine2"][key]), key
    b4 = run["before"]
    for af in (run["after_pre"], run["after_fine"]):
        assert af["lnl"] == b4["lnl"]
        assert np.array_equal(af["site"], b4["site"])
        for x, y in zip(b4["parts"], af["parts"]):
            assert np.array_equal(x, y)


def test_scores_do_not_depend_on_the_number_of_queries(run):
    if "chunks" not in run["case"]:
        return
    q1 = _queries(run["prob"], [7])
    assert q1["codes"].shape[1] > 2 * 2048 and q1["codes"].shape[1] % 2048
    tm = run["tm"]
    one = PL.prescore(tm, q1, L0)
    assert np.array_equal(one["scores"][:, 0], run["pre"]["scores"][:, 7])
    cand = [(int(e), 0) for e in run["chosen"][7]]
    fine1 = PL.refine(tm, q1, cand, len(one["edges"]), L0, TOL, MAX_ITER)
    fine = run["fine"]
    rows = [i for i in range(len(fine["lnl"])) if fine["query"][i] == 7 and
            fine["edge_num"][i] in run["chosen"][7]]
    assert np.array_equal(fine1["edge_num"], fine["edge_num"][rows])
    for key in ("pendant", "lnl", "derivs", "iters"):
        assert np.array_equal(fine1[key], fine[key][rows]), key


def test_end_to_end_against_the_joined_tree(run):
    """The three best (query, edge) of the 14-taxon case among the planted queries (the
    all-gap query's lnL is the tree's own at any edge): the refined lnL is the device's own lnL
    of the joined tree on the alignment extended by the query."""
    if run["case"] != "dna-coded-14x700-C4":
        return
    prob, fine, pre = run["prob"], run["fine"], run["pre"]
    q = run["q"]
    real = [i for i in np.argsort(-fine["lnl"], kind="stable") if fine["query"][i] in prob["planted"]]
    for i in real[:3]:
        e, k = int(fine["edge_num"][i]), int(fine["query"][i])
        tree = PL.attach(prob["tree"], pre["edges"][e], "query", float(fine["pendant"][i]))
        tm = TreeModel(device=0)
        tm.set_alignment_partials(
            np.concatenate([prob["table"][prob["codes"]], q["table"][q["codes"][k]][None]]),
            list(prob["names"]) + ["query"], prob["weights"])
        tm.set_substitution_model(prob["model"])
        tm.set_rate_model(prob["rm"])
        tm.set_tree(tree)
        tm.initialise()
        lnl = tm.likelihood()
        print("query %d at edge %d: refined %.10f, joined tree %.10f" % (k, e, fine["lnl"][i], lnl))
        assert abs(fine["lnl"][i] - lnl) <= 1e-10 * abs(lnl)


def test_place_and_treemodel_forward(run):
    if run["case"] != "dna-8x65-C3":
        return
    tm, q = run["tm"], run["q"]
    res = tm.place((q["names"], q["codes"], q["table"]), keep=3, pendant0=L0)
    assert np.array_equal(res["prescore"], run["pre"]["scores"])
    assert res["names"] == q["names"] and len(res["placements"]) == len(q["names"])
    for k, rows in enumerate(res["placements"]):
        assert [r["edge_num"] for r in sorted(rows, key=lambda r: r["edge_num"])] == \
            sorted(run["chosen"][k][:3])
        assert abs(sum(r["lwr"] for r in rows) - 1) <= 1e-12
        assert all(a["lnl"] >= b["lnl"] for a, b in zip(rows, rows[1:]))
        assert all(r["distal"] == 0.5 * res["lengths"][r["edge_num"]] for r in rows)


def test_refusals():
    lib = N.lib()
    prob = R.problem("dna-8x65-C3")
    q = _queries(prob)

    def calls(tm, q, l0=L0, length=0.2, cand_off=None, cand_query=None, cap=None):
        """The return codes of the three calls."""
        rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
        Q, full = len(q["codes"]), 2 * len(tm.names) - 3
        n = full if cap is None else cap  # edges cand_off holds; the pre-score's buffers are full
        args = PL._query_args(q)
        left, right = (int(v) for v in tm.traversal.root_edge)
        out = [np.zeros(Q) for _ in range(3)] + [np.zeros((Q, 2))]
        rc_edge = lib.pu_place_edge(tm._ctx, left, right, length, *args, l0, TOL, MAX_ITER,
                                    *[N.ptr(a) for a in out])
        edges, lens, sc, cnt = (np.zeros((full, 2), dtype=np.int32), np.zeros(full),
                                np.zeros((full, Q)), ctypes.c_int())
        rc_pre = lib.pu_place_prescore(tm._ctx, len(rows), N.ptr(rows), *args, l0, N.ptr(edges),
                                       N.ptr(lens), N.ptr(sc), ctypes.byref(cnt))
        off = np.arange(n + 1, dtype=np.int64) if cand_off is None else cand_off
        cq = np.zeros(max(int(off[-1]), 1), dtype=np.int32) if cand_query is None else cand_query
        m = len(cq)
        res = [np.zeros(m), np.zeros(m), np.zeros((m, 2)), np.zeros(m, dtype=np.int32)]
        rc_fine = lib.pu_place_refine(tm._ctx, len(rows), N.ptr(rows), *args, l0, TOL, MAX_ITER,
                                      n, N.ptr(off), N.ptr(cq), *[N.ptr(a) for a in res])
        return rc_edge, rc_pre, rc_fine

    assert lib.pu_place_max_cat(3) == N.PU_E_ARG
    kmax = lib.pu_place_max_cat(20)
    assert 4 <= kmax < 64
    # more categories than the table kernel's LDS holds
    m, rm = SM.LG(), GammaRateModel(kmax + 1, 0.8)
    tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
    big = dict(tree=tree, names=names, codes=st.astype(np.uint8), table=np.eye(20), model=m,
               rm=rm, compact=True, weights=np.ones(70))
    tm = _tm(big)
    lnl0 = tm.likelihood()
    qa = dict(names=["q"], codes=np.zeros((1, 70), dtype=np.uint8), table=np.eye(20),
              site_pattern=None, site_weight=None)
    assert calls(tm, qa) == (N.PU_E_ARG,) * 3
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
        PL.prescore(tm, qa, L0)
    assert tm.likelihood() == lnl0
    # an LNL_ONLY context, host matrices, the ascertainment correction
    assert calls(_tm(prob, keep=False), q) == (N.PU_E_STATE,) * 3
    with pytest.raises(ValueError, match="keep_partials"):
        PL.prescore(_tm(prob, keep=False), q, L0)
    tm = _tm(dict(prob, model=SM.Strsym(), rm=UniformRateModel()))
    assert calls(tm, q) == (N.PU_E_STATE,) * 3
    with pytest.raises(ValueError, match="reversible"):
        PL.prescore(tm, q, L0)
    tm = _tm(prob)
    tm.set_ascertainment_bias_correction()
    tm.initialise()
    assert calls(tm, q) == (N.PU_E_STATE,) * 3
    # arguments
    tm = _tm(prob)
    lnl0 = tm.likelihood()
    assert calls(tm, q) == (0, 0, 0)
    bad = dict(q, codes=q["codes"].copy())
    bad["codes"][1, 64] = len(q["table"])
    assert calls(tm, bad) == (N.PU_E_ARG,) * 3
    S = q["codes"].shape[1]
    short = dict(q, codes=np.ascontiguousarray(q["codes"][:, :S - 1]))
    assert calls(tm, short) == (N.PU_E_ARG,) * 3  # n_sites != patterns without a map
    mapped = dict(short, site_pattern=np.arange(S - 1, dtype=np.int32), site_weight=None)
    assert calls(tm, mapped) == (0, 0, 0)
    for entry in (-1, S):
        off_map = dict(mapped, site_pattern=mapped["site_pattern"].copy())
        off_map["site_pattern"][3] = entry
        assert calls(tm, off_map) == (N.PU_E_ARG,) * 3
    assert calls(tm, dict(q, table=np.ones((33, 4)))) == (N.PU_E_ARG,) * 3
    for l0 in (0.0, -0.1, float("nan"), float("inf")):
        assert calls(tm, q, l0=l0) == (N.PU_E_ARG,) * 3
    for length in (0.0, -1.0, float("nan"), float("inf")):
        assert calls(tm, q, length=length)[0] == N.PU_E_ARG
    n = 2 * len(tm.names) - 3
    Q = len(q["codes"])
    off = np.arange(n + 1, dtype=np.int64)
    assert calls(tm, q, cand_off=off, cand_query=np.full(n, Q, dtype=np.int32))[2] == N.PU_E_ARG
    assert calls(tm, q, cand_off=off, cand_query=np.full(n, -1, dtype=np.int32))[2] == N.PU_E_ARG
    down = off.copy()
    down[5] = 3
    assert calls(tm, q, cand_off=down)[2] == N.PU_E_ARG
    assert calls(tm, q, cap=n - 1)[2] == N.PU_E_ARG  # more edges in the rows than cand_off holds
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    args = PL._query_args(q)
    assert lib.pu_place_prescore(tm._ctx, len(rows), N.ptr(rows), *args, L0, None, None, None,
                                 None) == N.PU_E_ARG
    assert lib.pu_place_prescore(tm._ctx, len(rows), N.ptr(rows), Q, S, None, None, None, 16,
                                 None, L0, None, None, None, None) == N.PU_E_ARG
    assert tm.likelihood() == lnl0


def test_an_error_in_mid_walk_puts_the_context_back():
    """The last edge's PAR is replaced by a node that is not its neighbour: the walk has then
    re-oriented nodes, the call returns PU_E_ARG, and the context's lnL, sitewise lnL and
    partials are those of pu_run again."""
    lib = N.lib()
    prob = R.problem("dna-8x65-C3")
    q = _queries(prob)
    tm = _tm(prob)
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    last = max(i for i in range(len(rows)) if rows[i][3] >= 0)
    nod, par = int(rows[last][3]), int(rows[last][4])
    before = _snapshot(tm, par)
    bad = rows.copy()
    bad[last][4] = next(v for v in range(tm.traversal.n_nodes) if v not in (nod, par) and
                        (min(v, nod), max(v, nod)) not in tm.traversal.brlens)
    n, Q = 2 * len(tm.names) - 3, len(q["codes"])
    edges, lens, sc, cnt = (np.zeros((n, 2), dtype=np.int32), np.zeros(n), np.zeros((n, Q)),
                            ctypes.c_int())
    args = PL._query_args(q)
    assert lib.pu_place_prescore(tm._ctx, len(rows), N.ptr(bad), *args, L0, N.ptr(edges),
                                 N.ptr(lens), N.ptr(sc), ctypes.byref(cnt)) == N.PU_E_ARG
    off, cq = np.arange(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    res = [np.zeros(n), np.zeros(n), np.zeros((n, 2)), np.zeros(n, dtype=np.int32)]
    assert lib.pu_place_refine(tm._ctx, len(rows), N.ptr(bad), *args, L0, TOL, MAX_ITER, n,
                               N.ptr(off), N.ptr(cq), *[N.ptr(a) for a in res]) == N.PU_E_ARG
    assert N.last_error(tm._ctx)
    tm._site_valid = True
    after = _snapshot(tm, par)
    assert after["lnl"] == before["lnl"] and np.array_equal(after["site"], before["site"])
    for x, y in zip(before["parts"], after["parts"]):
        assert np.array_equal(x, y)
