"""Every copy of the branch-length Newton rule on the device against one traced restatement
(tests/newton_reference.py) on inputs that force the safeguard branches: both
clamps, a start on a bound, an overshoot that is halved, the non-concave halving, max_iter = 0,
1, 2 (tests/newton_cases.py: 8 taxa, DNA GTR + Gamma4 on 130 weighted patterns, protein LG +
Gamma4 on 97).

Per scenario the reference trace is recomputed from the CPU oracle and two conditions on the
INPUT are asserted first: the trace takes the branch the scenario is for, and every decision of
it has a margin (1e-9 |lnL| for an lnL comparison; for a sign test 1e-6 of the largest tested
|d| and 1e-9 |lnL|) that the copies' rounding differences (about 1e-16 per site) cannot cross.  Then, per
copy: the iteration (or evaluation) count is the reference's, the length within 1e-9 max(t, 1e-3)
-- on a bound, the bound itself -- and lnL within 1e-10 relative (DESIGN 4.19's device-versus-
restatement bound).

No `expand` scenario (d1 > 0, d2 >= 0): 400 log-spaced lengths in [1e-8, 100] of every edge of
the tree on every data set, of the three arrangements' central lengths and of the queries'
pendant lengths were scanned on the CPU oracle and none had it; the closed-form case of
tests/test_newton_reference.py is its only cover.  Likewise `gave_up` (30 halvings).  A
non-finite lnL is given to the host loop alone (test_host_loop_stops_on_a_non_finite_lnl).
k_edge_newton runs with C = 4 and with C = 1; under one rate `overshoot`, `upper` and
`upper-start` cannot keep the conditions (tests/newton_cases.py, C1_SCENARIOS, says why for
each) and the other seven scenarios run.

No device scenario joins a safeguard branch to the dt <= tol (1 + t) exit: a run that converges
ends on steps that gain less than 1e-13 |lnL|, which no lnL margin survives, so `overshoot` and
`shrink` are cut after 3 steps and end on `max_iter`.  (`lower` under one rate does end on
`converged`, after the clamp.)  That pairing is covered by the closed-form cases alone.

Measured (MI355X), worst length error over max(t, 1e-3) / worst relative lnL error: host loop
1.3e-15 / 1.9e-15, k_edge_newton 9.1e-15 / 6.2e-16, pu_nni_sweep 2.4e-13 / 8.6e-16,
k_place_newton 2.9e-14 / 6.0e-16, site-sharded driver 3.9e-16 / 4.9e-16; every count equal."""
import ctypes

import numpy as np
import pytest

import newton_cases as NC
import newton_reference as NT
import place_reference as PR
from test_gpu_edges import _newton_stats

from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import place as PL
from phylo_utils_amd.parallel import SiteShardedLikelihood, gpu_engine

pytestmark = pytest.mark.gpu

X_SCENARIOS = sorted(s for s in NC.SCENARIOS if NC.SCENARIOS[s][1] == "X")


def _tm(case):
    tm = TreeModel(device=0)
    tm.set_alignment_codes(np.asarray(case.codes), case.table, NC.NAMES,
                           np.asarray(case.weights))
    tm.set_substitution_model(case.model)
    tm.set_rate_model(case.rm)
    tm.set_tree(case.newick)
    tm.initialise()
    assert tm.traversal.optimising_traversal.tolist() == case.tr.optimising_traversal.tolist()
    return tm


def _reference(orc, kind, sid, quartet=False):
    case, max_iter, events, end = NC.scenario(orc, kind, sid)
    ev = case.quartet_evaluate(0) if quartet else case.evaluate
    t, lnl, d1, d2, it, trace = NT.newton_trace(ev, case.t0, NC.TOL, max_iter)
    NC.check_conditions(trace, events, (kind, sid))
    assert end is None or t == end
    return case, max_iter, dict(t=t, lnl=lnl, d1=d1, it=it, trace=trace, end=end)


class Worst(object):
    def __init__(self):
        self.t = self.lnl = 0.0

    def check(self, what, t, lnl, ref):
        if ref["end"] is not None:
            assert t == ref["end"], (what, t)
        et = abs(t - ref["t"]) / max(ref["t"], 1e-3)
        el = abs(lnl - ref["lnl"]) / abs(ref["lnl"])
        self.t, self.lnl = max(self.t, et), max(self.lnl, el)
        assert et <= 1e-9, (what, t, ref["t"])
        assert el <= 1e-10, (what, lnl, ref["lnl"])

    def report(self, copy):
        print("%s: worst length error %.2e (of max(t, 1e-3)), worst lnL error %.2e" %
              (copy, self.t, self.lnl))


def _sweep(tm, case, max_iter):
    """pu_optimise_sweep over the rows that stand the walk on the scenario's edge: (length as
    pu_get_branch_lengths stores it, lnL of the closing traversal, Newton iterations)."""
    rows = np.ascontiguousarray(case.rows, dtype=np.int32)
    lnl, n_it = ctypes.c_double(), ctypes.c_int()
    N.check(N.lib().pu_optimise_sweep(tm._ctx, len(rows), N.ptr(rows), NC.TOL, int(max_iter),
                                      ctypes.byref(lnl), ctypes.byref(n_it)), tm._ctx,
            "pu_optimise_sweep")
    tm._pull_lengths()
    return float(tm.traversal.brlens[case.edge]), lnl.value, n_it.value


def _edge_copy(orc, monkeypatch, kind, device, worst):
    monkeypatch.setenv("PU_EDGE_DEVICE_NEWTON", "1" if device else "0")
    for sid in NC.scenarios_of(kind):
        case, max_iter, ref = _reference(orc, kind, sid)
        tm = _tm(case)
        assert tm.rate_model.ncat == (1 if kind == "dna-c1" else 4)
        l0 = _newton_stats(tm)
        t, lnl, it = _sweep(tm, case, max_iter)
        l1 = _newton_stats(tm)
        assert it == ref["it"], (kind, sid, it, ref["it"], ref["trace"].events)
        worst.check((kind, sid), t, lnl, ref)
        if device:  # one persistent launch, all of the trace's evaluations in it, no fall-back
            assert (l1[0] - l0[0], l1[1] - l0[1]) == (1, ref["trace"].evaluations), (sid, l0, l1)
        else:
            assert l1 == l0 == (0, 0)
        # pu_optimise_edge on the same re-oriented partials (pu_update_partials builds its
        # matrices on another path than the sweep's rows: the last bit may differ): the length it
        # returns is the one it stores
        tm2 = _tm(case)
        tm2.update_partials(case.rows[:, :3], [[case.tr.brlens[r[0], r[1]],
                                                case.tr.brlens[r[0], r[2]]] for r in case.rows])
        t2, lnl2 = tm2.optimise_edge(case.edge[0], case.edge[1], tol=NC.TOL, max_iter=max_iter)
        assert t2 == float(tm2.traversal.brlens[case.edge]), (kind, sid, t2)
        worst.check((kind, sid, "pu_optimise_edge"), t2, lnl2, ref)


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_host_loop_takes_the_reference_steps(oracle_mod, monkeypatch, kind):
    """newton() of pu_edge.cpp, one k_edge launch per evaluation (PU_EDGE_DEVICE_NEWTON=0).
    Measured: length 1.3e-15 (DNA), 1.1e-15 (protein); lnL 6.2e-16, 1.9e-15."""
    worst = Worst()
    _edge_copy(oracle_mod, monkeypatch, kind, False, worst)
    worst.report("host loop, %s" % kind)


@pytest.mark.parametrize("kind", ["dna", "dna-c1"])
def test_device_newton_takes_the_reference_steps(oracle_mod, monkeypatch, kind):
    """k_edge_newton, the persistent grid (PU_EDGE_DEVICE_NEWTON=1), DNA with C = 4 and, on the
    scenarios one rate keeps (newton_cases.C1_SCENARIOS), C = 1: one launch per optimisation and
    exactly the reference's evaluations in it (pu_ctx_newton_stats), so no scenario fell back to
    the host loop.  Measured: length 3.2e-15 (C = 4), 9.1e-15 (C = 1); lnL 6.2e-16, 3.6e-16."""
    worst = Worst()
    _edge_copy(oracle_mod, monkeypatch, kind, True, worst)
    worst.report("k_edge_newton, %s" % kind)


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_host_loop_stops_on_a_non_finite_lnl(oracle_mod, monkeypatch, kind):
    """newton()'s exit on a non-finite lnL, on the host loop alone (PU_EDGE_DEVICE_NEWTON=0; the
    persistent grid is given no such input): the `overshoot` input with one pattern of weight 2
    made impossible -- its row zeroed at tips A and E, dense tips as in tests/
    test_gpu_invariant.py.  The reference trace is [start, non_finite]; pu_optimise_sweep and
    pu_optimise_edge report 0 iterations, leave the stored length at the start and return
    lnL = -inf."""
    monkeypatch.setenv("PU_EDGE_DEVICE_NEWTON", "0")
    case, max_iter, _, _ = NC.scenario(oracle_mod, kind, "overshoot")
    w = np.array(case.weights)
    hit = int(np.flatnonzero(w > 0)[3])
    w[hit] = 2.0
    part = case.table[np.asarray(case.codes)].copy()
    part[NC.NAMES.index("A"), hit] = part[NC.NAMES.index("E"), hit] = 0.0
    tips = {case.tr.names[n]: part[i] for i, n in enumerate(NC.NAMES)}
    st = NT.oracle_state(oracle_mod, tips, case.tr, case.e, w)
    P, S, rows = NT.walk_to(oracle_mod, st, case.tr, case.e, case.edge)
    assert rows.tolist() == case.rows.tolist()
    with np.errstate(all="ignore"):
        t, lnl, _, _, it, trace = NT.newton_trace(
            NT.edge_evaluate(oracle_mod, P, S, case.edge[0], case.edge[1], case.e, w), case.t0,
            NC.TOL, max_iter)
    assert trace.events == ["start", "non_finite"] and (t, lnl, it) == (case.t0, -np.inf, 0)

    def tm_of():
        tm = TreeModel(device=0, compact_tips=False)
        tm.set_alignment_partials(part, NC.NAMES, w)
        tm.set_substitution_model(case.model)
        tm.set_rate_model(case.rm)
        tm.set_tree(case.newick)
        tm.initialise()
        assert tm.traversal.optimising_traversal.tolist() == \
            case.tr.optimising_traversal.tolist()
        return tm

    tm = tm_of()
    assert _sweep(tm, case, max_iter) == (case.t0, -np.inf, 0)
    assert _newton_stats(tm) == (0, 0)
    tm2 = tm_of()
    tm2.update_partials(case.rows[:, :3], [[case.tr.brlens[r[0], r[1]],
                                            case.tr.brlens[r[0], r[2]]] for r in case.rows])
    assert tm2.optimise_edge(case.edge[0], case.edge[1], tol=NC.TOL, max_iter=max_iter) == \
        (case.t0, -np.inf)
    assert float(tm2.traversal.brlens[case.edge]) == case.t0


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_quartet_newton_takes_the_reference_steps(oracle_mod, kind):
    """struct Newton of pu_nni.hip through pu_nni_sweep (nni_scores): arrangement 0 of the
    quartet around the scenario's edge, from the standing length.  The ABI reports evaluations,
    not iterations: they are the trace's.  Measured: length 3.3e-14 (DNA), 2.4e-13 (protein);
    lnL 8.6e-16, 4.0e-16."""
    worst = Worst()
    for sid in X_SCENARIOS:
        case, max_iter, ref = _reference(oracle_mod, kind, sid, quartet=True)
        tm = _tm(case)
        quartets, scores = tm.nni_scores(tol=NC.TOL, max_iter=max_iter)
        i = [tuple(q[:2]) for q in quartets.tolist()].index(case.edge)
        assert tuple(quartets[i][2:]) == case.quartet()[0]
        t, lnl, d1, evals = scores[i][0]
        assert int(evals) == ref["trace"].evaluations, (kind, sid, evals, ref["trace"].events)
        worst.check((kind, sid), float(t), float(lnl), ref)
        assert abs(d1 - ref["d1"]) <= 1e-10 * max(1.0, abs(ref["d1"]))
    worst.report("pu_nni_sweep, %s" % kind)


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_pendant_newton_takes_the_reference_steps(oracle_mod, kind):
    """k_place_newton through pu_place_refine (root edge and edge X: iterations, length, lnL,
    derivatives) and pu_place_edge (root edge: length, lnL, derivatives).  Measured: length
    2.9e-14 (DNA), 1.8e-14 (protein); lnL 6.0e-16, 5.4e-16."""
    prob = NC.place_problem(kind)
    ref_walk = PR.Restated(oracle_mod, prob)
    k = NC.place_edge_number(ref_walk)
    tm = TreeModel(device=0)
    tm.set_alignment_codes(prob["codes"], prob["table"], prob["names"], prob["weights"])
    tm.set_substitution_model(prob["model"])
    tm.set_rate_model(prob["rm"])
    tm.set_tree(prob["tree"])
    tm.initialise()
    q = prob["queries"]
    worst = Worst()
    for sid in sorted(NC.PLACE_SCENARIOS):
        qi, start, max_iter, events, end = NC.PLACE_SCENARIOS[sid]
        l0 = NC.STARTS[kind][start]
        refs = {}
        for kk in (0, k):
            t, lnl, d1, d2, it, trace = NT.newton_trace(
                NT.pendant_evaluate(oracle_mod, ref_walk, qi, kk), l0, NC.TOL, max_iter)
            NC.check_conditions(trace, events, (kind, sid, kk))
            refs[kk] = dict(t=t, lnl=lnl, d1=d1, d2=d2, it=it, end=end)
        if max_iter > 0:  # with max_iter = 0 pu_place_edge returns the pre-score alone
            nod, par = (int(v) for v in ref_walk.edges[0])
            one = PL.place_edge(tm, q, nod, par, pendant0=l0, tol=NC.TOL, max_iter=max_iter)
            worst.check((kind, sid, "pu_place_edge"), float(one["pendant"][qi]),
                        float(one["lnl"][qi]), refs[0])
            for got, want in zip(one["derivs"][qi], (refs[0]["d1"], refs[0]["d2"])):
                assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (kind, sid, "place_edge")
        fine = PL.refine(tm, q, [(0, qi), (k, qi)], len(ref_walk.edges), l0, NC.TOL, max_iter)
        for row, kk in enumerate((0, k)):
            r = refs[kk]
            assert int(fine["iters"][row]) == r["it"], (kind, sid, kk, fine["iters"][row], r["it"])
            worst.check((kind, sid, kk), float(fine["pendant"][row]), float(fine["lnl"][row]), r)
            if max_iter > 0:
                for got, want in zip(fine["derivs"][row], (r["d1"], r["d2"])):
                    assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (kind, sid, kk)
    worst.report("k_place_newton, %s" % kind)


def test_site_sharded_driver_takes_the_reference_steps(oracle_mod, monkeypatch):
    """parallel.newton_edge inside SiteShardedLikelihood.optimise_branch_lengths on one rank
    over the GPU engine, its walk cut to the rows that stand it on the scenario's edge:
    `lower`, `upper`, `overshoot`.  The driver reports evaluations: they are the trace's.
    Measured: length 3.9e-16, lnL 4.9e-16."""
    monkeypatch.setenv("PU_EDGE_DEVICE_NEWTON", "0")
    worst = Worst()
    for sid in ("lower", "upper", "overshoot"):
        case, max_iter, ref = _reference(oracle_mod, "dna", sid)
        sh = SiteShardedLikelihood(case.newick, np.asarray(case.codes), case.table, NC.NAMES,
                                   case.model, case.rm, siteweights=np.asarray(case.weights),
                                   engine_factory=gpu_engine(0))
        tr = sh.engine.traversal
        assert tr.optimising_traversal.tolist() == case.tr.optimising_traversal.tolist()
        # the driver walks this attribute: cut to the rows up to the scenario's edge, it
        # optimises that edge alone, from the partials the reference stands on
        tr.optimising_traversal = case.rows
        lnl = sh.optimise_branch_lengths(tol=NC.TOL, max_iter=max_iter)
        assert sh.last_evaluations == ref["trace"].evaluations, (sid, sh.last_evaluations)
        # tr.brlens is the driver's own table; that the engine got the length shows in lnl,
        # the engine's closing traversal
        worst.check(("sharded", sid), float(tr.brlens[case.edge]), lnl, ref)
    worst.report("site-sharded driver")
