"""The traced Newton rule (tests/newton_reference.py) against the library's Python copy
(parallel.newton_edge) and the oracle's (oracle.newton_edge, the one nni_reference uses) on
closed-form evaluate functions, each built to take one branch of the rule: the expected events in
order, and (t, lnL, iterations) equal bit for bit.  The functions need not be likelihoods, nor
even have the derivatives they report: the rule sees three numbers per length.  The library's
C++ rule (csrc/pu_newton.h) replays the same runs on the host (tests/newton_check.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

import newton_cases as NC
import newton_reference as NT
import place_reference as PR

from conftest import ROOT
from phylo_utils_amd.parallel import newton_edge

CSRC = os.path.join(ROOT, "phylo_utils_amd", "csrc")
TOL = 1e-8

# a concave lnL falling from 0: the step from 0.1 passes the lower bound, the bound is accepted
# and the next step ends on tn == t
falls_from_0 = lambda t: (-10.0 - t - t * t, -1.0 - 2.0 * t, -2.0)
# a concave lnL rising over the whole range: the step from 0.1 passes the upper bound
rises_to_100 = lambda t: (-10.0 + t - 0.001 * t * t, 1.0 - 0.002 * t, -0.002)
# convex with the minimum at 1: decreasing at 0.5 (halve), increasing at 1.5 (t + 0.1)
convex = lambda t: (-10.0 + (t - 1.0) ** 2, 2.0 * (t - 1.0), 2.0)
# the optimum at 0.09 with the curvature understated 1000-fold: from 0.1 the step lands on the
# lower bound; 1e-8 and the halvings near 0.05 and 0.075 are lower than the start, the one near
# 0.0875 is higher
understated = lambda t: (-10.0 - (t - 0.09) ** 2, -2.0 * (t - 0.09), -2e-3)
HALVINGS = [1e-8]
for _ in range(3):
    HALVINGS.append(0.5 * (0.1 + HALVINGS[-1]))
# a concave quadratic: one Newton step lands on the optimum at 0.3, the next is no step
quadratic = lambda t: (-10.0 - (t - 0.3) ** 2, -2.0 * (t - 0.3), -2.0)
# concave, no quadratic: plain Newton steps towards the optimum at 0.3 until dt <= tol (1 + t)
smooth = lambda t: (-10.0 + 0.3 * math.log(t) - t, 0.3 / t - 1.0, -0.3 / (t * t))
# -inf everywhere
minus_inf = lambda t: (-math.inf, 0.0, 0.0)


def jitter(t0):
    """Flat to rounding: 2e-13 relative (above the 1e-13 slack) higher at the start than at any
    other length, as a sum over many sites may round; d1 > 0 asks for a step of 1."""
    return lambda t: (-1e4 + (2e-9 if t == t0 else 0.0), 1.0, -1.0)


CASES = {
    "optimum-at-0": (falls_from_0, 0.1, 50,
                     ["start", "newton", "clamp_lo", "accept", "newton", "clamp_lo", "stall"],
                     (1e-8, 1)),
    "start-below-the-bound": (falls_from_0, 0.0, 50,
                              ["clamp_lo", "start", "newton", "clamp_lo", "stall"], (1e-8, 0)),
    "rises-to-the-bound": (rises_to_100, 0.1, 50,
                           ["start", "newton", "clamp_hi", "accept", "newton", "clamp_hi",
                            "stall"], (100.0, 1)),
    "start-above-the-bound": (rises_to_100, 250.0, 50,
                              ["clamp_hi", "start", "newton", "clamp_hi", "stall"], (100.0, 0)),
    "convex-decreasing": (convex, 0.5, 1, ["start", "shrink", "accept", "max_iter"], (0.25, 1)),
    "convex-increasing": (convex, 1.5, 1, ["start", "expand", "accept", "max_iter"],
                          (1.5 + 1.5 + 0.1, 1)),
    "overshoot-3-halvings": (understated, 0.1, 1,
                             ["start", "newton", "clamp_lo", "reject", "reject", "reject",
                              "accept", "max_iter"], (HALVINGS[3], 1)),
    "flat-gives-up": (jitter(0.25), 0.25, 50,
                      ["start", "newton"] + ["reject"] * 30 + ["gave_up"], (0.25, 0)),
    "minus-inf": (minus_inf, 0.1, 50, ["start", "non_finite"], (0.1, 0)),
    "max-iter-0": (quadratic, 0.1, 0, ["start", "max_iter"], (0.1, 0)),
    "stall-on-the-optimum": (quadratic, 0.1, 50,
                             ["start", "newton", "accept", "newton", "stall"], (0.3, 1)),
    "converges": (smooth, 0.2, 50, None, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_closed_form_case_takes_its_branch(oracle_mod, case):
    f, t0, max_iter, events, end = CASES[case]
    calls = [0]

    def counted(t):
        calls[0] += 1
        return f(t)

    t, lnl, d1, d2, it, trace = NT.newton_trace(counted, t0, TOL, max_iter)
    if events is None:  # plain steps, as many as it takes
        events = ["start"] + ["newton", "accept"] * it + ["converged"]
        assert 3 <= it < max_iter and abs(t - 0.3) <= 1e-8
    assert trace.events == events, trace
    assert trace.evaluations == calls[0] == 1 + trace.count("accept") + trace.count("reject")
    assert len(trace.lnl_margins) == trace.count("accept") + trace.count("reject")
    assert (lnl, d1, d2) == f(t)
    if end is not None:
        assert (t, it) == end
    for copy in (newton_edge, oracle_mod.newton_edge):
        calls[0] = 0
        got = copy(counted, t0, TOL, max_iter)
        assert got == (t, lnl, it), (copy.__module__, got, (t, lnl, it))
        assert calls[0] == trace.evaluations


def test_cpp_rule_replays_every_closed_form_case(tmp_path):
    """The C++ rule (csrc/pu_newton.h, the one every driver in the library steps) on the same
    twelve cases, on the host: tests/newton_check.cpp replays each run of the traced reference
    and must name every abscissa the reference evaluated, be done exactly when the reference
    stops, and end on its (t, lnL, d1, d2, iterations, evaluations), all bit for bit."""
    hx = lambda v: float(v).hex()
    lines = []
    for case in sorted(CASES):
        f, t0, max_iter, _, _ = CASES[case]
        seen = []

        def recorded(t):
            seen.append((t,) + tuple(float(v) for v in f(t)))
            return seen[-1][1:]

        t, lnl, d1, d2, it, trace = NT.newton_trace(recorded, t0, TOL, max_iter)
        assert len(seen) == trace.evaluations and (case != "flat-gives-up" or len(seen) == 31)
        lines.append("case %s %s %s %d %d" % (case, hx(t0), hx(TOL), max_iter, len(seen)))
        lines += [" ".join(hx(v) for v in row) for row in seen]
        lines.append("end %s %d %d" % (" ".join(hx(v) for v in (t, lnl, d1, d2)), it, len(seen)))
    script = tmp_path / "newton_cases.txt"
    script.write_text("\n".join(lines) + "\n")
    obj = str(tmp_path / "obj")
    build = subprocess.run(["make", "-C", CSRC, "OBJ=" + obj, "newton_check"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([os.path.join(obj, "newton_check"), str(script)], capture_output=True,
                         text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert len(CASES) == 12 and "12 cases" in run.stdout and " 0 failures" in run.stdout


def test_margins_of_a_trace():
    """The margins of the overshoot case by hand: lnL bar = lnL(0.1) - 1e-13 |lnL(0.1)|, the
    four candidates' distances from it over |lnL(0.1)|; one sign test on d2 = -2e-3 (the same
    at every length: margin 1)."""
    *_, trace = NT.newton_trace(understated, 0.1, TOL, 1)
    l0 = understated(0.1)[0]
    bar = l0 - 1e-13 * abs(l0)
    want = [abs(understated(x)[0] - bar) / abs(l0) for x in HALVINGS]
    assert trace.lnl_margins == want
    assert [round(m * 1e5, 2) for m in want] == [80.0, 15.0, 1.25, 0.94]
    assert trace.sign_tests == [("d2", 2e-3)] and trace.sign_margins == [1.0]
    *_, trace = NT.newton_trace(convex, 0.5, TOL, 2)
    assert trace.sign_tests == [("d2", 2.0), ("d1", 1.0), ("d2", 2.0), ("d1", 1.5)]
    # three lengths evaluated (0.5, 0.25, 0.125): the largest |d1| is 1.75 at the last, which no
    # sign test looked at
    assert trace.seen == [(1.0, 2.0), (1.5, 2.0), (1.75, 2.0)]
    assert trace.sign_margins == [1.0, 1.0 / 1.5, 1.0, 1.0]
    assert trace.sign_margins_all == [1.0, 1.0 / 1.75, 1.0, 1.5 / 1.75]
    l0, l1 = abs(convex(0.5)[0]), abs(convex(0.25)[0])
    assert trace.sign_floors == [2.0 / l0, 1.0 / l0, 2.0 / l1, 1.5 / l1]


def test_pendant_evaluate_is_the_placement_restatement(oracle_mod):
    """newton_reference.pendant_evaluate gives orc.edge_derivs the midpoint vectors of
    place_reference.Restated: its lnL is Restated.lnl_at's (transition matrices, 1e-12) and its
    first derivative the central difference of lnl_at within tests/test_gpu_place.py's bound
    (the derivatives themselves are the oracle's own edge_derivs)."""
    prob = PR.problem("dna-8x65-C3")
    ref = PR.Restated(oracle_mod, prob)
    eps = np.finfo(float).eps
    for q, k in ((0, 0), (1, 3), (1, len(ref.edges) - 1)):
        ev = NT.pendant_evaluate(oracle_mod, ref, q, k)
        for l in (1e-8, 0.02, 0.4, 7.0):
            lnl, d1, d2 = ev(l)
            want = ref.lnl_at(q, k, l)
            assert abs(lnl - want) <= 1e-12 * abs(want), (q, k, l, lnl, want)
            f1, _ = ref.fd_derivs(q, k, l)
            assert abs(d1 - f1) <= 3.96e-7 * abs(f1) + 4 * eps * abs(lnl) / (2 * PR.H1)


@pytest.mark.parametrize("kind", ["dna", "dna-c1", "protein"])
def test_scenarios_take_their_branch(oracle_mod, kind):
    """Every scenario of tests/newton_cases.py on the CPU oracle: the reference trace takes the
    branch the scenario is for, ends where it says, and keeps the decision margins (under one
    rate, "dna-c1", the scenarios that newton_cases.C1_SCENARIOS keeps) -- for the
    edge, for arrangement 0 of the quartet around an internal edge (the same lnL by the pulley
    principle, another evaluate) and for the pendant lengths of the placement scenarios."""
    for sid in NC.scenarios_of(kind):
        case, max_iter, events, end = NC.scenario(oracle_mod, kind, sid)
        evs = [case.evaluate] + ([case.quartet_evaluate(0)] if case.edge_name == "X" else [])
        for ev in evs:
            t, lnl, d1, d2, it, trace = NT.newton_trace(ev, case.t0, NC.TOL, max_iter)
            NC.check_conditions(trace, events, (kind, sid))
            assert end is None or t == end
            if sid.startswith("max-iter"):
                assert it == max_iter
    if kind == "dna-c1":  # the edge copies' second launch shape only
        return
    prob = NC.place_problem(kind)
    ref = PR.Restated(oracle_mod, prob)
    k = NC.place_edge_number(ref)
    for sid in sorted(NC.PLACE_SCENARIOS):
        q, start, max_iter, events, end = NC.PLACE_SCENARIOS[sid]
        for kk in (0, k):
            t, lnl, d1, d2, it, trace = NT.newton_trace(
                NT.pendant_evaluate(oracle_mod, ref, q, kk), NC.STARTS[kind][start], NC.TOL,
                max_iter)
            NC.check_conditions(trace, events, (kind, sid, kk))
            assert end is None or t == end
