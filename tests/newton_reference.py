"""The branch-length Newton rule once more, in plain Python floats, with a trace of every branch
it takes.  The rule is csrc/pu_newton.h's:

* lengths are kept in [1e-8, 100];
* the step is -d1 / d2 where d2 < 0; where d2 >= 0 it is t + 0.1 for d1 > 0 (`expand`), else
  -0.5 t (`shrink`);
* a step is accepted when lnL_new >= lnL - 1e-13 |lnL|, otherwise it is halved, up to 30 times;
* it ends on tn == t (`stall`), dt <= tol (1 + t) (`converged`), it >= max_iter (`max_iter`),
  30 halvings (`gave_up`) or a non-finite lnL (`non_finite`).

``newton_trace`` is what the tests hold every copy of the rule against; the ``*_evaluate``
functions build its evaluate(t) -> (lnL, d1, d2) from the CPU oracle's own ``edge_derivs`` on the
ends the existing restatements give (tests/test_gpu_edges.py's oracle state, nni_reference's
quartet ends, place_reference's midpoint) -- no likelihood is written here.  `orc` is the oracle
module (the ``oracle_mod`` fixture)."""
import math

import numpy as np

MIN_LEN, MAX_LEN = 1e-8, 100.0
SLACK = 1e-13
MAX_HALVINGS = 30
EVENTS = ("start", "newton", "expand", "shrink", "clamp_lo", "clamp_hi", "reject", "accept",
          "stall", "converged", "max_iter", "gave_up", "non_finite")


class Trace(list):
    """The events [(name, t)] in order.  ``lnl_margins``: for every accept / reject,
    |lnL_new - (lnL - 1e-13 |lnL|)| / |lnL|.  ``sign_tests``: [(which, |d|)] of every sign test
    on d2 (each planned step) and d1 (where d2 >= 0).  ``sign_margins`` relates them to the largest
    tested |d2| (|d1|), ``sign_margins_all`` to the largest of all the lengths the trace evaluated
    (``seen``), the rejected ones included -- a step rejected on the lower bound has |d2| of
    1 / t^2 size there, which says nothing about the rounding of a tested derivative.
    ``sign_floors``: the tested |d| over |lnL| at the same length, an absolute measure: d1, d2 and
    lnL are sums over the same sites, so the copies' rounding differences in them are of one
    size.  ``evaluations``: calls of evaluate."""

    def __init__(self):
        list.__init__(self)
        self.lnl_margins = []
        self.sign_tests = []
        self.sign_floors = []
        self.seen = []
        self.evaluations = 0

    def add(self, name, t):
        assert name in EVENTS
        self.append((name, float(t)))

    def saw(self, r):
        self.evaluations += 1
        self.seen.append((abs(r[1]), abs(r[2])))

    @property
    def events(self):
        return [name for name, _ in self]

    @property
    def sign_margins(self):
        top = {w: max([d for v, d in self.sign_tests if v == w and math.isfinite(d)] + [0.0])
               for w in ("d1", "d2")}
        return [d / top[w] if top[w] > 0 else 0.0 for w, d in self.sign_tests]

    @property
    def sign_margins_all(self):
        top = {w: max([d[i] for d in self.seen if math.isfinite(d[i])] + [0.0])
               for i, w in enumerate(("d1", "d2"))}
        return [d / top[w] if top[w] > 0 else 0.0 for w, d in self.sign_tests]

    def count(self, name):
        return self.events.count(name)


def newton_trace(evaluate, t0, tol, max_iter):
    """(t, lnL, d1, d2, iterations, trace) of the rule from t0 over evaluate(t) -> (lnL, d1, d2)."""
    tr = Trace()
    t = float(t0)
    if t < MIN_LEN:
        t = MIN_LEN
        tr.add("clamp_lo", t)
    elif t > MAX_LEN:
        t = MAX_LEN
        tr.add("clamp_hi", t)
    tr.add("start", t)
    r = tuple(float(x) for x in evaluate(t))
    tr.saw(r)
    it = 0
    while True:
        if it >= max_iter:
            tr.add("max_iter", t)
            break
        lnl, d1, d2 = r
        if not math.isfinite(lnl):
            tr.add("non_finite", t)
            break
        tr.sign_tests.append(("d2", abs(d2)))
        tr.sign_floors.append(abs(d2) / abs(lnl) if lnl != 0 else math.inf)
        if d2 < 0.0:
            step = -d1 / d2
            tr.add("newton", t)
        else:
            tr.sign_tests.append(("d1", abs(d1)))
            tr.sign_floors.append(abs(d1) / abs(lnl) if lnl != 0 else math.inf)
            if d1 > 0.0:
                step = t + 0.1
                tr.add("expand", t)
            else:
                step = -0.5 * t
                tr.add("shrink", t)
        tn = t + step
        if tn < MIN_LEN:
            tn = MIN_LEN
            tr.add("clamp_lo", tn)
        elif tn > MAX_LEN:
            tn = MAX_LEN
            tr.add("clamp_hi", tn)
        if tn == t:
            tr.add("stall", t)
            break
        ok = False
        for _ in range(MAX_HALVINGS):
            rn = tuple(float(x) for x in evaluate(tn))
            tr.saw(rn)
            bar = lnl - SLACK * abs(lnl)
            tr.lnl_margins.append(abs(rn[0] - bar) / abs(lnl) if math.isfinite(rn[0]) and lnl != 0
                                  else math.inf)
            if rn[0] >= bar:
                ok = True
                tr.add("accept", tn)
                break
            tr.add("reject", tn)
            tn = 0.5 * (t + tn)
        if not ok:
            tr.add("gave_up", t)
            break
        dt = abs(tn - t)
        t, r = tn, rn
        it += 1
        if dt <= tol * (1.0 + t):
            tr.add("converged", t)
            break
    return t, r[0], r[1], r[2], it, tr


# ------------------------------------------------------------------ evaluate(t) from the oracle
def oracle_state(orc, tips, tr, e, site_weights=None):
    """tests/test_gpu_edges.py's _oracle_state with pattern weights: the post-order partials."""
    return orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                        tr.root_length(), e["evecs"], e["evals"], e["ivecs"], e["freqs"],
                        e["rates"], e["weights"], site_weights=site_weights, n_nodes=tr.n_nodes,
                        return_all=True)


def walk_to(orc, st, tr, e, edge):
    """The oracle's partials as the optimising traversal holds them when it stands on `edge` =
    (NOD, PAR): its re-orientation and restore rows up to and including the edge's own applied to
    copies of st's partials.  Returns (P, S, rows sent [n][5])."""
    P, S = st["partials"].copy(), st["scale"].copy()
    pm = lambda t: orc.pmatrix(e["evecs"], e["evals"], e["ivecs"], t, e["rates"])
    sent = []
    for row in tr.optimising_traversal:
        here = (int(row[3]), int(row[4])) == tuple(int(v) for v in edge)
        if row[0] >= 0:
            p, x, y = (int(v) for v in row[:3])
            cml = np.zeros(S[p].shape)
            P[p] = orc.clv_c(pm(tr.brlens[p, x]), pm(tr.brlens[p, y]), P[x], P[y], S[x], S[y], cml)
            S[p] = cml
            if not here:
                sent.append((p, x, y, -1, -1))
        if here:
            sent.append(tuple(int(v) for v in row))
            return P, S, np.array(sent, dtype=np.int32).reshape(-1, 5)
    raise ValueError("the optimising traversal has no row for edge %r" % (edge,))


def edge_evaluate(orc, P, S, a, b, e, site_weights=None):
    """evaluate(t) of edge (a, b) on partials P, scalers S: the derivative restatement of
    tests/test_gpu_edges.py (orc.edge_derivs: P(0) on a, P(t) on b)."""
    return lambda t: tuple(orc.edge_derivs(P[a], S[a], P[b], S[b], e["evecs"], e["evals"],
                                           e["ivecs"], t, e["rates"], e["weights"], e["freqs"],
                                           site_weights))


def quartet_evaluate(orc, P, S, nodes, lens, k, e, site_weights=None):
    """evaluate(t) of the central length of arrangement k of a quartet (nni_reference)."""
    import nni_reference as NR
    ends = NR.quartet_ends(orc, P, S, nodes, lens, k, e)
    return lambda t: tuple(NR.derivs_at(orc, ends, t, e, site_weights))


def pendant_evaluate(orc, ref, q, k, length=None, ends=None):
    """evaluate(l) of the pendant length of query q at the midpoint of edge number k of `ref`
    (place_reference.Restated).  Its formulas: the two ends carried half the edge's length each,
    their product the vector at the midpoint with the scalers added, the query's table row
    across P(l) -- given to orc.edge_derivs as one more edge (the midpoint at distance 0, the
    query at distance l), whose lnL is Restated.lnl_at's."""
    A_, sA, B_, sB = ref.ends[k] if ends is None else ends
    half = ref.pm(0.5 * (ref.lengths[k] if length is None else length))
    mid = np.einsum("cij,scj->sci", half, A_) * np.einsum("cij,scj->sci", half, B_)
    mid, sigma = mid[ref.map], (sA + sB)[ref.map]
    z = np.ascontiguousarray(np.broadcast_to(ref.z[q][:, None, :], mid.shape))
    zero = np.zeros(sigma.shape)
    e = ref.e
    return lambda l: tuple(orc.edge_derivs(mid, sigma, z, zero, e["evecs"], e["evals"],
                                           e["ivecs"], l, e["rates"], e["weights"], e["freqs"],
                                           ref.sw))
