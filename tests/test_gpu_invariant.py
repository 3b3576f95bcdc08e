"""Rate models with an invariable class (+I, +I+G) on every resident-partials kernel (DESIGN
4.21): the traversal, k_edge, k_quartet (NNI scores, per-pattern lnL, supports), k_ancestral,
k_counts, the placement kernels and k_regraft against the exact yardstick of
tests/invariant_reference.py -- the existing CPU restatements run on ``Exact``, the oracle with
P_0 = I, which tests/test_invariant.py pins to the product formula and to enumeration.

Tolerances: 1e-10 relative on lnL-type scalars (DESIGN 4.19's device-versus-restatement bound;
the oracle's own distance from the yardstick is below 1.5e-13, tests/test_invariant.py); 1e-10
absolute times the row's scale on posteriors and counts, since the invariable category leaves
entries that are 0 in truth.

Each case makes its device calls once (the `run` fixture); the tests below read what it kept."""
import numpy as np
import pytest

import ancestral_reference as AR
import counts_reference as CR
import invariant_reference as IR
import nni_reference as NR
import place_reference as PR
import spr_reference as SPR_R
import support_reference as SR
import walk_errors as W

from phylo_utils_amd import TreeModel, gradient, support
from phylo_utils_amd import place as PL
from phylo_utils_amd import spr as SPR

pytestmark = pytest.mark.gpu

L0, TOL, MAX_ITER = 0.1, 1e-8, 50
LENS = (0.11, 0.07, 0.2, 0.13, 0.09)
N_REP = 50


def _tm(prob, dense=None):
    tm = TreeModel(device=0, keep_partials=True, compact_tips=dense is None)
    if dense is None:
        tm.set_alignment_codes(prob["codes"], prob["table"], prob["names"], prob["weights"])
    else:
        tm.set_alignment_partials(dense, prob["names"], prob["weights"])
    tm.set_substitution_model(prob["model"])
    tm.set_rate_model(prob["rm"])
    tm.set_tree(prob["tree"])
    tm.initialise()
    return tm


def _same(a, b):
    assert np.array_equal(a["lnl"], b["lnl"], equal_nan=True) and np.array_equal(a["site"], b["site"])
    for (p0, s0), (p1, s1) in zip(a["parts"], b["parts"]):
        assert np.array_equal(p0, p1) and np.array_equal(s0, s1)


def _edges_to_test(tr):
    """An inner edge and a tip edge of the post-order orientation: (child, parent)."""
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    root = set(int(v) for v in tr.root_edge)
    rows = [(int(c), int(p)) for p, a, b in tr.postorder_traversal for c in (a, b)
            if int(p) not in root]
    return (next(x for x in rows if x[0] in internal), next(x for x in rows if x[0] not in internal))


def _device_calls(tm, prob, tr, snaps):
    """Every call of the issue's list, once, with a snapshot of the context after each."""
    out = {}

    def keep(name, value):
        out[name] = value
        snaps.append((name, W.snapshot(tm)))

    keep("lnl", (tm.likelihood(), tm.sitewise_patterns().copy()))
    keep("edges", [(x, tm.edge_derivatives(*x), tm.edge_derivatives(x[0], x[1], 0.37))
                   for x in _edges_to_test(tr) + (tuple(int(v) for v in tr.root_edge),)])
    keep("nni", tm.nni_scores(tol=TOL, max_iter=MAX_ITER))
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    tips = sorted(tr.names.values())
    nodes = (inner[0], tips[0], inner[1], tips[-1])
    keep("site3", (nodes, tm.quartet_site_lnl(nodes, LENS, (0.02, 0.3, 1.5))))
    keep("support", tm.branch_support(n_replicates=N_REP, seed=7, full=True))
    keep("support2", tm.branch_support(n_replicates=N_REP, seed=7, full=True))
    keep("rates", tm.site_rates())
    keep("anc", tm.ancestral_states(full=True))
    keep("counts", tm.edge_counts())
    q = prob["queries"]
    pre = PL.prescore(tm, q, L0)
    keep("pre", pre)
    chosen = PL.select_candidates(pre["scores"], 2)
    cand = sorted(set((e, k) for k, es in enumerate(chosen) for e in es) |
                  set((0, k) for k in range(len(chosen))))
    keep("fine", PL.refine(tm, q, cand, len(pre["edges"]), L0, TOL, MAX_ITER))
    keep("regraft", [((a, b, s), SPR.regraft_edge(tm, a, b, s, 0.23, 0.11))
                     for a, b, s in ((inner[0], inner[1], inner[2]), (inner[-1], tips[0], inner[0]),
                                     (tips[1], inner[1], tips[2]))])
    keep("spr", SPR.spr_scores(tm, radius=2))
    return out


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def run(request, oracle_mod):
    prob = IR.problem(request.param)
    tr, e, tips = IR.setting(prob)
    x = IR.Exact(oracle_mod)
    tm = _tm(prob)
    tm.likelihood()
    snaps = [("start", W.snapshot(tm))]
    got = _device_calls(tm, prob, tr, snaps)
    return dict(case=request.param, prob=prob, tr=tr, e=e, tips=tips, x=x, tm=tm, got=got,
                snaps=snaps, st=IR.state(x, tips, tr, e, prob["weights"]),
                const=IR.invariant_site_likelihood(tips, tr, e["freqs"]) > 0,
                w=np.asarray(prob["weights"], dtype=np.float64))


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_context_is_bitwise_unchanged_after_every_call(run):
    for name, snap in run["snaps"][1:]:
        _same(run["snaps"][0][1], snap)


def test_traversal(run):
    """likelihood() and sitewise_patterns().  Measured worst (lnL; per pattern, relative):
    binary-8x70-IG3 0 and 9.6e-16, dna-8x65-I 3.2e-16 and 7.1e-15, dna-8x65-IG3 3.7e-16 and
    3.4e-15, dna-coded-14x700-I 8.9e-16 and 3.7e-14, dna-coded-14x700-IG3 9.1e-16 and 2.2e-14,
    protein-8x97-IG3 3.1e-15 and 1.4e-13, dna-caterpillar-150x130-IG3 6.9e-16 and 1.4e-13."""
    lnl, site = run["got"]["lnl"]
    st = run["st"]
    worst = (np.abs(site - st["site_lnl"]) / np.abs(st["site_lnl"])).max()
    print("%s: traversal lnL %.2e, per pattern %.2e" % (run["case"], _rel(lnl, st["lnl"]), worst))
    assert _rel(lnl, st["lnl"]) <= 1e-10 and worst <= 1e-10


def test_edge_derivatives(run):
    """pu_edge_lnl / derivatives on an inner, a tip and the root edge, at the edge's length and at
    0.37, against the analytic form on the yardstick's partials (category 0 adds nothing to
    either derivative); relative to max(1, |value|) as tests/test_gpu_nni.py does for
    derivatives.  Measured worst: 7.4e-13 (dna-coded-14x700-I); 4.8e-15 on binary-8x70-IG3, 2.8e-13 on
    the caterpillar."""
    st, e, tr = run["st"], run["e"], run["tr"]
    P, S = st["partials"], st["scale"]
    worst = 0.0
    for (a, b), at_own, at_t in run["got"]["edges"]:
        for t, got in ((tr.brlens[a, b] if (a, b) != tuple(tr.root_edge) else tr.root_length(),
                        at_own), (0.37, at_t)):
            want = IR.analytic_edge_derivs(run["x"], P, S, a, b, t, e, run["w"])
            err = [abs(g - v) / max(1.0, abs(v)) for g, v in zip(got, want)]
            worst = max(worst, max(err))
    print("%s: edge (lnL, d1, d2) worst error %.2e" % (run["case"], worst))
    assert worst <= 1e-10


def test_nni_scores_and_supports(run):
    """The three arrangements' (t*, lnL), the per-pattern lnL matrix of pu_quartet_site_lnl, and
    the supports of pu_branch_support (the RELL sums of pu_rell.hip bit-equal across two calls).
    Measured worst: t* 1.4e-14, lnL 3.5e-15, per-pattern lnL 1.6e-14, RELL sums 8.5e-15 (all
    protein-8x97-IG3), aBayes / LRT 2.9e-11 (dna-caterpillar-150x130-IG3)."""
    x, e, tr, tips, w = run["x"], run["e"], run["tr"], run["tips"], run["w"]
    quartets, scores = run["got"]["nni"]
    rq, rs, ref, _ = SR.branch_support(x, tips, tr, e, w, N_REP, seed=7, tol=TOL,
                                       max_iter=MAX_ITER)
    assert np.array_equal(rq, quartets)
    e_t = (np.abs(scores[:, :, 0] - rs[:, :, 0]) / (1.0 + rs[:, :, 0])).max()
    e_l = (np.abs(scores[:, :, 1] - rs[:, :, 1]) / np.abs(rs[:, :, 1])).max()
    nodes, (site, out9) = run["got"]["site3"]
    st = run["st"]
    want = SR.site_lnl(x, st["partials"], st["scale"], nodes, LENS, (0.02, 0.3, 1.5), e)
    e_s = (np.abs(site - want) / np.maximum(1.0, np.abs(want))).max()
    q1, s1, sup, rell = run["got"]["support"]
    q2, s2, sup2, rell2 = run["got"]["support2"]
    assert np.array_equal(q1, quartets) and np.array_equal(s1, scores)
    assert np.array_equal(rell, rell2) and np.array_equal(s1, s2)
    assert all(np.array_equal(sup[f], sup2[f]) for f in support.FIELDS)
    e_r = e_a = 0.0
    for i, r in enumerate(ref):
        wnt = np.vstack([r["l"][None, :], r["B"]])
        e_r = max(e_r, (np.abs(rell[i] - wnt) / np.maximum(1.0, np.abs(wnt))).max())
        e_a = max(e_a, abs(sup["abayes"][i] - r["abayes"]), abs(sup["lrt"][i] - r["lrt"]) /
                  max(1.0, r["lrt"]))
    print("%s: NNI t* %.2e, lnL %.2e, per-pattern lnL %.2e, RELL sums %.2e, aBayes/LRT %.2e" % (
        run["case"], e_t, e_l, e_s, e_r, e_a))
    assert e_t <= 1e-6          # t* is Newton's to tol = 1e-8 (1 + t) on both sides
    assert e_l <= 1e-10 and e_s <= 1e-10 and e_r <= 1e-9 and e_a <= 1e-8


def test_ancestral_states_and_site_rates(run):
    """Posteriors, MAP states at decided patterns, cat_post with column 0, mean_rate: absolute
    1e-10 (rows sum to 1; mean_rate against the largest rate).  cat_post[:, 0] is <= 1e-12 at
    variable patterns and the yardstick's at constant ones.  Measured worst:
    posteriors 8.2e-15, cat_post 7.5e-14, mean_rate 3.7e-14 (all protein-8x97-IG3), column 0 at
    constant patterns below 1e-15."""
    x, e, tr, tips, w = run["x"], run["e"], run["tr"], run["tips"], run["w"]
    ref = AR.sweep(x, tips, tr, e, site_weights=w)
    got, (cat, rate) = run["got"]["anc"], run["got"]["rates"]
    assert got["nodes"].tolist() == ref["nodes"].tolist()
    const = run["const"]
    errs = dict(posteriors=np.abs(got["posteriors"] - ref["posteriors"]).max(),
                map_prob=np.abs(got["map_prob"] - ref["posteriors"].max(axis=2)).max(),
                cat_post=np.abs(cat - ref["cat_post"]).max(),
                cat0_variable=np.abs(cat[~const, 0]).max(),
                cat0_constant=np.abs(cat[const, 0] - ref["cat_post"][const, 0]).max(),
                mean_rate=np.abs(rate - ref["mean_rate"]).max() / e["rates"].max(),
                node_lnl=np.abs(got["node_lnl"] / ref["lnl"] - 1).max())
    print("%s: %s" % (run["case"], {k: "%.2e" % v for k, v in errs.items()}))
    assert (ref["cat_post"][const, 0] > 1e-3).all() and (ref["cat_post"][~const, 0] == 0).all()
    run["cat0_variable"] = errs.pop("cat0_variable")
    for k, v in errs.items():
        assert v <= 1e-10, (k, v)
    ok = AR.decided(ref["posteriors"])
    assert np.array_equal(got["map_state"][ok], ref["posteriors"].argmax(axis=2)[ok])


def test_cat_post_0_at_variable_patterns(run):
    """cat_post[:, 0] <= 1e-12 absolute at variable patterns, where the truth is 0.  Measured:
    exactly 0 on all seven cases.  With P_0 = U U^-1 (identity plus rounding of either sign) the
    noise F_0 took a weight where it was positive and the column reached 1.65e-12 (protein-8x97-
    IG3) and 1.72e-12 (dna-caterpillar-150x130-IG3); the builders now write I itself for a rate-0
    category."""
    _, (cat, _) = run["got"]["anc"], run["got"]["rates"]
    worst = np.abs(cat[~run["const"], 0]).max()
    print("%s: cat_post[:, 0] at variable patterns, worst %.2e" % (run["case"], worst))
    assert worst <= 1e-12


def test_edge_counts_and_gradients(run):
    """M_c, c >= 1, of every edge against the yardstick, absolutely: 1e-10 of the edge's largest
    entry over all categories (M_0 is test_counts_of_the_invariable_category's); the
    invariant of counts_reference.invariant; rate_gradient and branch_gradient against the
    yardstick's M through the same host algebra and, for the lengths, against the central
    differences of P.  Measured worst: M_c (c >= 1) 1.3e-13, invariant 2.6e-15, dlnL/dr_c 1.2e-14,
    dlnL/dw_c 4.0e-15 (all protein-8x97-IG3), edge lnL 8.9e-16, branch gradient 1.5e-11."""
    x, e, tr, tips, prob = run["x"], run["e"], run["tr"], run["tips"], run["prob"]
    ref = CR.sweep(x, tips, tr, e, site_weights=prob["weights"])
    got = run["got"]["counts"]
    assert got["edges"].tolist() == ref["edges"].tolist()
    scale = np.abs(ref["counts"]).max(axis=(1, 2, 3))
    err = np.abs(got["counts"] - ref["counts"]).max(axis=(2, 3)) / scale[:, None]  # [edge][c]
    inv = CR.invariant(got, e, x)
    e_inv = np.abs(inv / run["w"].sum() - 1).max()
    e_lnl = np.abs(got["edge_lnl"] / ref["lnl"] - 1).max()
    tm = run["tm"]
    d_rate, d_weight = gradient.rate_gradient(tm, got)
    r_rate, r_weight = gradient.rate_gradient(tm, ref)
    bg = gradient.branch_gradient(tm, got)
    bg = np.array([bg[(int(a), int(b))] for a, b in ref["edges"]])
    want = CR.branch_gradient(x, prob, ref)
    run["M0"] = (err[:, 0].max(), abs(d_rate[0] - r_rate[0]) / np.abs(r_rate).max())
    errs = dict(M=err[:, 1:].max(), invariant=e_inv, edge_lnl=e_lnl,
                d_rate=np.abs(d_rate[1:] - r_rate[1:]).max() / np.abs(r_rate).max(),
                d_weight=np.abs(d_weight - r_weight).max() / np.abs(r_weight).max(),
                branch=np.abs(bg - want).max() / np.abs(want).max())
    print("%s: %s" % (run["case"], {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["invariant"] <= 1e-12
    assert errs["branch"] <= 1e-9          # tests/test_gpu_counts.py's bound
    for k in ("M", "edge_lnl", "d_rate", "d_weight"):
        assert errs[k] <= 1e-10, (k, errs[k])


def test_counts_of_the_invariable_category(run):
    """M_0 against the yardstick, absolutely (1e-10 of the edge's largest entry), and with it
    rate_gradient's dlnL/dr_0 over the largest rate derivative.  Measured worst: M_0 5.8e-16
    (dna-coded-14x700-IG3), dlnL/dr_0 4.6e-16.  With P_0 = U U^-1 the device's F_0 at a variable
    pattern was rounding noise of either sign, and where it was positive k_counts added pw w_0 /
    Z x A_0(i) B_0(j), whose off-diagonal entries are of order 1: errors of 0.86 (dna-8x65-IG3)
    to 24.6 (the caterpillar) times the edge's scale in M_0 and 0.21 to 1.18 in dlnL/dr_0, which
    patterns added depending on the sign of a rounding error.  The P builders of the traversal,
    of the re-orientation and of the kernels now write I itself for a rate-0 category (DESIGN
    4.21)."""
    test_edge_counts_and_gradients(run) if "M0" not in run else None
    m0, r0 = run["M0"]
    print("%s: M_0 %.2e of the edge's scale, dlnL/dr_0 %.2e" % (run["case"], m0, r0))
    assert m0 <= 1e-10 and r0 <= 1e-10


def test_placement(run):
    """The pre-score table of the copy, sister and all-gap queries and the Newton-optimised
    pendant lengths.  Measured worst: pre-score 6.9e-15, all-gap query against the tree's lnL 1.1e-14,
    refined lnL 6.6e-15 (all protein-8x97-IG3), short of the Brent optimum 5.0e-16."""
    ref = PR.Restated(run["x"], run["prob"])
    pre, fine = run["got"]["pre"], run["got"]["fine"]
    assert pre["edges"].tolist() == ref.edges.tolist()
    want = ref.prescore(L0)
    e_pre = (np.abs(pre["scores"] - want) / np.abs(want)).max()
    e_gap = np.abs(pre["scores"][:, 2] / run["st"]["lnl"] - 1).max()
    e_fine, e_opt = 0.0, -np.inf
    for ed, k, l, lnl in zip(fine["edge_num"], fine["query"], fine["pendant"], fine["lnl"]):
        e_fine = max(e_fine, _rel(lnl, ref.lnl_at(int(k), int(ed), float(l))))
        if k != 2:
            _, best = ref.optimum(int(k), int(ed), L0)
            e_opt = max(e_opt, (best - lnl) / abs(best))
    print("%s: pre-score %.2e, all-gap vs tree %.2e, refined lnL %.2e, short of Brent %.2e" % (
        run["case"], e_pre, e_gap, e_fine, e_opt))
    assert e_pre <= 1e-10 and e_gap <= 1e-10 and e_fine <= 1e-10
    assert e_opt <= 1e-8                   # tests/test_gpu_place.py's bound
    # the copy's best edge is its tip's, on the lower bound
    rows = [i for i in range(len(fine["lnl"])) if fine["query"][i] == 0]
    best = max(rows, key=lambda i: fine["lnl"][i])
    tip = run["tr"].names[run["prob"]["planted"][0]]
    assert int(pre["edges"][fine["edge_num"][best]][0]) == tip or \
        tip in (int(v) for v in pre["edges"][fine["edge_num"][best]])
    assert fine["pendant"][best] <= 1e-7


def test_regraft_and_spr_scores(run):
    """regraft_edge on post-order vectors and spr_scores(radius=2) (every move; on the
    caterpillar every 40th).  Measured worst: regraft_edge 1.9e-15, spr scores 6.4e-15 (protein-8x97-IG3; 2786
    moves on the caterpillar, 6.9e-16)."""
    ref = SPR_R.Restated(run["x"], run["prob"])
    st, w = run["st"], run["prob"]["weights"]
    P, S = st["partials"], st["scale"]
    e_one = 0.0
    for (a, b, s), got in run["got"]["regraft"]:
        want = SPR_R.score_from(ref.orc, ref.e, w, P[a], S[a], P[b], S[b], P[s], S[s], 0.23, 0.11)
        e_one = max(e_one, _rel(got, want))
    moves, scores = run["got"]["spr"]
    assert len(moves) and moves[:, 4].max() == 2
    step = 40 if "caterpillar" in run["case"] else 1
    e_spr = 0.0
    if step == 1:
        want = ref.all_moves(radius=2)
        assert sorted(want) == sorted(SPR_R.key(*m[:4]) for m in moves)
    for m, s in list(zip(moves, scores))[::step]:
        n, o, u, v = (int(z) for z in m[:4])
        val = SPR_R.score_from(ref.orc, ref.e, w, *ref.ends(n, o, u, v)) if step > 1 else \
            want[SPR_R.key(n, o, u, v)][1]
        e_spr = max(e_spr, _rel(s, val))
    print("%s: regraft_edge %.2e, %d spr scores %.2e" % (run["case"], e_one, len(moves), e_spr))
    assert e_one <= 1e-10 and e_spr <= 1e-10


# ---------------------------------------------------------------- impossible patterns
@pytest.fixture(scope="module")
def dense(oracle_mod):
    """dna-8x65-IG3 on dense tips with an all-zero row of one tip at a pattern of weight 2 and at
    one of weight 0; then the same with both weights 0."""
    prob = IR.problem("dna-8x65-IG3")
    w = prob["weights"].copy()
    const = (prob["table"][prob["codes"]].prod(axis=0).sum(axis=1) > 0)
    hit = int(np.flatnonzero(~const & (w > 0))[1])
    zero = int(np.flatnonzero(w == 0)[0])
    w[hit] = 2.0
    part = prob["table"][prob["codes"]].copy()
    part[3, hit] = part[3, zero] = 0.0
    bad = [hit, zero]
    out = dict(prob=prob, bad=bad, hit=hit, part=part)
    for name, weights in (("live", w), ("dead", np.where(np.arange(len(w)) == hit, 0.0, w))):
        p = dict(prob, weights=weights, queries=dict(prob["queries"], site_weight=weights))
        tm = _tm(p, dense=part)
        tm.likelihood()
        snap = W.snapshot(tm)
        tr, e, _ = IR.setting(p)
        tips = {tr.names[n]: part[i] for i, n in enumerate(p["names"])}
        got = {}
        got["lnl"] = (tm.likelihood(), tm.sitewise_patterns().copy())
        got["edge"] = tm.edge_derivatives(*(int(v) for v in tr.root_edge))
        got["nni"] = tm.nni_scores(tol=TOL, max_iter=MAX_ITER)
        got["rates"] = tm.site_rates()
        got["anc"] = tm.ancestral_states(full=True)
        try:
            got["counts"] = tm.edge_counts()
        except ValueError as err:
            got["counts"] = err
        got["pre"] = PL.prescore(tm, p["queries"], L0)
        inner = sorted(set(int(v) for v in tr.postorder_traversal[:, 0]))
        got["regraft"] = SPR.regraft_edge(tm, inner[0], inner[1], inner[2], 0.23, 0.11)
        got["spr"] = SPR.spr_scores(tm, radius=2)
        _same(snap, W.snapshot(tm))
        out[name] = dict(prob=p, tm=tm, tr=tr, e=e, tips=tips, got=got)
    return out


def test_impossible_pattern_of_nonzero_weight(dense):
    """Every lnL is -inf, from the first of the two patterns only (the second has weight 0); the
    per-pattern quotients are NaN at the two patterns and nowhere else (include/phylo_hip.h)."""
    got, bad = dense["live"]["got"], dense["bad"]
    ok = np.ones(65, dtype=bool)
    ok[bad] = False
    _, site = got["lnl"]
    assert np.isneginf(site[bad]).all() and np.isfinite(site[ok]).all()
    assert got["edge"][0] == -np.inf
    assert np.isneginf(got["nni"][1][:, :, 1]).all()
    assert np.isneginf(got["anc"]["node_lnl"]).all()
    assert isinstance(got["counts"], ValueError) and "not finite" in str(got["counts"])
    assert np.isneginf(got["pre"]["scores"]).all()
    assert got["regraft"] == -np.inf and np.isneginf(got["spr"][1]).all()
    cat, rate = got["rates"]
    post = got["anc"]["posteriors"]
    assert np.isnan(cat[bad]).all() and np.isnan(rate[bad]).all() and np.isnan(post[:, bad]).all()
    assert np.isnan(got["anc"]["map_prob"][:, bad]).all()
    assert np.isfinite(cat[ok]).all() and np.isfinite(rate[ok]).all()
    assert np.isfinite(post[:, ok]).all()


def test_impossible_patterns_of_zero_weight_leave_every_sum_finite(dense, oracle_mod):
    """With both patterns at weight 0 every lnL is finite and the yardstick's on the remaining
    patterns, M, the gradients and the scores are finite and the yardstick's, and the per-pattern
    outputs are NaN at the two patterns alone."""
    d, bad = dense["dead"], dense["bad"]
    got, tr, e, tips, p = d["got"], d["tr"], d["e"], d["tips"], d["prob"]
    x = IR.Exact(oracle_mod)
    w = np.asarray(p["weights"], dtype=np.float64)
    ok = np.ones(65, dtype=bool)
    ok[bad] = False
    # the yardstick on the 63 possible patterns: the impossible ones carry weight 0
    tips_ok = {n: v[ok] for n, v in tips.items()}
    st = IR.state(x, tips_ok, tr, e, w[ok])
    want = st["lnl"]
    lnl, site = got["lnl"]
    errs = dict(edge=_rel(got["edge"][0], want),
                node_lnl=np.abs(got["anc"]["node_lnl"] / want - 1).max(),
                gap_query=np.abs(got["pre"]["scores"][:, 2] / want - 1).max())
    assert np.isneginf(site[bad]).all()
    assert np.isfinite(got["edge"]).all()
    _, rq, rs = NR.sweep(x, tips_ok, tr, e, TOL, MAX_ITER, site_weights=w[ok])
    errs["nni"] = (np.abs(got["nni"][1][:, :, 1] - rs[:, :, 1]) / np.abs(rs[:, :, 1])).max()
    ref = CR.sweep(x, tips_ok, tr, e, site_weights=w[ok])
    cnt = got["counts"]
    assert not isinstance(cnt, Exception) and np.isfinite(cnt["counts"]).all()
    scale = np.abs(ref["counts"]).max(axis=(1, 2, 3))  # M_0: test_counts_of_the_invariable_..
    errs["M"] = (np.abs(cnt["counts"] - ref["counts"])[:, 1:].max(axis=(1, 2, 3)) / scale).max()
    tm = d["tm"]
    for g in gradient.rate_gradient(tm, cnt) + (np.array(list(gradient.branch_gradient(
            tm, cnt).values())),):
        assert np.isfinite(g).all()
    mg = gradient.model_gradient(tm, ["pinvar", "alpha", "freqs", "rates"], cnt)
    assert all(np.isfinite(v).all() for v in mg.values())
    assert np.isfinite(got["pre"]["scores"]).all() and np.isfinite(got["spr"][1]).all()
    assert np.isfinite(got["regraft"])
    sr = SPR_R.Restated(x, p)
    sr.tips = tips_ok
    sr.prob = dict(p, weights=w[ok])
    allm = sr.all_moves(radius=2)
    errs["spr"] = max(_rel(s, allm[SPR_R.key(*m[:4])][1]) for m, s in zip(*got["spr"]))
    cat, rate = got["rates"]
    post = got["anc"]["posteriors"]
    assert np.isnan(cat[bad]).all() and np.isnan(rate[bad]).all() and np.isnan(post[:, bad]).all()
    assert np.isfinite(cat[ok]).all() and np.isfinite(rate[ok]).all()
    assert np.isfinite(post[:, ok]).all()
    refa = AR.sweep(x, tips_ok, tr, e, site_weights=w[ok])
    errs["posteriors"] = np.abs(post[:, ok] - refa["posteriors"]).max()
    errs["cat_post"] = np.abs(cat[ok] - refa["cat_post"]).max()
    print("dense 8x65, impossible patterns of weight 0: %s" % {k: "%.2e" % v
                                                               for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= 1e-10, (k, v)


def test_traversal_lnl_at_impossible_patterns(dense, oracle_mod):
    """likelihood() is -inf with an impossible pattern of non-zero weight and, with weight 0 on
    both, finite and the yardstick's (measured -604.4756109709818, 1e-16 relative).  Both were
    NaN while the traversal's pattern-weighted sum formed pw x lnL_s unconditionally, 0 x -inf;
    it now adds exactly 0 for weight 0, as every resident kernel does."""
    live, dead = dense["live"]["got"]["lnl"][0], dense["dead"]["got"]["lnl"][0]
    d = dense["dead"]
    ok = np.ones(65, dtype=bool)
    ok[dense["bad"]] = False
    w = np.asarray(d["prob"]["weights"], dtype=np.float64)
    want = IR.state(IR.Exact(oracle_mod), {n: v[ok] for n, v in d["tips"].items()}, d["tr"],
                    d["e"], w[ok])["lnl"]
    print("dense 8x65: likelihood() %r with an impossible pattern of weight 2, %r with weight 0 "
          "(yardstick %.6f)" % (live, dead, want))
    assert live == -np.inf
    assert np.isfinite(dead) and _rel(dead, want) <= 1e-10


# ---------------------------------------------------------------- pinvar: gradient and fit
@pytest.mark.parametrize("case", ["dna-8x65-IG3", "protein-8x97-IG3"])
def test_model_gradient_pinvar_alpha_freqs(oracle_mod, case):
    """model_gradient(tm, ["pinvar", "alpha", "freqs"]) against the CPU restatement
    (counts_reference.gradient on the yardstick's M), at the 1e-8 of the largest derivative that
    tests/test_gpu_counts.py asks of "alpha".  Measured worst: protein-8x97-IG3 pinvar 8.6e-13, alpha 5.2e-13, freqs
    1.3e-10 of max |g| = 307."""
    prob = IR.problem(case)
    tr, e, tips = IR.setting(prob)
    x = IR.Exact(oracle_mod)
    ref = CR.sweep(x, tips, tr, e, site_weights=prob["weights"])
    tm = _tm(prob)
    names = ["pinvar", "alpha", "freqs"]
    got = gradient.model_gradient(tm, names)
    got = np.concatenate([np.atleast_1d(got[n]) for n in names])
    K = len(prob["model"].freqs)
    keys = ["pinvar", "alpha"] + [("freqs", k) for k in range(K - 1)]
    want = np.array([CR.gradient(x, prob, tr, ref, k) for k in keys])
    err = np.abs(got - want) / np.abs(want).max()
    print("%s: model gradient pinvar %.2e, alpha %.2e, freqs %.2e of max |g| = %.3g" % (
        case, err[0], err[1], err[2:].max(), np.abs(want).max()))
    assert err.max() <= 1e-8


def test_fit_of_pinvar_and_alpha():
    """optimise_model(("pinvar", "alpha")) from (0.05, 1.0) on data simulated at (0.2, 0.5): it
    ends no lower than the lnL at the generating values, both derivatives are below the fit's
    own stopping threshold -- tests/test_gpu_counts.py's bound sqrt(2 lambda_max lnl_tol) with
    lambda_max <= sites x taxa, in the optimiser's coordinates -- and `tm` holds the returned
    values.  tests/test_invariant.py shows on the oracle that the maximum is interior for this seed."""
    from phylo_utils_amd import modelfit
    from phylo_utils_amd.rate_models import InvariantGammaModel
    prob = IR.fit_problem()
    lnl_truth = _tm(prob).likelihood()
    tm = _tm(dict(prob, rm=InvariantGammaModel(0.05, 3, 1.0)))
    lnl_tol = 1e-6
    fit = tm.optimise_model(("pinvar", "alpha"), branch_lengths=False, lnl_tol=lnl_tol)
    g = modelfit.coordinate_gradient(tm, fit)
    p = fit["params"]
    print("fit: lnL %.6f (at the generating values %.6f), pinvar %.4f, alpha %.4f, %d "
          "iterations, coordinate gradient %s" % (fit["lnl"], lnl_truth, p["pinvar"], p["alpha"],
                                                  fit["n_iter"], g))
    assert fit["lnl"] >= lnl_truth
    assert np.abs(g).max() <= np.sqrt(2.0 * 700 * 8 * lnl_tol)
    assert 0.0 < p["pinvar"] < 1.0
    assert tm.rate_model.pinvar == p["pinvar"] and tm.rate_model.alpha == p["alpha"]
    assert isinstance(tm.rate_model, InvariantGammaModel) and tm.likelihood() == fit["lnl"]
