"""The device against exact arithmetic: every P builder, the traversal, the rescaling, the edge
derivatives and the resident kernels against the 50-digit fixtures tests/golden/hp_*.npz
(tests/golden/make_golden_hp.py), each allowed ``4 x E_orc + tol_project`` (tests/hp_check.py):
four times the stored error of the fp64 oracle on the same case and quantity plus the suite's
device-versus-oracle tolerance.  Reads the fixtures only: no mpmath, no oracle.

The bound holds value by value: per matrix, per pattern, per length of an edge.

Every test prints its worst error / bound ratio and the raw device and oracle errors (the device
column of DESIGN.md's accuracy table is copied from these lines)."""
import math

import numpy as np
import pytest

import hp_cases as H
import hp_check as CK
from conftest import load_golden

from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import spr as SPR
from phylo_utils_amd.likelihood import hip_likelihood_engine as E

pytestmark = pytest.mark.gpu

CASES = [(m, r) for m in H.MODELS for r in H.TREE_RATE_MODELS]
IDS = ["%s-%s" % c for c in CASES]


def _tm(newick, names, codes, table, weights, model, rm, keep=True, coded=True):
    tm = TreeModel(device=0, keep_partials=keep, compact_tips=coded)
    if coded:
        tm.set_alignment_codes(codes, table, names, weights)
    else:
        tm.set_alignment_partials(table[codes], names, weights)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.set_tree(newick)
    tm.initialise()
    return tm


def _t8(model, rmn, rooting, keep=True, coded=True):
    g = load_golden("hp_tree8_" + model)
    rm = H.rate_model_of(rmn)
    assert np.array_equal(rm.rates, g[rmn + "_rates"]) and np.array_equal(rm.weights,
                                                                         g[rmn + "_catw"])
    tm = _tm(H.text(g["newick_" + rooting]), H.T8_NAMES, g["codes"], g["table"], g["weights"],
             H.model_of(model), rm, keep, coded)
    return g, tm


# ---------------------------------------------------------------- P
@pytest.mark.parametrize("model", H.MODELS)
@pytest.mark.parametrize("rmn", H.P_RATE_MODELS)
def test_pmatrices(model, rmn):
    """k_pmatrix_lane / k_pmatrix_aa through pu_get_pmatrices on lengths 0, 1e-14 .. 1000."""
    g = load_golden("hp_pmat_" + model)
    table, state, _ = H.table_of(model)
    rm = H.rate_model_of(rmn)
    assert np.array_equal(rm.rates, g[rmn + "_rates"])
    tm = _tm(H.text(g["newick"]), H.P_NAMES, state[g["codes"]], table, np.ones(4),
             H.model_of(model), rm)
    tr = tm.traversal
    lens = np.vstack([tr.op_lengths(), [[0.0, tr.root_length()]]])
    assert np.array_equal(lens, g[rmn + "_len"])
    truth = g[rmn + "_P"]
    P = np.empty(truth.shape)
    N.check(N.lib().pu_get_pmatrices(tm._ctx, N.ptr(P)))
    assert not np.isnan(P).any()
    a, r = CK.check_p(P, truth, g[rmn + "_E_orc_abs"], g[rmn + "_E_orc_rel"])
    d_abs, d_rel = CK.p_errors(P, truth)
    print("P %s-%s: %s; %s; device abs %.3e rel %.3e, oracle abs %.3e rel %.3e, %d entries < 0"
          % (model, rmn, a, r, d_abs.max(), d_rel.max(), g[rmn + "_E_orc_abs"].max(),
             g[rmn + "_E_orc_rel"].max(), int((P < 0).sum())))
    assert a.ok and r.ok


# ---------------------------------------------------------------- traversal
def _check_tree(label, tm, g, key):
    site = tm.sitewise_patterns()
    lnl = tm.likelihood()
    assert not np.isnan(site).any() and not math.isnan(lnl)
    rs = CK.check_site(site, g[key + "_site"], g[key + "_E_orc_site"])
    rl = CK.check_total(lnl, float(g[key + "_lnl"]), g[key + "_E_orc_lnl"])
    print("%s %s; oracle error %.3e" % (label, rs, g[key + "_E_orc_site"].max()))
    print("%s %s; oracle error %.3e" % (label, rl, float(g[key + "_E_orc_lnl"])))
    assert rs.ok and rl.ok


@pytest.mark.parametrize("coded", [True, False], ids=["coded", "dense"])
@pytest.mark.parametrize("keep", [True, False], ids=["keep", "lnl_only"])
@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_traversal(model, rmn, keep, coded):
    """Site lnL and total lnL of the 8-taxon tree: 80 patterns (one tile and a partial one),
    weights with zeros, ambiguity and gap codes, lengths 1e-8 .. 5."""
    g, tm = _t8(model, rmn, "r5", keep, coded)
    _check_tree("traversal %s-%s keep=%s coded=%s:" % (model, rmn, keep, coded), tm, g, rmn)


@pytest.mark.parametrize("coded", [True, False], ids=["coded", "dense"])
@pytest.mark.parametrize("keep", [True, False], ids=["keep", "lnl_only"])
def test_rescaling(keep, coded):
    """The 200-taxon caterpillar under GTR + G4: the device's scalers against the unscaled
    truth."""
    g = load_golden("hp_deep")
    rm = H.rate_model_of("g05")
    assert np.array_equal(rm.rates, g["rates"])
    tm = _tm(H.text(g["newick"]), H.DEEP_NAMES, g["codes"], g["table"], g["weights"],
             H.model_of("gtr"), rm, keep, coded)
    # lnL-only contexts keep no partials to read: the same shapes rescale the same way there
    if keep:
        assert np.count_nonzero(tm.node_partials(tm.traversal.root_edge[1])[1]) > 0
    _check_tree("rescaling keep=%s coded=%s:" % (keep, coded), tm, g, "g05")


# ---------------------------------------------------------------- zero lengths
@pytest.mark.parametrize("keep", [True, False], ids=["keep", "lnl_only"])
@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_zero_lengths(model, rmn, keep):
    """t1 and t2 on pendant edges of exactly 0: no NaN; where the true likelihood is exactly 0
    the device gives -inf or at most log(4 E_orc_P(tau = 0)) -- P(0)'s rounding noise, which is
    all such a pattern's likelihood can be made of; every other pattern is held to the site
    bound."""
    g, tm = _t8(model, rmn, "z", keep)
    key = rmn + "_z"
    site = tm.sitewise_patterns()
    zero = g[key + "_zero"]
    assert zero.any() and not zero.all()
    assert not np.isnan(site).any()
    cap = math.log(CK.FACTOR * float(g["E_orc_P0"]))
    worst = site[zero].max()
    r = CK.check_site(site, g[key + "_site"], g[key + "_E_orc_site"], mask=~zero)
    print("zero lengths %s-%s keep=%s: %d patterns of likelihood 0, device at most %.3f (cap %.3f, "
          "%d of them -inf); %s; oracle error %.3e"
          % (model, rmn, keep, zero.sum(), worst, cap, np.isneginf(site[zero]).sum(), r,
             g[key + "_E_orc_site"][~zero].max()))
    assert (site[zero] <= cap).all()
    assert r.ok


# ---------------------------------------------------------------- edge derivatives
def _edge_results(label, got, g, rmn, rooting):
    truth, Eo = g["%s_edge_%s" % (rmn, rooting)], g["%s_E_orc_edge_%s" % (rmn, rooting)]
    got = np.asarray(got)
    assert not np.isnan(got).any()
    r = CK.check_deriv(got, truth, Eo)
    dev = CK.deriv_error(got, truth)
    print("%s root edge %s: %s; device lnL %.3e d1 %.3e d2 %.3e, oracle lnL %.3e d1 %.3e d2 %.3e"
          % ((label, rooting, r) + tuple(dev.max(axis=0)) + tuple(Eo.max(axis=0))))
    return r.ok


@pytest.mark.parametrize("inline", [None, "0"], ids=["inline_default", "device_p"])
@pytest.mark.parametrize("two_pass", [None, "0"], ids=["default", "ticket"])
@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_edge_derivatives(model, rmn, two_pass, inline, monkeypatch):
    """TreeModel.edge_derivatives on a 1e-8 pendant edge, the internal 0.1 edge and the length-5
    edge, each the root edge of its own rooting so that the post-order partials are the edge's
    directed partials, at t = 1e-8, 1e-3, 1 and the edge's own length, on both paths of the
    final sum.  By default small K x C (GTR at C <= 4) get P, P' and P'' from the host in the
    launch; PU_EDGE_INLINE_P=0 sends them to the device build of pu_edge_dev.h as well."""
    for key, val in (("PU_EDGE_TWO_PASS", two_pass), ("PU_EDGE_INLINE_P", inline)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)
    ok = True
    for rooting in H.EDGE_ROOTINGS:
        g, tm = _t8(model, rmn, rooting)
        a, b = tm.traversal.root_edge
        ts = g["%s_edge_%s_t" % (rmn, rooting)]
        assert tm.traversal.root_length() in ts
        got = [tm.edge_derivatives(a, b, float(t)) for t in ts]
        ok &= _edge_results("edge derivatives %s-%s two_pass=%s inline_p=%s"
                            % (model, rmn, two_pass, inline), got, g, rmn, rooting)
    assert ok


def _mix(out, catw, w, dropped_ok):
    """(lnL, d1, d2) from lnl_branch_derivs' [S][C][3] = (log f_c, f_c'/f_c, (f_c'' f_c - f_c'^2)
    / f_c^2): the category mixture per pattern, then the weighted sum over patterns.  The
    reference's per-category formula takes log f_c, which is NaN where the rounding noise of a
    near-zero rate's P makes f_c negative.  Such a category is left out of the mixture, but only
    where `dropped_ok` [S][C] says that it carries no more of the pattern's likelihood than the
    site bound allows."""
    nan = np.isnan(out[..., 0])
    assert not (nan & ~dropped_ok).any(), np.argwhere(nan & ~dropped_ok)[:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(nan, -np.inf, out[..., 0]) + np.log(catw)[None, :]
        m = L.max(axis=1)
        u = np.exp(L - m[:, None])
        r1 = np.where(u > 0, out[..., 1], 0.0)
        r2 = np.where(u > 0, out[..., 2], 0.0)
    F0 = u.sum(axis=1)
    d1 = (u * r1).sum(axis=1) / F0
    d2 = (u * (r2 + r1 * r1)).sum(axis=1) / F0 - d1 * d1
    nz = w != 0
    return (float(np.dot(w[nz], (m + np.log(F0))[nz])), float(np.dot(w[nz], d1[nz])),
            float(np.dot(w[nz], d2[nz]))), int(nan.sum())


def _negligible(P, pi, catw, pa, pb, sa, sb, E_site):
    """[S][C]: the categories whose share of the pattern's likelihood, |f_c| w_c over the sum of
    those, formed in fp64 on the host from the same partials and P, is at most the pattern's
    site bound FACTOR E_p + TOL_SITE: leaving one out moves the pattern's lnL by no more."""
    f = (np.einsum("cij,scj->sci", P, pa) * pb * pi).sum(axis=-1)
    sc = sa + sb
    F = np.abs(f) * catw * np.exp(sc - sc.max(axis=1, keepdims=True))
    return F / F.sum(axis=1, keepdims=True) <= (CK.FACTOR * E_site + CK.TOL_SITE)[:, None]


@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_lnl_branch_derivs_dropin(model, rmn):
    """The lnl_branch_derivs drop-in on the device's own end partials of the same three edges,
    with the host's eigen-form P, P' and P'' (Model.p_derivative), mixed over categories and
    summed over patterns on the host.  A NaN log f_c is accepted only in a category of negligible
    share (_negligible)."""
    ok = True
    for rooting in H.EDGE_ROOTINGS:
        g, tm = _t8(model, rmn, rooting)
        a, b = tm.traversal.root_edge
        pa, sa = tm.node_partials(a)
        pb, sb = tm.node_partials(b)
        m, rm = tm.substitution_model, tm.rate_model
        got, n_nan = [], 0
        for t in g["%s_edge_%s_t" % (rmn, rooting)]:
            probs = np.stack([m.p_derivative(float(t), rm.rates, k) for k in range(3)], axis=1)
            out = E.lnl_branch_derivs(np.ascontiguousarray(probs), m.freqs, pa, pb, sa, sb)
            v, n = _mix(out, rm.weights, g["weights"],
                        _negligible(probs[:, 0], m.freqs, rm.weights, pa, pb, sa, sb,
                                    g[rmn + "_E_orc_site"]))
            got.append(v)
            n_nan += n
        ok &= _edge_results("lnl_branch_derivs %s-%s (%d NaN log f_c left out)"
                            % (model, rmn, n_nan), got, g, rmn, rooting)
    assert ok


# ---------------------------------------------------------------- the resident kernels' P build
def _root_quartet(tm):
    tr = tm.traversal
    kids = {int(p): (int(x), int(y)) for p, x, y in tr.postorder_traversal}
    L, R = tr.root_edge
    nodes = kids[L] + kids[R]
    lens = [tr.brlens[L, nodes[0]], tr.brlens[L, nodes[1]], tr.brlens[R, nodes[2]],
            tr.brlens[R, nodes[3]], tr.root_length()]
    return nodes, lens


@pytest.mark.parametrize("rooting", ["r01", "r1e8"])
@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_quartet_site_lnl(model, rmn, rooting):
    """pu_quartet_site_lnl around the internal 0.1 edge and the internal 1e-8 edge (each the root
    edge of its rooting): the standing arrangement's per-pattern lnL is the tree's."""
    g, tm = _t8(model, rmn, rooting)
    nodes, lens = _root_quartet(tm)
    assert lens[4] == {"r01": 0.1, "r1e8": 1e-8}[rooting]
    site, _ = tm.quartet_site_lnl(nodes, lens)
    assert not np.isnan(site[0]).any()
    r = CK.check_site(site[0], g[rmn + "_site"], g[rmn + "_E_orc_site"])
    print("quartet %s-%s %s: %s; oracle error %.3e" % (model, rmn, rooting, r,
                                                        g[rmn + "_E_orc_site"].max()))
    assert r.ok


@pytest.mark.parametrize("model,rmn", CASES, ids=IDS)
def test_regraft_back_in_place(model, rmn):
    """pu_regraft_edge of the subtree on the near side of the length-5 root edge onto the edge
    its far end's two children make when that end is dissolved -- two halves of 1e-4, the lengths
    they had -- on its old pendant length: the tree itself, so the score is the tree's lnL."""
    g, tm = _t8(model, rmn, "r5")
    tr = tm.traversal
    kids = {int(p): (int(x), int(y)) for p, x, y in tr.postorder_traversal}
    n, o = tr.root_edge
    x, y = kids[o]
    assert tr.brlens[o, x] == tr.brlens[o, y] == 1e-4
    got = SPR.regraft_edge(tm, x, y, n, tr.brlens[o, x] + tr.brlens[o, y], tr.root_length())
    r = CK.check_total(got, float(g[rmn + "_lnl"]), g[rmn + "_E_orc_lnl"], "regraft lnL")
    print("regraft %s-%s: %s; oracle error %.3e" % (model, rmn, r, float(g[rmn + "_E_orc_lnl"])))
    assert r.ok
