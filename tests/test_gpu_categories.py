"""Wide category counts on the device: pu_ctx_create accepts C up to 64, and the kernels change
shape with C (4 % C == 0: fused categories; otherwise per category + k_site_lse; K = 20: a
workgroup per (tile, category)).  Coded tips, kept partials and lnL-only, K = 4, 2 and 20, 12
taxa x 130 sites (3 tiles, the last one partial), GammaRateModel(C, 0.4), against
oracle.tree_lnl(return_all=True) at the tolerances of tests/test_gpu_parity.py: sitewise lnL
rtol 1e-12, total 1e-12 relative, partials 1e-12 of each vector's largest entry, scalers rtol
1e-13 / atol 1e-10, P rtol 1e-12 / atol 1e-15.

What the library refuses is pinned too: C = 65, and the edge kernels above the category count
whose matrices fit the 160 KiB of LDS one workgroup may have (pu_edge.hip, EdgeLds)."""
import numpy as np
import pytest

import twostate as T
from test_gpu_parity import assert_partials_close
from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem

pytestmark = pytest.mark.gpu

N_TAXA, N_SITES = 12, 130


def problem(K, C):
    """(model, rate model, tree, names, codes, table) -- no gaps: every sitewise lnL is far
    from zero, so the relative bound applies to every site."""
    rm = GammaRateModel(C, 0.4)
    if K == 2:
        model = T.TwoState(0.3)
        tree, names, codes, table, _ = T.binary_problem(N_TAXA, N_SITES, 0.3, rm.rates, seed=C,
                                                        ambiguous=False)
        return model, rm, tree, names, codes, table
    model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if K == 4 else SM.LG()
    tree, names, states = make_problem(N_TAXA, N_SITES, model, rm.rates, seed=C)
    return model, rm, tree, names, states.astype(np.uint8), np.eye(K)


def build(K, C, keep=True):
    model, rm, tree, names, codes, table = problem(K, C)
    tm = TreeModel(keep_partials=keep)
    tm.set_alignment_codes(codes, table, names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    return tm


def oracle_state(orc, tm, device_p=False):
    tr, m, rm = tm.traversal, tm.substitution_model, tm.rate_model
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    ev, el, iv = m.engine_eigen()
    ref = orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                       tr.root_length(), ev, el, iv, m.freqs, rm.rates, rm.weights,
                       n_nodes=tr.n_nodes, return_all=True)
    if not device_p:
        return ref
    K, C = len(m.freqs), rm.ncat
    P = np.empty((len(tr.postorder_traversal) + 1, 2, C, K, K))
    N.check(N.lib().pu_get_pmatrices(tm._ctx, N.ptr(P)))
    np.testing.assert_allclose(P[:-1], ref["P"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(P[-1], ref["Proot"], rtol=1e-12, atol=1e-15)
    return orc.tree_lnl_p(tips, tr.postorder_traversal, P[:-1], P[-1], tr.root_edge, m.freqs,
                          rm.weights, n_nodes=tr.n_nodes, return_all=True)


def vec_err(got, ref):
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(got - ref) / np.where(scale > 0, scale, 1)).max())


WIDE = [(4, C) for C in (7, 12, 17, 32, 33, 64)] + [(2, C) for C in (7, 32, 64)] + \
       [(20, C) for C in (7, 16, 64)]


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("K,C", WIDE)
def test_wide_category_counts_vs_oracle(oracle_mod, K, C, keep):
    """Sitewise and total lnL against oracle.tree_lnl (rtol 1e-12).  The root and, with kept
    partials, every partial and scaler against the oracle's traversal on the device's own P
    (1e-12 of a vector's largest entry; scalers rtol 1e-13 / atol 1e-10), that P being read back
    and held to the oracle's at rtol 1e-12 / atol 1e-15 -- the decomposition of
    test_protein_partials_deviation_is_the_pmatrix.

    Against the oracle on its own P the partials do NOT meet 1e-12 and the scalers do not meet
    1e-10 at wide C; the figures are printed, not asserted.  Measured on an MI355X, partials /
    scalers: K = 4: 1.3e-12 (C = 7), 6.4e-12 (12), 6.2e-12 (17), 2.4e-11 (32), 6.4e-11 (33),
    3.9e-10 (64), scalers 0; K = 2: 1.0e-15 (7), 1.0e-11 (32), 7.4e-11 (64); K = 20: 2.7e-11
    (7), 5.3e-11 (16), 3.1e-9 / 2.7e-9 (64).  Cause: the slowest of C Gamma(0.4) categories
    has rate 1.6e-5 at C = 64, so a short branch's off-diagonal P entry is ~1e-7; the eigen form
    gives an entry only absolute accuracy (a few eps), the device (fused multiply-add) and the
    oracle (multiply, then add) round it differently, and a vector that needs a change on that
    branch is proportional to that one entry."""
    tm = build(K, C, keep)
    tr = tm.traversal
    ref = oracle_state(oracle_mod, tm)
    site = tm.sitewise_patterns()
    assert np.all(np.isfinite(site))
    np.testing.assert_allclose(site, ref["site_lnl"], rtol=1e-12)
    lnl = tm.likelihood()
    assert abs(lnl - ref["lnl"]) <= 1e-12 * abs(ref["lnl"]), (lnl, ref["lnl"])
    pref = oracle_state(oracle_mod, tm, device_p=True)
    rp, rs = tm.compute_partials_at_edge(*tr.root_edge)
    assert rp.shape == (N_SITES, C, K)
    assert_partials_close(rp, pref["root_partials"])
    np.testing.assert_allclose(rs, pref["root_scale"], rtol=1e-13, atol=1e-10)
    e_p = e_o = e_s = e_so = 0.0
    if keep:
        parts, scale = tm.partials, tm.scale
        assert_partials_close(parts, pref["partials"])
        np.testing.assert_allclose(scale, pref["scale"], rtol=1e-13, atol=1e-10)
        e_p, e_o = vec_err(parts, pref["partials"]), vec_err(parts, ref["partials"])
        e_s = float(np.abs(scale - pref["scale"]).max())
        e_so = float(np.abs(scale - ref["scale"]).max())
    print("K=%d C=%d keep=%s max errors: sitewise %.2e, lnL %.2e; on the device's P: root %.2e, "
          "partials %.2e, scalers %.2e; on the oracle's own P (not asserted): root %.2e, "
          "partials %.2e, scalers %.2e" % (
              K, C, keep, float(np.abs(site / ref["site_lnl"] - 1).max()),
              abs(lnl - ref["lnl"]) / abs(ref["lnl"]), vec_err(rp, pref["root_partials"]), e_p,
              e_s, vec_err(rp, ref["root_partials"]), e_o, e_so))


# the most categories whose matrices fit one workgroup's 160 KiB of LDS (EdgeLds, pu_edge.hip):
# derivatives hold 4 matrices and 4 x 64 values per category
EDGE_DERIV_MAX_C = {2: 64, 4: 60, 20: 10}


@pytest.mark.parametrize("K,C", [(2, 64), (4, 17), (4, 60), (4, 64), (20, 10), (20, 17),
                                 (20, 64)])
def test_wide_edge_derivatives_or_clean_refusal(oracle_mod, K, C):
    """edge_derivatives on the root edge against oracle.edge_derivs (1e-10 of max(1, |v|)) up
    to the category count the edge kernel's LDS holds -- the limit itself included -- and a clean
    PhyloHipError (PU_E_ARG, nothing launched) above it, after which the context still gives the
    traversal's numbers."""
    tm = build(K, C)
    tr, m, rm = tm.traversal, tm.substitution_model, tm.rate_model
    a, b = tr.root_edge
    lnl0, site0 = tm.likelihood(), tm.sitewise_patterns().copy()
    if C > EDGE_DERIV_MAX_C[K]:
        with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
            tm.edge_derivatives(a, b)
        with pytest.raises(N.PhyloHipError):
            tm.optimise_edge(a, b)
        assert tm.likelihood() == lnl0
        np.testing.assert_array_equal(tm.sitewise_patterns(), site0)
        # a sweep re-orients partials (pu_update_partials fits) before its first derivative
        # call is refused: the lengths are untouched, and one traversal restores every number
        lens0 = dict(tr.brlens)
        with pytest.raises(N.PhyloHipError):
            tm.optimise_branch_lengths()
        assert dict(tr.brlens) == lens0
        tm.compute_partials()
        assert tm.likelihood() == lnl0
        np.testing.assert_array_equal(tm.sitewise_patterns(), site0)
        return
    ref = oracle_state(oracle_mod, tm, device_p=(K == 20))
    ev, el, iv = m.engine_eigen()
    P, S = ref["partials"], ref["scale"]
    worst = 0.0
    for t in (None, 0.05, 0.7):
        got = tm.edge_derivatives(a, b, t)
        tt = tr.root_length() if t is None else t
        want = oracle_mod.edge_derivs(P[a], S[a], P[b], S[b], ev, el, iv, tt, rm.rates,
                                      rm.weights, m.freqs)
        for k in range(3):
            worst = max(worst, abs(got[k] - want[k]) / max(1.0, abs(want[k])))
            assert abs(got[k] - want[k]) <= 1e-10 * max(1.0, abs(want[k])), (t, got, want)
    print("K=%d C=%d edge derivatives: max error relative to max(1, |v|) %.2e" % (K, C, worst))
    assert abs(tm.edge_derivatives(a, b)[0] - lnl0) <= 1e-12 * abs(lnl0)


def test_sixty_five_categories_are_refused():
    """pu_ctx_create takes 1 <= C <= 64: C = 65 is PU_E_ARG, through the Python wrapper a
    PhyloHipError before anything is allocated."""
    model, _, tree, names, codes, table = problem(4, 64)
    tm = TreeModel()
    tm.set_alignment_codes(codes, table, names)
    tm.set_substitution_model(model)
    tm.set_rate_model(GammaRateModel(65, 0.4))
    tm.set_tree(tree)
    with pytest.raises(N.PhyloHipError, match=r"pu_ctx_create failed \(%d\)" % N.PU_E_ARG):
        tm.initialise()
    assert tm._ctx is None
    tm.set_rate_model(GammaRateModel(64, 0.4))  # the same model object goes on at the limit
    tm.initialise()
    assert np.isfinite(tm.likelihood())
