"""The two-state (K = 2) kernel family on the device against the CPU oracle and the closed form
(tests/twostate.py; both proved against each other in tests/test_twostate_reference.py):
k_pmatrix_lane<2>, every k_prune<2, ...> build and plan, k_site_lse, k_untile, k_edge<2>,
k_edge_newton<2, 1|2>, the minimisers, the batch kernels, k_ascbias and the facade.

Tolerances are the ones tests/test_gpu_parity.py and tests/test_gpu_edges.py hold K = 4 to:
partials 1e-12 of each vector's largest entry, scalers rtol 1e-13 / atol 1e-10, P rtol 1e-12 /
atol 1e-15, sitewise lnL rtol 1e-12, total lnL 1e-12 relative, derivatives 1e-10 of
max(1, |v|), optimised lengths 1e-6 relative, lnL after a sweep 1e-9 relative.

A column of gaps only has lnL = log(1) = 0 exactly, where a relative bound says nothing: there
the absolute value is bounded instead (gap_atol below).

Shapes: a tile is 64 sites and a workgroup is 4 waves, one (tile, category) pair each."""
import ctypes

import numpy as np
import pytest

import twostate as T
from test_gpu_batch import GRID_ENVS
from test_gpu_parity import (KEEP_OCC_ENVS, PLAN_ENVS, RSLOT_ENVS, _height_order,
                             assert_partials_close)
from phylo_utils_amd import TreeModel
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd.batch import TreeBatch
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import random_tree

pytestmark = pytest.mark.gpu

PI0 = 0.3
EPS = np.finfo(float).eps
TV_GENERIC, TV_CHAIN = 16, 64  # pu_internal.h (N.ctx_plan's variant bits)


def gap_atol(n_taxa):
    """|lnL| of an all-gap column: every vector is a product of row sums of P, each within a
    few roundings of 1 (an entry of P is a sum of two O(1) terms: <= 4 eps, a row 8 eps), over
    at most 2 n_taxa edges."""
    return 8 * EPS * 2 * n_taxa


def rates_of(C):
    return GammaRateModel(C, 0.5) if C > 1 else UniformRateModel()


def make_tm(tree, names, codes, table, rm, coded=True, keep=True, pi0=PI0, **kw):
    tm = TreeModel(keep_partials=keep, compact_tips=coded, **kw)
    if coded:
        tm.set_alignment_codes(codes, table, names)
    else:
        tm.set_alignment_partials(table[codes], names)
    tm.set_substitution_model(T.TwoState(pi0))
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    return tm


def oracle_state(orc, tm, return_all=True):
    tr, m, rm = tm.traversal, tm.substitution_model, tm.rate_model
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    ev, el, iv = m.engine_eigen()
    return orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                        tr.root_length(), ev, el, iv, m.freqs, rm.rates, rm.weights,
                        n_nodes=tr.n_nodes, return_all=return_all)


def oracle_on_device_p(orc, tm, ref):
    """The oracle's traversal on the device's own P, which is first held to the oracle's
    (rtol 1e-12, atol 1e-15)."""
    tr, m, rm = tm.traversal, tm.substitution_model, tm.rate_model
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    P = np.empty((len(tr.postorder_traversal) + 1, 2, rm.ncat, 2, 2))
    N.check(N.lib().pu_get_pmatrices(tm._ctx, N.ptr(P)))
    np.testing.assert_allclose(P[:-1], ref["P"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(P[-1], ref["Proot"], rtol=1e-12, atol=1e-15)
    return orc.tree_lnl_p(tips, tr.postorder_traversal, P[:-1], P[-1], tr.root_edge, m.freqs,
                          rm.weights, n_nodes=tr.n_nodes, return_all=True)


def vec_err(got, ref):
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(got - ref) / np.where(scale > 0, scale, 1)).max()) if ref.size else 0.0


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max()) if ref.size else 0.0


def check_site(got, ref, codes, n_taxa):
    """sitewise lnL rtol 1e-12; all-gap columns |lnL| <= gap_atol.  Returns the max errors."""
    gap = T.all_gap_columns(codes)
    np.testing.assert_allclose(got[~gap], ref[~gap], rtol=1e-12)
    assert np.all(np.abs(got[gap]) <= gap_atol(n_taxa)), np.abs(got[gap]).max()
    return rel_err(got[~gap], ref[~gap]), float(np.abs(got[gap]).max()) if gap.any() else 0.0


def close(x, y, rtol):
    assert abs(x - y) <= rtol * max(1.0, abs(y)), (x, y, abs(x - y))


# ---------------------------------------------------------------- P matrices
@pytest.mark.parametrize("C", [1, 4])
def test_pmatrices_vs_closed_form(C):
    """k_pmatrix_lane<2> (pu_get_pmatrices) against the closed form on branch lengths 0, 1e-8,
    0.1 and 10: rtol 1e-12, atol 1e-15."""
    rm = rates_of(C)
    nwk = "((a:0,b:1e-8):0.1,(c:10,d:0.1):1e-8,(e:10,f:0):0.1);"
    rng = np.random.default_rng(C)
    names = list("abcdef")
    codes = rng.integers(0, len(T.BIN_TABLE), (6, 10)).astype(np.uint8)
    tm = make_tm(nwk, names, codes, T.BIN_TABLE, rm)
    tr = tm.traversal
    bl = tr.op_lengths()
    assert set(np.unique(bl)) | {tr.root_length()} == {0.0, 1e-8, 0.1, 10.0}
    P = np.empty((len(bl) + 1, 2, C, 2, 2))
    N.check(N.lib().pu_get_pmatrices(tm._ctx, N.ptr(P)))
    ref = np.stack([np.stack([T.closed_p(PI0, l1, rm.rates), T.closed_p(PI0, l2, rm.rates)])
                    for l1, l2 in bl] +
                   [np.stack([T.closed_p(PI0, 0.0, rm.rates),
                              T.closed_p(PI0, tr.root_length(), rm.rates)])])
    print("C=%d: max |P - closed form| %.2e" % (C, np.abs(P - ref).max()))
    np.testing.assert_allclose(P, ref, rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------- whole traversal
SITES = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("coded", [True, False])
@pytest.mark.parametrize("n_taxa", [2, 3, 17])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
def test_all_partials_and_root_vs_oracle(oracle_mod, C, n_taxa, coded, keep):
    """Every partial, scaler, the root and the sitewise lnL against oracle.tree_lnl, coded and
    dense tips, kept partials and lnL-only (coded: the tip products, TV_PTIP), with gaps.
    C in {1, 2, 4}: the fused-category path; C in {3, 5}: per category + k_site_lse.  S: one
    site, a tile less one, a tile, a tile and one, 257 (5 tiles: at C = 1 a second workgroup
    with 3 dead waves; at C = 4, 65 sites are 2 tiles = 2 workgroups)."""
    rm = rates_of(C)
    worst = dict(partials=0.0, scale=0.0, root=0.0, site=0.0, gap=0.0, lnl=0.0)
    for S in SITES:
        tree, names, codes, table, _ = T.binary_problem(n_taxa, S, PI0, rm.rates,
                                                        seed=100 * C + n_taxa)
        tm = make_tm(tree, names, codes, table, rm, coded=coded, keep=keep)
        tr = tm.traversal
        ref = oracle_state(oracle_mod, tm)
        e_site, e_gap = check_site(tm.sitewise_patterns(), ref["site_lnl"], codes, n_taxa)
        worst["site"], worst["gap"] = max(worst["site"], e_site), max(worst["gap"], e_gap)
        lnl = tm.likelihood()
        assert abs(lnl - ref["lnl"]) <= 1e-12 * abs(ref["lnl"]), (S, lnl, ref["lnl"])
        worst["lnl"] = max(worst["lnl"], abs(lnl - ref["lnl"]) / max(abs(ref["lnl"]), 1e-300))
        rp, rs = tm.compute_partials_at_edge(*tr.root_edge)
        assert rp.shape == (S, C, 2) and rs.shape == (S, C)
        assert_partials_close(rp, ref["root_partials"])
        np.testing.assert_allclose(rs, ref["root_scale"], rtol=1e-13, atol=1e-10)
        worst["root"] = max(worst["root"], vec_err(rp, ref["root_partials"]))
        if keep:
            parts, scale = tm.partials, tm.scale
            assert parts.shape == (tr.n_nodes, S, C, 2)
            assert_partials_close(parts, ref["partials"])
            np.testing.assert_allclose(scale, ref["scale"], rtol=1e-13, atol=1e-10)
            worst["partials"] = max(worst["partials"], vec_err(parts, ref["partials"]))
            worst["scale"] = max(worst["scale"], float(np.abs(scale - ref["scale"]).max()))
    print("C=%d taxa=%d coded=%s keep=%s max errors: %s" % (
        C, n_taxa, coded, keep, ", ".join("%s %.2e" % kv for kv in worst.items())))


# ---------------------------------------------------------------- rescaling
RESCALE = dict(n_taxa=400, n_sites=130, seed=11, lo=0.01, hi=1.0)


def rescale_problem():
    rm = rates_of(4)
    p = RESCALE
    return (rm,) + T.binary_problem(p["n_taxa"], p["n_sites"], PI0, rm.rates, seed=p["seed"],
                                    lo=p["lo"], hi=p["hi"])


@pytest.mark.parametrize("keep", [True, False])
def test_rescaling_and_scalers_across_runs(oracle_mod, keep):
    """A tree deep enough to rescale on two states: 400 taxa, branches U(0.01, 1), 130 sites
    (3 tiles, the last of 2 sites), C = 4, with gaps.  Chosen with the oracle on the CPU
    (0.04 s per evaluation): non-zero scalers are 0.31 % of all (node, site, category) entries
    at the simulated lengths, 0.84 % at 0.01 x and 0.39 % at 0.3 x them.  Evaluated four times on
    one context with changed lengths: scaler tiles that were non-zero and become zero must be
    rewritten and vice versa (TV_SKIP_ZERO_SCALE and its sflag bookkeeping, keep=True)."""
    rm, tree, names, codes, table, _ = rescale_problem()
    tm = make_tm(tree, names, codes, table, rm, keep=keep)
    tr = tm.traversal
    orig = dict(tr.brlens)
    seen = []
    for factor in (1.0, 0.01, 1.0, 0.3):
        for k in orig:
            tr.brlens[k] = orig[k] * factor
        tm.update_branch_lengths()
        ref = oracle_state(oracle_mod, tm)
        nz = ref["scale"] != 0
        assert nz.any()
        seen.append(nz)
        e_site, e_gap = check_site(tm.sitewise_patterns(), ref["site_lnl"], codes,
                                   RESCALE["n_taxa"])
        assert abs(tm.likelihood() - ref["lnl"]) <= 1e-12 * abs(ref["lnl"])
        # partials: 1e-12 against the oracle's traversal on the device's own P (itself held to
        # the oracle's P at rtol 1e-12 / atol 1e-15).  Against the oracle on its own P they
        # meet 1e-12 at the simulated lengths (2.8e-14) and at 0.3 x (1.1e-13) but NOT at
        # 0.01 x (2.3e-11; printed, not asserted): there the shortest branch in the slowest
        # category has P_01 ~ 1e-6, which the eigen form gives only absolute accuracy, and
        # the two P builders round it differently
        dev = oracle_on_device_p(oracle_mod, tm, ref)
        rp, rs = tm.compute_partials_at_edge(*tr.root_edge)
        assert_partials_close(rp, dev["root_partials"])
        np.testing.assert_allclose(rs, ref["root_scale"], rtol=1e-13, atol=1e-10)
        e_p = e_s = 0.0
        if keep:
            parts, scale = tm.partials, tm.scale
            assert_partials_close(parts, dev["partials"])
            np.testing.assert_allclose(scale, ref["scale"], rtol=1e-13, atol=1e-10)
            e_p, e_s = vec_err(parts, ref["partials"]), float(np.abs(scale - ref["scale"]).max())
            print("   partials vs oracle on device P %.2e, on its own P %.2e (not asserted)" % (
                vec_err(parts, dev["partials"]), e_p))
        print("keep=%s x%.2f: %.3f %% scalers non-zero; max errors: site %.2e, gap column %.2e, "
              "partials %.2e, scalers %.2e" % (keep, factor, 100.0 * nz.mean(), e_site, e_gap,
                                               e_p, e_s))
    # the runs differ in which entries are scaled, both ways
    assert (seen[0] & ~seen[1]).any() or (seen[1] & ~seen[0]).any()
    assert (seen[1] & ~seen[2]).any()


# ---------------------------------------------------------------- builds and plans
_BASE = {}


def _plan_problem(case):
    if case == "taxa17":
        rm = rates_of(4)
        return (rm,) + T.binary_problem(17, 257, PI0, rm.rates, seed=17)
    return rescale_problem()


def _plan_base(case, keep):
    """The default run of a case (built before any env of the test is set)."""
    if (case, keep) not in _BASE:
        rm, tree, names, codes, table, _ = _plan_problem(case)
        tm = make_tm(tree, names, codes, table, rm, keep=keep)
        _BASE[case, keep] = (tm.likelihood(), tm.sitewise_patterns().copy(),
                             tm.partials if keep else None, tm.scale if keep else None)
    return _BASE[case, keep]


ALL_PLAN_ENVS = PLAN_ENVS + RSLOT_ENVS + KEEP_OCC_ENVS + [{"PU_NO_PTIP": "1"}]
_PLAN_VARS = sorted({k for e in ALL_PLAN_ENVS for k in e})


@pytest.mark.parametrize("env", ALL_PLAN_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in
                                                                       sorted(e.items())))
@pytest.mark.parametrize("case", ["taxa17", "rescale"])
def test_builds_and_plans_bitwise_equal(monkeypatch, case, env):
    """Every k_prune<2, ...> build and plan the env lists of the K = 4 / K = 20 tests select
    (test_kernel_builds_and_plans_bitwise_equal, test_register_stash_slots_bitwise,
    test_keep_occupancy_rule_bitwise) and PU_NO_PTIP=1 (lnL-only coded K = 2 without tip
    products: launch_prune_w's re-routed variant 0): lnL and sitewise lnL bit for bit the
    default run's, kept partials and lnL-only; with kept partials every partial and scaler too."""
    for k in _PLAN_VARS:
        monkeypatch.delenv(k, raising=False)
    base = {keep: _plan_base(case, keep) for keep in (True, False)}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rm, tree, names, codes, table, _ = _plan_problem(case)
    for keep in (True, False):
        l0, s0, p0, c0 = base[keep]
        tm = make_tm(tree, names, codes, table, rm, keep=keep)
        assert tm.likelihood() == l0
        np.testing.assert_array_equal(tm.sitewise_patterns(), s0)
        if keep:
            np.testing.assert_array_equal(tm.partials, p0)
            np.testing.assert_array_equal(tm.scale, c0)
    # lnL-only and kept partials run different builds of the same arithmetic per node
    np.testing.assert_array_equal(base[True][1], base[False][1])


def test_plans_reach_the_generic_and_chain_variants(monkeypatch):
    """The plan variants the two-state runs above take, read from the context
    (pu_ctx_plan_info): HBM read-backs (TV_GENERIC) under PU_LDS_SLOTS=0 and a chain plan
    (TV_CHAIN) under PU_SPLIT=2.  (TV_PTIP is decided per launch -- lnL-only, coded tips,
    eigen model, no PU_NO_PTIP -- and no facility reports it.)"""
    rm, tree, names, codes, table, _ = _plan_problem("taxa17")
    for k in _PLAN_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PU_LDS_SLOTS", "0")
    tm = make_tm(tree, names, codes, table, rm)
    assert N.ctx_plan(tm._ctx)["variant"] & TV_GENERIC
    monkeypatch.delenv("PU_LDS_SLOTS")
    monkeypatch.setenv("PU_SPLIT", "2")
    for keep in (True, False):
        tm = make_tm(tree, names, codes, table, rm, keep=keep)
        v = N.ctx_plan(tm._ctx)["variant"]
        assert v & TV_CHAIN and v & TV_GENERIC, v


@pytest.mark.parametrize("keep", [True, False])
def test_non_dfs_caller_order(oracle_mod, keep):
    """The caller's own post-order (sorted by subtree height, PU_NO_REORDER): children come
    from HBM (the general variant), the numbers are the planned order's."""
    rm = rates_of(4)
    tree, names, codes, table, _ = T.binary_problem(17, 257, PI0, rm.rates, seed=17)
    base = make_tm(tree, names, codes, table, rm, keep=keep)
    tm = TreeModel(keep_partials=keep, reorder=False)
    tm.set_alignment_codes(codes, table, names)
    tm.set_substitution_model(T.TwoState(PI0))
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tr = tm.traversal
    order = _height_order(tr.postorder_traversal)
    assert not np.array_equal(order, tr.postorder_traversal)
    tr.postorder_traversal = order
    tm.initialise()
    st = N.plan_stats(tr.n_nodes, order, tr.root_edge, 0, 2, N.PU_NO_REORDER)
    assert st["mem"] > 0
    assert N.ctx_plan(tm._ctx)["variant"] & TV_GENERIC
    gap = T.all_gap_columns(codes)
    got, want = tm.sitewise_patterns(), base.sitewise_patterns()
    np.testing.assert_allclose(got[~gap], want[~gap], rtol=1e-13)  # device against device
    assert np.all(np.abs(got[gap]) <= gap_atol(17))
    check_site(tm.sitewise_patterns(), oracle_state(oracle_mod, tm)["site_lnl"], codes, 17)
    if keep:
        assert_partials_close(tm.partials, base.partials, rtol=1e-13)


def test_new_topology_reuses_resident_tips():
    rm = rates_of(4)
    tree_a, names, codes, table, _ = T.binary_problem(17, 257, PI0, rm.rates, seed=31)
    tree_b = random_tree(np.random.default_rng(32), 17)
    tm = make_tm(tree_a, names, codes, table, rm)
    lnl_a, parts_a = tm.likelihood(), tm.partials
    ctx = tm._ctx.value
    for tree, ref in ((tree_b, make_tm(tree_b, names, codes, table, rm)), (tree_a, None)):
        tm.set_tree(tree)
        tm.initialise()
        assert tm._ctx.value == ctx  # reused, tips resident
        if ref is None:
            assert tm.likelihood() == lnl_a
            np.testing.assert_array_equal(tm.partials, parts_a)
        else:
            assert tm.likelihood() == ref.likelihood() != lnl_a
            np.testing.assert_array_equal(tm.sitewise_patterns(), ref.sitewise_patterns())
            np.testing.assert_array_equal(tm.partials, ref.partials)
            np.testing.assert_array_equal(tm.scale, ref.scale)


# ---------------------------------------------------------------- edges (k_edge<2>)
def edge_setup(n_taxa=14, n_sites=700, seed=2, C=4, gap_taxon=True, **kw):
    """gap_taxon=False for the optimisers: lnL does not depend on the length of an all-gap
    taxon's branch, so its 'optimum' is decided by the rounding of a zero derivative."""
    rm = rates_of(C)
    tree, names, codes, table, _ = T.binary_problem(n_taxa, n_sites, PI0, rm.rates, seed=seed,
                                                    gap_taxon=gap_taxon)
    tm = make_tm(tree, names, codes, table, rm, **kw)
    return tm, tm.substitution_model, rm, tm.traversal, codes


def test_root_edge_lnl_bitwise_equals_traversal():
    tm, m, rm, tr, _ = edge_setup()
    site_trav = tm.sitewise_patterns().copy()
    lnl, site = tm._edge_lnl(*tr.root_edge)
    np.testing.assert_array_equal(site, site_trav)
    close(lnl, tm.likelihood(), 1e-12)


@pytest.mark.parametrize("coded", [True, False])
def test_any_edge_uses_current_partials(oracle_mod, coded):
    tm, m, rm, tr, codes = edge_setup(coded=coded)
    st = oracle_state(oracle_mod, tm)
    ev, el, iv = m.engine_eigen()
    P, S = st["partials"], st["scale"]
    # the tips below each node: an edge lnL of current (post-order) partials sees only the tips
    # below its two ends, and is log(1) = 0 where all of those are gaps
    tip_row = {tr.names[n]: i for n, i in tm.names.items()}
    below = {v: [i] for v, i in tip_row.items()}
    for p, a, b in tr.postorder_traversal:
        below[int(p)] = below[int(a)] + below[int(b)]
    worst = 0.0
    for p, a, b in tr.postorder_traversal[::5]:
        for u, v in ((int(a), int(p)), (int(p), int(b))):
            site = tm.compute_likelihood_at_edge(u, v)
            ref = oracle_mod.edge_lnl(P[u], S[u], P[v], S[v], ev, el, iv, tr.brlens[u, v],
                                      rm.rates, rm.weights, m.freqs)
            worst = max(worst, check_site(site, ref, codes[sorted(set(below[u] + below[v]))],
                                          14)[0])
    print("edge lnL (coded=%s): max relative sitewise error %.2e" % (coded, worst))
    close(tm.likelihood(), st["lnl"], 1e-12)


def test_edge_derivatives_vs_oracle(oracle_mod):
    tm, m, rm, tr, _ = edge_setup()
    st = oracle_state(oracle_mod, tm)
    ev, el, iv = m.engine_eigen()
    P, S = st["partials"], st["scale"]
    a, b = tr.root_edge
    worst = 0.0
    for t in (None, 1e-6, 0.05, 0.7, 3.0):
        got = tm.edge_derivatives(a, b, t)
        tt = tr.root_length() if t is None else t
        ref = oracle_mod.edge_derivs(P[a], S[a], P[b], S[b], ev, el, iv, tt, rm.rates,
                                     rm.weights, m.freqs)
        for k in range(3):
            worst = max(worst, abs(got[k] - ref[k]) / max(1.0, abs(ref[k])))
            close(got[k], ref[k], 1e-10)
    print("edge derivatives: max error relative to max(1, |v|) %.2e" % worst)
    close(tm.edge_derivatives(a, b)[0], tm.likelihood(), 1e-12)


@pytest.mark.parametrize("C", [1, 4])
def test_two_taxon_derivatives_vs_closed_form(C):
    """Two taxa, 700 sites with gaps: the root edge joins the two tips, so lnL, lnL' and lnL''
    at any length t have a closed form.  Lengths from 1e-3 up: the eigen form of P (the
    kernel's and the oracle's alike) gets a short branch's off-diagonal entry by a cancellation
    whose relative error is 1e-16 / (mu t pi_j) -- at t = 1e-6 the CPU oracle itself is 1.5e-10
    off the closed form in lnL'' (tests/test_twostate_reference.py), which is the tolerance."""
    rm = rates_of(C)
    tree, names, codes, table, tipv = T.binary_problem(2, 700, PI0, rm.rates, seed=5)
    tm = make_tm(tree, names, codes, table, rm)
    tr = tm.traversal
    a, b = tr.root_edge
    node_name = {v: k for k, v in tr.names.items()}
    x, y = tipv[node_name[a]], tipv[node_name[b]]
    worst = 0.0
    for t in (None, 1e-3, 0.05, 0.7, 3.0):
        got = tm.edge_derivatives(a, b, t)
        tt = tr.root_length() if t is None else t
        ref = T.closed_two_taxon_derivs(PI0, x, y, tt, rm.rates, rm.weights)
        for k in range(3):
            worst = max(worst, abs(got[k] - ref[k]) / max(1.0, abs(ref[k])))
            close(got[k], ref[k], 1e-10)
    site = T.closed_two_taxon_site_lnl(PI0, x, y, tr.root_length(), 0.0, rm.rates, rm.weights)
    e_site, _ = check_site(tm.sitewise_patterns(), site, codes, 2)
    print("C=%d two taxa vs closed form: derivatives %.2e, sitewise %.2e" % (C, worst, e_site))
    assert abs(tm.likelihood() - site.sum()) <= 1e-12 * abs(site.sum())


def test_reorientation_updates_vs_oracle(oracle_mod):
    """update_partials along the optimising traversal gives oracle.clv_c's partials, and every
    re-oriented edge the root lnL (the pulley principle)."""
    tm, m, rm, tr, _ = edge_setup(n_taxa=11, n_sites=500, seed=9)
    st = oracle_state(oracle_mod, tm)
    ev, el, iv = m.engine_eigen()
    P, S = st["partials"], st["scale"]
    lnl0 = tm.likelihood()
    for row in tr.optimising_traversal:
        if row[0] >= 0:
            p, x, y = (int(v) for v in row[:3])
            bl = [tr.brlens[p, x], tr.brlens[p, y]]
            tm.update_partials([row[:3]], [bl])
            cml = np.zeros(S[p].shape)
            P[p] = oracle_mod.clv_c(oracle_mod.pmatrix(ev, el, iv, bl[0], rm.rates),
                                    oracle_mod.pmatrix(ev, el, iv, bl[1], rm.rates), P[x], P[y],
                                    S[x], S[y], cml)
            S[p] = cml
            gp, gs = tm.node_partials(p)
            assert_partials_close(gp, P[p], rtol=1e-11)
            np.testing.assert_allclose(gs, S[p], rtol=1e-12, atol=1e-9)
        if row[3] >= 0:
            close(tm.edge_derivatives(int(row[3]), int(row[4]))[0], lnl0, 1e-11)


@pytest.mark.parametrize("coded", [True, False])
def test_optimise_sweep_vs_oracle(oracle_mod, coded):
    tm, m, rm, tr, _ = edge_setup(n_taxa=10, n_sites=600, seed=4, coded=coded, gap_taxon=False)
    ev, el, iv = m.engine_eigen()
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    ops, bl0, root, rl0 = tr.postorder_traversal.copy(), tr.op_lengths(), tr.root_edge, \
        tr.root_length()
    lens, lnl_ref = oracle_mod.optimise_sweep(tips, ops, bl0, root, rl0, ev, el, iv, m.freqs,
                                              rm.rates, rm.weights, tr.optimising_traversal,
                                              tr.n_nodes)
    lnl0 = tm.likelihood()
    lnl = tm.optimise_branch_lengths(tol=1e-8, max_iter=50)
    assert lnl > lnl0
    close(lnl, lnl_ref, 1e-9)
    worst = 0.0
    for key, t in lens.items():
        got = tr.brlens[key]
        worst = max(worst, abs(got - t) / max(t, 1e-3))
        assert abs(got - t) <= 1e-6 * max(t, 1e-3), (key, got, t)
    print("sweep (coded=%s): max length error %.2e, lnL error %.2e" % (
        coded, worst, abs(lnl - lnl_ref) / abs(lnl_ref)))
    close(tm.likelihood(), lnl, 1e-12)
    ref2, _ = oracle_mod.tree_lnl(tips, ops, tr.op_lengths(), root, tr.root_length(), ev, el, iv,
                                  m.freqs, rm.rates, rm.weights, n_nodes=tr.n_nodes)
    close(lnl, ref2, 1e-12)


# ---------------------------------------------------------------- device Newton, minimisers
def _newton_stats(tm):
    launches, evals = ctypes.c_int(), ctypes.c_int()
    N.check(N.lib().pu_ctx_newton_stats(tm._ctx, ctypes.byref(launches), ctypes.byref(evals)),
            tm._ctx)
    return launches.value, evals.value


@pytest.mark.parametrize("tpw", ["1", "2"])
@pytest.mark.parametrize("C,n_sites", [(1, 700), (2, 5000), (4, 900)])
def test_device_newton_matches_the_host_loop(monkeypatch, C, n_sites, tpw):
    """k_edge_newton<2, TPW> (PU_NT_TPW tiles per wave) against the host loop of k_edge
    launches: lengths 1e-9 relative, lnL 1e-12, and every optimisation ran on the device."""
    monkeypatch.setenv("PU_NT_TPW", tpw)
    rm = rates_of(C)
    n_taxa = 16
    tree, names, codes, table, _ = T.binary_problem(n_taxa, n_sites, PI0, rm.rates, seed=31,
                                                    gap_taxon=False)

    def run(device):
        monkeypatch.setenv("PU_EDGE_DEVICE_NEWTON", "1" if device else "0")
        tm = make_tm(tree, names, codes, table, rm)
        a, b = tm.traversal.root_edge
        t1, l1 = tm.optimise_edge(a, b, tol=1e-10)
        p, c1, _ = (int(v) for v in tm.traversal.postorder_traversal[2])
        t2, l2 = tm.optimise_edge(p, c1, tol=1e-8, max_iter=3)
        lnl = tm.optimise_branch_lengths(tol=1e-8, max_iter=50)
        return (t1, l1, t2, l2, lnl, dict(tm.traversal.brlens)), _newton_stats(tm)

    host, hs = run(False)
    dev, ds = run(True)
    assert hs == (0, 0)
    assert ds[0] == 2 + 2 * n_taxa - 3 and ds[1] > ds[0]
    for i in (0, 2):
        assert abs(dev[i] - host[i]) <= 1e-9 * max(host[i], 1e-3), (i, dev[i], host[i])
    for i in (1, 3, 4):
        close(dev[i], host[i], 1e-12)
    for k, v in host[5].items():
        assert abs(dev[5][k] - v) <= 1e-9 * max(v, 1e-3), (k, dev[5][k], v)


def test_device_newton_falls_back_at_five_categories(monkeypatch, oracle_mod):
    """C = 5 is more than k_edge_newton holds per lane: the host loop runs, and the sweep is
    the oracle's."""
    monkeypatch.delenv("PU_EDGE_DEVICE_NEWTON", raising=False)
    tm, m, rm, tr, _ = edge_setup(n_taxa=10, n_sites=500, seed=32, C=5, gap_taxon=False)
    ev, el, iv = m.engine_eigen()
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    lens, lnl_ref = oracle_mod.optimise_sweep(tips, tr.postorder_traversal.copy(),
                                              tr.op_lengths(), tr.root_edge, tr.root_length(),
                                              ev, el, iv, m.freqs, rm.rates, rm.weights,
                                              tr.optimising_traversal, tr.n_nodes)
    lnl0 = tm.likelihood()
    lnl = tm.optimise_branch_lengths(tol=1e-8, max_iter=50)
    assert lnl > lnl0 and _newton_stats(tm) == (0, 0)
    close(lnl, lnl_ref, 1e-9)
    for key, t in lens.items():
        assert abs(tr.brlens[key] - t) <= 1e-6 * max(t, 1e-3), (key, tr.brlens[key], t)


@pytest.mark.parametrize("method", ["brent", "dbrent"])
def test_minimise_edge_is_the_reference_minimiser(monkeypatch, method):
    """pu_minimise_edge on two states, (C, S) = (4, 3000): the host driver takes the Python
    restatement's steps bit for bit, the device driver reaches the same optimum (dbrent to its
    tolerance, brent to 1e-6 relative) and lnL to 1e-12, in one launch."""
    tm, m, rm, tr, _ = edge_setup(n_taxa=14, n_sites=3000, seed=41, gap_taxon=False)
    a, b = tr.root_edge
    key = tuple(sorted((a, b)))
    t_true = tr.brlens[key]
    for t0, bracket, tol in ((t_true, (1e-8, 10.0), 1e-8), (0.5 * t_true, (1e-6, 2.0), 1e-10),
                             (3.0 * t_true, (1e-8, 10.0), 1.5e-8)):
        res = {}
        for mode in ("py", "host", "device"):
            monkeypatch.setenv("PU_EDGE_DEVICE_NEWTON", "1" if mode == "device" else "0")
            if mode == "py":
                monkeypatch.setenv("PU_PY_MINIMISE", "1")
            else:
                monkeypatch.delenv("PU_PY_MINIMISE", raising=False)
            tr.brlens[key] = t0
            tm.update_branch_lengths()
            tm.likelihood()
            l0, _ = _newton_stats(tm)
            t, lnl = tm.optimise_edge(a, b, tol=tol, method=method, bracket=bracket)
            l1, _ = _newton_stats(tm)
            res[mode] = (t, lnl, tm.last_edge_evaluations, l1 - l0)
        assert res["host"][:3] == res["py"][:3], (t0, bracket, res)
        assert res["host"][3] == 0 and res["device"][3] == 1
        t_h, l_h = res["host"][:2]
        t_d, l_d = res["device"][:2]
        lim = (1e-6 if method == "brent" else 10 * tol) * max(t_h, 1e-3) + 1e-9
        assert abs(t_d - t_h) <= lim, (t_d, t_h)
        close(l_d, l_h, 1e-12)


# ---------------------------------------------------------------- batch
def batch_models(C, n_trees=5, n_taxa=20, n_sites=300):
    rm = rates_of(C)
    _, names, codes, table, _ = T.binary_problem(n_taxa, n_sites, PI0, rm.rates, seed=5)
    out = []
    for i in range(n_trees):
        tm = TreeModel(keep_partials=False)
        if out:
            tm.share_alignment(out[0])
        else:
            tm.set_alignment_codes(codes, table, names)
        tm.set_substitution_model(T.TwoState(PI0))
        tm.set_rate_model(rm)
        tm.set_tree(random_tree(np.random.default_rng(100 + i), n_taxa))
        tm.initialise()
        out.append(tm)
    return out, codes


def _site(tm):
    out = np.empty(tm._n_patterns())
    N.check(N.lib().pu_get_site_lnl(tm._ctx, N.ptr(out)), tm._ctx, "pu_get_site_lnl")
    return out


@pytest.mark.parametrize("env", [{}] + GRID_ENVS, ids=lambda e: ",".join(
    "%s=%s" % kv for kv in sorted(e.items())) or "default")
@pytest.mark.parametrize("C", [1, 4])
def test_batch_bitwise_and_vs_oracle(monkeypatch, oracle_mod, C, env):
    """k_pmatrix_lane_trees<2> and k_prune_trees<2, ...>: 5 trees x 20 taxa x 300 sites on one
    shared alignment, every grid order and build of test_batch_grid_orders_bitwise: each tree
    bit for bit its own launch, and the oracle's to tolerance."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tms, codes = batch_models(C)
    single = [tm.likelihood() for tm in tms]
    site1 = [_site(tm) for tm in tms]
    b = TreeBatch(tms)
    got = b.likelihoods()
    assert list(got) == single
    worst = 0.0
    for i, tm in enumerate(tms):
        s = b.sitewise(i)
        np.testing.assert_array_equal(s, site1[i])
        ref = oracle_state(oracle_mod, tm)
        worst = max(worst, check_site(s, ref["site_lnl"], codes, 20)[0])
        assert abs(got[i] - ref["lnl"]) <= 1e-12 * abs(ref["lnl"]), (i, got[i], ref["lnl"])
    print("batch C=%d %s: max relative sitewise error %.2e" % (C, env, worst))
    b.close()


def test_batch_refuses_three_categories():
    tms, _ = batch_models(3, n_trees=2, n_taxa=12)
    b = TreeBatch(tms)
    with pytest.raises(N.PhyloHipError, match="C = 1, 2 or 4"):
        b.enqueue()
    b.close()


# ---------------------------------------------------------------- ascertainment, facade
@pytest.mark.parametrize("C,weighted,coded", [(1, False, True), (1, False, False),
                                              (1, True, True), (4, True, True),
                                              (4, True, False), (4, False, True)])
def test_ascertainment_vs_oracle(oracle_mod, C, weighted, coded):
    """The Lewis correction on binary characters (its main use: morphological data), the
    reference's form and the weighted form, against oracle.tree_lnl_ascbias: the correction
    1e-12, sitewise rtol 1e-12, total 1e-9 relative; the reference's unweighted form is NaN for
    Gamma C > 1 and so is the engine's."""
    rm = GammaRateModel(C, 0.5)
    m = T.TwoState(PI0)
    S = 800
    tree, names, codes, table, tipv = T.binary_problem(12, S, PI0, rm.rates, seed=21)
    tm = TreeModel(device=0, compact_tips=coded)
    if coded:
        tm.set_alignment_codes(codes, table, names)
    else:
        tm.set_alignment_partials(table[codes], names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.set_ascertainment_bias_correction(weighted=weighted)
    tm.initialise()
    tr = tm.traversal
    tips = {tr.names[n]: tipv[n] for n in names}
    ev, el, iv = m.engine_eigen()
    lnl, site, corr = oracle_mod.tree_lnl_ascbias(tips, tr.postorder_traversal, tr.op_lengths(),
                                                  tr.root_edge, tr.root_length(), ev, el, iv,
                                                  m.freqs, rm.rates, rm.weights,
                                                  n_nodes=tr.n_nodes, weighted=weighted)
    got_site = tm.compute_likelihood_at_edge(*tr.root_edge)
    assert got_site.shape == (S,)
    c = np.zeros(1)
    N.check(N.lib().pu_get_ascertainment_correction(tm._ctx, N.ptr(c)), tm._ctx)
    if np.isnan(corr):
        assert C > 1 and not weighted
        assert np.isnan(c[0]) and np.isnan(tm.likelihood())
        return
    np.testing.assert_allclose(c[0], corr, rtol=1e-12)
    # every site carries -correction, so the all-gap columns are not near zero here
    np.testing.assert_allclose(got_site, site[:S], rtol=1e-12)
    print("ascertainment C=%d weighted=%s coded=%s: correction error %.2e, sitewise %.2e" % (
        C, weighted, coded, abs(c[0] - corr) / abs(corr), rel_err(got_site, site[:S])))
    close(tm.likelihood(), lnl, 1e-9)
    with pytest.raises(N.PhyloHipError):
        tm.edge_derivatives(*tr.root_edge)


def test_facade_binary_strings(oracle_mod):
    """TreeModel.set_alignment(records, BINARY) on strings over 0, 1, ? and -, compressed and
    not: the same total lnL, the oracle's."""
    rm = rates_of(4)
    tree, names, codes, table, tipv = T.binary_problem(9, 400, PI0, rm.rates, seed=8)
    rng = np.random.default_rng(8)
    chars = np.where(codes == T.STATE_CODE[0], "0", np.where(codes == T.STATE_CODE[1], "1",
                     np.where(rng.random(codes.shape) < 0.5, "?", "-")))
    records = [(n, "".join(row)) for n, row in zip(names, chars)]
    assert {c for _, s in records for c in s} == set("01?-")
    lnls = {}
    for compress in (True, False):
        tm = TreeModel()
        tm.set_alignment(records, A.BINARY, compress=compress)
        tm.set_substitution_model(T.TwoState(PI0))
        tm.set_rate_model(rm)
        tm.set_tree(tree)
        tm.initialise()
        lnls[compress] = tm.likelihood()
        if compress:
            assert tm.alignment.shape[1] < 400
        else:
            np.testing.assert_array_equal(np.asarray(tm.alignment),
                                          np.stack([tipv[n] for n in names]))
            check_site(tm.compute_likelihood_at_edge(*tm.traversal.root_edge),
                       oracle_state(oracle_mod, tm)["site_lnl"], codes, 9)
    ref = oracle_state(oracle_mod, tm)["lnl"]
    assert abs(lnls[False] - ref) <= 1e-12 * abs(ref)
    assert abs(lnls[True] - ref) <= 1e-12 * abs(ref)
    assert abs(lnls[True] - lnls[False]) <= 1e-12 * abs(ref)
