"""The extended-precision restatement (tests/hp_reference.py) checks itself, the committed
fixtures tests/golden/hp_*.npz are what tests/golden/make_golden_hp.py writes, the oracle's error
against them is the stored yardstick, and the comparison of tests/hp_check.py -- what
tests/test_gpu_hp.py applies to the device -- rejects values that are wrong.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest

import hp_cases as H
import hp_check as CK
import twostate as T
from conftest import GOLDEN, load_golden

pytest.importorskip("mpmath")
from mpmath import mp, mpf  # noqa: E402

import hp_reference as R  # noqa: E402


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_hp",
                                                  os.path.join(GOLDEN, "make_golden_hp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gtr():
    return R.Exact.of_model(H.model_of("gtr"))


@pytest.fixture(scope="module")
def small(gtr):
    """The 8-taxon GTR + I + G4 case on its first six patterns: (schedule pieces, tips, rm, w)."""
    table, _, _ = H.table_of("gtr")
    codes, w = H.t8_tips("gtr")
    tr, rows = H.schedule(H.t8_newick("r5"), H.T8_NAMES)
    tips = {n: table[codes[i, :6]].astype(int).tolist() for n, i in rows.items()}
    return tr, tips, H.rate_model_of("g05i"), w[:6]


def _mat_err(a, b):
    return max(abs(a[i, j] - b[i, j]) for i in range(a.rows) for j in range(a.cols))


# ---------------------------------------------------------------- the restatement checks itself
def test_p_is_a_transition_matrix(gtr):
    lg = R.Exact.of_model(H.model_of("lg"))
    for X, taus in ((gtr, (0.0, 1e-14, 1e-8, 0.1, 1.0, 1000.0)), (lg, (0.0, 0.1))):
        assert _mat_err(X.p(0.0), mp.eye(X.K)) == 0
        for tau in taus:
            P = X.p(tau)
            assert max(abs(sum(P[i, j] for j in range(X.K)) - 1) for i in range(X.K)) < mpf(10) ** -40
            # reversibility of the assembled Q: pi_i P_ij = pi_j P_ji
            assert max(abs(X.pi[i] * P[i, j] - X.pi[j] * P[j, i])
                       for i in range(X.K) for j in range(X.K)) < mpf(10) ** -40


def test_semigroup(gtr):
    for s, t in ((1e-8, 1e-4), (0.1, 1.0), (1.0, 10.0)):
        both = gtr.p(mpf(s) + mpf(t))
        assert _mat_err(both, gtr.p(s) * gtr.p(t)) < mpf(10) ** -40


def test_two_state_closed_form():
    """tests/twostate.py's closed form (expm1 keeps it to a few ulp) for P, P' and P''."""
    pi0 = 0.25
    m = T.TwoState(pi0)
    X = R.Exact.of_model(m)
    rates = np.array([0.3, 1.0, 2.5])
    for t in (1e-8, 1e-3, 0.1, 5.0):
        for order in range(3):
            got = R.to_float(X.p_cats(t, rates, order))
            np.testing.assert_allclose(got, T.closed_p(pi0, t, rates, order), rtol=1e-14, atol=0)


def test_edge_derivatives_against_central_differences(gtr, small):
    tr, tips, rm, w = small
    args = (tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge, tr.root_length())
    edges = [tr.root_edge, (0, int(tr.postorder_traversal[0][0]))]
    for edge in edges:
        ops, lens, t0 = R.reroot(*args[1:], edge)
        part = gtr.partials(tips, ops, lens, rm.rates)
        for t in (mpf(t0), mpf("0.37")):
            h = t * mpf(10) ** -12  # truncation (h / t)^2 = 1e-24 relative
            f = {k: gtr.edge(tips, ops, lens, edge, t0, edge, t + k * h, rm.rates, rm.weights, w,
                             rerooted=True, part=part) for k in (-1, 0, 1)}
            d1 = (f[1]["lnl"] - f[-1]["lnl"]) / (2 * h)
            d2 = (f[1]["lnl"] - 2 * f[0]["lnl"] + f[-1]["lnl"]) / (h * h)
            assert abs(d1 - f[0]["d1"]) <= mpf(10) ** -18 * max(1, abs(d1))
            assert abs(d2 - f[0]["d2"]) <= mpf(10) ** -15 * max(1, abs(d2))


def test_pulley_principle(gtr, small):
    tr, tips, rm, w = small
    args = (tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge, tr.root_length())
    ref = gtr.prune(*args, rm.rates, rm.weights, w)
    for (a, b), t in tr.brlens.items():
        got = gtr.edge(*args, (a, b), t, rm.rates, rm.weights, w)
        assert abs(got["lnl"] - ref["lnl"]) <= mpf(10) ** -40 * abs(ref["lnl"])
        assert all(abs(x - y) <= mpf(10) ** -40 for x, y in zip(got["site"], ref["site"]))


# ---------------------------------------------------------------- the fixtures are current
@pytest.mark.parametrize("name", ["hp_pmat_gtr", "hp_tree8_gtr", "hp_deep"])
def test_gtr_fixtures_are_current(name, oracle_mod):
    """Everything but the oracle's own errors (which may differ with the host's BLAS and are held
    by test_yardstick_holds) is regenerated bit for bit."""
    new, old = _generator().FILES[name](oracle_mod), load_golden(name)
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        if "E_orc" not in k:
            assert np.array_equal(np.asarray(new[k]), old[k], equal_nan=True), k


def test_three_lg_matrices_are_current():
    g = load_golden("hp_pmat_lg")
    X = R.Exact.of_model(H.model_of("lg"))
    for rmn, length, c in (("c1", 1e-8, 0), ("g01", 1.0, 2), ("g05", 1000.0, 3)):
        lens = g[rmn + "_len"]
        o, s = (int(v[0]) for v in np.nonzero(lens == length))
        tau = mpf(float(length)) * mpf(float(g[rmn + "_rates"][c]))
        assert np.array_equal(R.to_float(X.p(tau)), g[rmn + "_P"][o, s, c]), (rmn, length)


# ---------------------------------------------------------------- the yardstick holds
def _errors(orc, name):
    g = load_golden(name)
    if name.startswith("hp_pmat"):
        return g, H.oracle_errors_pmat(orc, g, name.split("_")[-1])
    if name.startswith("hp_tree8"):
        return g, H.oracle_errors_tree8(orc, g, name.split("_")[-1])
    return g, H.oracle_errors_deep(orc, g)


@pytest.mark.parametrize("name", ["hp_pmat_gtr", "hp_pmat_lg", "hp_tree8_gtr", "hp_tree8_lg",
                                  "hp_deep"])
def test_yardstick_holds(name, oracle_mod):
    """The oracle's error recomputed here is at most twice the stored E_orc_*, value by value:
    per matrix, per pattern, per length of an edge."""
    g, new = _errors(oracle_mod, name)
    assert sorted(new) == sorted(k for k in g.files if "E_orc" in k)
    for k, v in new.items():
        assert np.all(v <= 2 * g[k]), (k, float(np.max(v)), float(np.max(g[k])))


@pytest.mark.parametrize("model", H.MODELS)
def test_one_rounding_is_no_yardstick_for_a_single_value(model):
    """Why E_orc_* of a pattern or of one length of an edge is the largest error over several
    fp64 roundings of the oracle's formula (tests/hp_cases.py) and not the oracle's own error
    alone (E_orc0_*): value by value the oracle's own error falls below a quarter of another
    rounding's -- an equally valid fp64 evaluation would then miss a 4 x E_orc0 bound -- although
    over a whole case the two differ by less than a factor of two.  That is the scatter of single
    values, not a lost digit."""
    g = load_golden("hp_tree8_" + model)
    n_low = 0
    for k in g.files:
        if "E_orc_" in k and k.replace("E_orc_", "E_orc0_") in g.files and g[k].ndim:
            own, many = g[k.replace("E_orc_", "E_orc0_")], g[k]
            assert np.all(own <= many)
            assert many.max() <= 2 * own.max(), k
            n_low += int((own < 0.25 * many).sum())
    print("%s: %d single values with E_orc0 < E_orc / 4" % (model, n_low))
    assert n_low >= 5
    if model == "lg":
        # the two values at which the device missed 4 x E_orc0 (length-5 edge, d1)
        for rmn in ("g01", "g05i"):
            r = g[rmn + "_E_orc0_edge_r5"][:, 1] / g[rmn + "_E_orc_edge_r5"][:, 1]
            assert r.min() < 0.25, (rmn, r)


# ---------------------------------------------------------------- the checker can fail
EPS = 2.0 ** -40


@pytest.mark.parametrize("model", H.MODELS)
@pytest.mark.parametrize("rmn", H.P_RATE_MODELS)
def test_checker_rejects_perturbed_eigenvalues(model, rmn, oracle_mod):
    """The oracle's P with every eigenvalue multiplied by 1 + 2^-40, matrix by matrix.  The
    unperturbed oracle passes everywhere.  Every matrix with 1e-2 <= tau <= 10 is rejected.  Beyond
    that P is the stationary matrix to the last bit -- e^(lambda tau) of the slowest non-zero
    eigenvalue, -0.27 (LG) and -0.49 (GTR), is below 2e-12 at tau = 100, times 2^-40 tau lambda --
    so that no comparison can tell the two apart: there the test asserts just that, |perturbed -
    unperturbed| < 1e-15, and asks no rejection."""
    g = load_golden("hp_pmat_" + model)
    m = H.model_of(model)
    ev, el, iv = m.engine_eigen()
    lens, rates, truth = g[rmn + "_len"], g[rmn + "_rates"], g[rmn + "_P"]
    Ea, Er = g[rmn + "_E_orc_abs"], g[rmn + "_E_orc_rel"]
    n_rejected = 0
    for o in range(lens.shape[0]):
        for s in range(2):
            good = oracle_mod.pmatrix(ev, el, iv, lens[o, s], rates)
            bad = oracle_mod.pmatrix(ev, el * (1 + EPS), iv, lens[o, s], rates)
            for c, r in enumerate(rates):
                tau = lens[o, s] * r
                a, b = CK.check_p(good[c], truth[o, s, c], Ea[o, s, c], Er[o, s, c])
                assert a.ok and b.ok
                a, b = CK.check_p(bad[c], truth[o, s, c], Ea[o, s, c], Er[o, s, c])
                if 1e-2 <= tau <= 10:
                    assert not (a.ok and b.ok), (lens[o, s], r, str(a), str(b))
                    n_rejected += 1
                elif tau >= 100:
                    assert np.abs(bad[c] - good[c]).max() < 1e-15
    assert n_rejected >= 3


def test_checker_and_a_scaled_category(oracle_mod):
    """One category's root partials scaled by 1 + eps on the well-conditioned case (the 200-taxon
    caterpillar, E_orc 3.4e-13 per pattern).  That moves a pattern's lnL by the category's share
    of the pattern's likelihood times eps.  With eps = 1e-11 this is below the 1e-10 that the
    suite's own tolerance adds to every site bound, so no comparison built on that bound can
    reject it; the checker must still measure it (to 1e-13), and it must reject eps = 1e-9, where
    the shift passes the bound."""
    g = load_golden("hp_deep")
    model, rm = H.model_of("gtr"), H.rate_model_of("g05")
    args = (oracle_mod, H.text(g["newick"]), H.DEEP_NAMES, g["codes"], g["table"], model, rm,
            g["weights"])
    clean = H.oracle_tree(*args)
    assert np.count_nonzero(clean["scale"]) > 0
    share = g["g05_f"] * rm.weights / (g["g05_f"] * rm.weights).sum(axis=1, keepdims=True)
    c = int(np.argmax(share.max(axis=0)))
    assert share[:, c].max() > 0.25
    E = g["g05_E_orc_site"]
    assert CK.check_site(clean["site_lnl"], g["g05_site"], E).ok
    shift = {}
    for eps in (1e-11, 1e-9):
        bad = H.oracle_tree(*args, cat_scale=(c, 1 + eps))
        shift[eps] = bad["site_lnl"] - clean["site_lnl"]
        np.testing.assert_allclose(shift[eps], share[:, c] * eps, rtol=0, atol=1e-13)
        r = CK.check_site(bad["site_lnl"], g["g05_site"], E)
        assert abs(r.err - np.abs(bad["site_lnl"] - g["g05_site"]).max()) == 0
        assert r.ok == (eps == 1e-11), (eps, str(r))
    assert share[:, c].max() * 1e-9 > CK.FACTOR * E.max() + CK.TOL_SITE
