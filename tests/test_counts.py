"""Per-edge joint count matrices and the gradients built on them, on the CPU: the
restatement of tests/counts_reference.py against finite differences of the oracle's lnL, the
Frechet formula of phylo_utils_amd/gradient.py against scipy, the invariant of M, and the
``phy --fit`` plumbing.  Needs no device."""
import types

import numpy as np
import pytest

import counts_reference as R

from phylo_utils_amd import gradient as G
from phylo_utils_amd import modelfit, phy
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import (GammaRateModel, InvariantGammaModel,
                                         InvariantSitesModel, UniformRateModel)
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES

CPU_CASES = ("dna-pendant-root-4x70-C4", "dna-8x65-C3")


@pytest.fixture(scope="module", params=CPU_CASES)
def ref(request, oracle_mod):
    prob = R.problem(request.param)
    tr, e, tips, res = R.restate(oracle_mod, prob)
    return dict(case=request.param, prob=prob, tr=tr, e=e, tips=tips, res=res)


def _five(ref):
    """alpha, one exchangeability, one frequency, one tip length, one internal length."""
    res, tr = ref["res"], ref["tr"]
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    edges = [(int(a), int(b)) for a, b in res["edges"]]
    tip = next(e for e in edges[1:] if e[0] not in internal)
    inner = [e for e in edges if e[0] in internal and e[1] in internal][-1]
    return ["alpha", ("rates", 1), ("freqs", 1), ("length", tip), ("length", inner)]


def test_restatement_against_finite_differences(ref, oracle_mod):
    """Formulas (1)-(3) on the restatement's M against central differences of the oracle's lnL
    at h = 1e-6, for the five parameters of _five, relative to the largest of the five
    derivatives.  Measured worst: quartet 1.43e-8, dna-8x65-C3 3.96e-8 (the frequency both
    times; the rounding of lnL, ~1e-16 |lnL| with |lnL| ~ 1e3, over 2h = 2e-6 is ~5e-8 absolute,
    which is what is seen).  The bound is ten times the worst measured value, 3.96e-8."""
    names = _five(ref)
    g = np.array([R.gradient(oracle_mod, ref["prob"], ref["tr"], ref["res"], n) for n in names])
    fd = np.array([R.fd_gradient(oracle_mod, ref["prob"], ref["tips"], ref["tr"], n)
                   for n in names])
    err = np.abs(g - fd) / np.abs(fd).max()
    print("%s: restatement vs finite differences %s, worst %.2e" % (
        ref["case"], ["%.2e" % v for v in err], err.max()))
    assert err.max() <= 3.96e-7


def test_gradient_module_on_the_restatement(ref, oracle_mod):
    """gradient.py's host algebra (Frechet form, analytic dQ/dtheta with the scale_q
    normalisation) on the restatement's M against the restatement's own gradient (central
    differences of P): 1e-8 of the largest derivative, the bound of the device test."""
    tm = types.SimpleNamespace(substitution_model=ref["prob"]["model"],
                               rate_model=ref["prob"]["rm"])
    res = ref["res"]
    names = ["alpha", "rates", "freqs"]
    got = G.model_gradient(tm, names, res)
    got = np.concatenate([np.atleast_1d(got[n]) for n in names])
    keys = ["alpha"] + [("rates", k) for k in range(5)] + [("freqs", k) for k in range(3)]
    want = np.array([R.gradient(oracle_mod, ref["prob"], ref["tr"], res, k) for k in keys])
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    bg = G.branch_gradient(tm, res)
    want = R.branch_gradient(oracle_mod, ref["prob"], res)
    got = np.array([bg[(int(a), int(b))] for a, b in res["edges"]])
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # dlnL/dQ along Q itself is the derivative in a common factor of all lengths
    gq = G.q_gradient(tm, res)
    along = np.sum(gq * ref["prob"]["model"].q())
    assert abs(along - np.dot(got, res["lengths"])) <= 1e-9 * np.abs(got * res["lengths"]).sum()
    d_rate, d_weight = G.rate_gradient(tm, res)
    assert abs(d_rate.dot(tm.rate_model.rates) - along) <= 1e-9 * np.abs(got * res["lengths"]).sum()
    assert np.allclose(d_weight.dot(tm.rate_model.weights), ref["prob"]["weights"].sum(),
                       rtol=1e-12)


def test_invariant(ref, oracle_mod):
    """sum_c sum_ij M[c][i][j] pi_j P_c[j][i] = sum pw on every edge, and every edge's lnL is the
    tree's."""
    inv = R.invariant(ref["res"], ref["e"], oracle_mod)
    assert np.abs(inv / ref["prob"]["weights"].sum() - 1).max() <= 1e-12
    assert np.abs(ref["res"]["edge_lnl"] / ref["res"]["lnl"] - 1).max() <= 1e-12
    assert len(ref["res"]["edges"]) == 2 * len(ref["prob"]["names"]) - 3


@pytest.mark.parametrize("model,taus", [
    (SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), (0.01, 0.4, 3.0)),
    (SM.JC69(), (0.3,)), (SM.K80(2.5), (0.3,)), (SM.LG(), (0.3,))],
    ids=["GTR", "JC69", "K80", "LG"])
def test_frechet_formula_against_scipy(model, taus):
    from scipy.linalg import expm_frechet
    rng = np.random.default_rng(4)
    ev, el, iv = model.engine_eigen()
    q = model.q()
    for tau in taus:
        dq = rng.normal(size=q.shape)
        want = expm_frechet(q * tau, dq * tau, compute_expm=False)
        got = G.frechet(ev, el, iv, tau, dq)
        assert np.linalg.norm(got - want) <= 1e-10 * np.linalg.norm(want), (tau,)


def test_cli_fit_parsing_and_model_string():
    args = phy.parse_cli(["-t", "a", "-s", "b"])
    assert args.fit is None
    assert phy.parse_cli(["-t", "a", "-s", "b", "--fit"]).fit == ""
    assert phy.parse_cli(["-t", "a", "-s", "b", "--fit", "alpha,kappa"]).fit == "alpha,kappa"
    with pytest.raises(ValueError, match="--fit excludes"):
        phy.validate_args(phy.parse_cli(["-s", "b", "--distances", "--fit"]))
    cases = [(SM.GTR([1.2, 3.456789012345, 0.8, 1.1, 4.2], CFG2_FREQS), GammaRateModel(4, 0.6125)),
             (SM.HKY85(2.25, CFG2_FREQS), GammaRateModel(5, 1.5)),
             (SM.K80(3.0), UniformRateModel()), (SM.JC69(), UniformRateModel()),
             (SM.F81(CFG2_FREQS), UniformRateModel()),
             (SM.F84(1.5, CFG2_FREQS), GammaRateModel(4, 0.5)),
             (SM.TN93(2.0, 3.0, 1.0, CFG2_FREQS), UniformRateModel()),
             (SM.LG(), GammaRateModel(4, 0.8)),
             (SM.WAG(freqs=np.full(20, 0.05)), UniformRateModel())]
    for m, rm in cases:
        text = modelfit.model_string(m, rm)
        desc = phy.parse_model_string(text)
        m2, rm2 = phy.build_model(desc), phy.build_rate_model(desc)
        assert type(m2) is type(m) and type(rm2) is type(rm), text
        assert np.allclose(m2.q(), m.q(), rtol=1e-9, atol=1e-12), text
        assert np.allclose(m2.freqs, m.freqs, rtol=1e-9), text
        assert np.allclose(rm2.rates, rm.rates, rtol=1e-9) and rm2.ncat == rm.ncat, text


def test_parameter_names():
    gtr, gam = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    assert modelfit.free_parameters(gtr, gam) == ["rates", "freqs", "alpha"]
    assert modelfit.free_parameters(SM.LG(), gam) == ["freqs", "alpha"]
    assert modelfit.free_parameters(SM.JC69(), UniformRateModel()) == []
    assert modelfit.free_parameters(SM.F84(1.5, CFG2_FREQS), gam) == ["kappa", "freqs", "alpha"]
    with pytest.raises(ValueError, match="valid: freqs, alpha"):
        G.check_params(SM.LG(), gam, ["rates"])
    with pytest.raises(ValueError, match="valid: rates, freqs$"):
        G.check_params(gtr, UniformRateModel(), ["alpha"])
    with pytest.raises(ValueError, match="valid: none"):
        G.check_params(SM.JC69(), UniformRateModel(), ["kappa"])
    # build_models round-trips the values it is given
    m, rm = modelfit.build_models(gtr, gam, dict(alpha=0.9, rates=np.arange(1.0, 6.0),
                                                 freqs=np.array([0.1, 0.2, 0.3, 0.4])))
    assert rm.alpha == 0.9 and np.allclose(m.freqs, [0.1, 0.2, 0.3, 0.4])
    assert np.allclose(m.rates[SM._UPPER], [1, 2, 3, 4, 5, 1])
    f84 = SM.F84(1.5, CFG2_FREQS)
    assert abs(G.kappa_of(f84) - 1.5) < 1e-14


# ---------------------------------------------------------------- +I: pinvar
def _invariant_ref(oracle_mod, case):
    import invariant_reference as IR
    prob = IR.problem(case)
    tr, e, tips, res = R.restate(oracle_mod, prob)
    return dict(case=case, prob=prob, tr=tr, e=e, tips=tips, res=res)


@pytest.mark.parametrize("rm", [InvariantSitesModel(0.3), InvariantGammaModel(0.2, 3, 0.5),
                                InvariantGammaModel(0.45, 4, 1.7)], ids=repr)
def test_rate_model_derivs_of_the_invariant_models(rm):
    """rate_model_derivs against the central difference of rm.rates / rm.weights at h = 1e-6
    (truncation h^2 f''' / 6 ~ 1e-12, rounding eps / h ~ 2e-10 of the value): 1e-8 of the largest
    entry."""
    h = 1e-6
    names = ["pinvar"] + (["alpha"] if isinstance(rm, InvariantGammaModel) else [])
    for name in names:
        def at(delta):
            prob = dict(model=None, rm=rm)
            return R.shifted(prob, None, name, delta)[1]
        hi, lo = at(h), at(-h)
        dr, dw = G.rate_model_derivs(rm, name)
        fr, fw = (hi.rates - lo.rates) / (2 * h), (hi.weights - lo.weights) / (2 * h)
        assert np.abs(dr - fr).max() <= 1e-8 * max(np.abs(fr).max(), 1.0), name
        assert np.abs(dw - fw).max() <= 1e-8 * max(np.abs(fw).max(), 1.0), name
        assert dr[0] == 0.0 and abs(dw.sum()) <= 1e-15
    with pytest.raises(ValueError, match="no parameter"):
        G.rate_model_derivs(GammaRateModel(4, 0.5), "pinvar")


@pytest.mark.parametrize("case", ["dna-8x65-I", "dna-8x65-IG3"])
def test_model_gradient_pinvar_against_finite_differences(oracle_mod, case):
    """gradient.model_gradient's "pinvar" (and "alpha" under +I+G) on the restatement's M against
    central differences of the oracle's lnL: the step (h = 1e-6) and the bound (3.96e-7 of the
    largest derivative) of test_restatement_against_finite_differences.  Measured worst:
    dna-8x65-I 8.5e-9 (pinvar), dna-8x65-IG3 4.5e-9."""
    ref = _invariant_ref(oracle_mod, case)
    tm = types.SimpleNamespace(substitution_model=ref["prob"]["model"],
                               rate_model=ref["prob"]["rm"])
    names = ["pinvar"] + (["alpha"] if case.endswith("IG3") else [])
    got = G.model_gradient(tm, names, ref["res"])
    g = np.array([got[n] for n in names])
    fd = np.array([R.fd_gradient(oracle_mod, ref["prob"], ref["tips"], ref["tr"], n)
                   for n in names])
    rg = np.array([R.gradient(oracle_mod, ref["prob"], ref["tr"], ref["res"], n) for n in names])
    err = np.abs(g - fd) / np.abs(fd).max()
    print("%s: %s model_gradient %s, finite differences %s, worst %.2e" % (case, names, g, fd,
                                                                          err.max()))
    assert err.max() <= 3.96e-7
    assert np.abs(g - rg).max() <= 1e-8 * np.abs(rg).max()  # test_gradient_module_..'s bound
    # the invariable category carries a real share of dlnL/dw
    d_rate, d_weight = G.rate_gradient(tm, ref["res"])
    assert d_weight[0] > 0 and np.isfinite(d_rate).all()
    assert np.allclose(d_weight.dot(tm.rate_model.weights), ref["prob"]["weights"].sum(),
                       rtol=1e-12)


def test_pinvar_coordinates_and_parameter_names():
    """modelfit's logit coordinate: the round trip at pinvar 1e-6, 0.5 and 1 - 1e-6 loses at most
    the rounding of 1 - p (eps / 2 absolute) through the quotient, the logarithm and back, each
    of relative error eps on a quantity whose derivative in p is at most 1: 8 eps absolute; the
    chain rule is dp/dz = p (1 - p)."""
    eps = np.finfo(float).eps
    for p in (1e-6, 0.5, 1.0 - 1e-6):
        co = modelfit._Coordinates({"pinvar": p}, [], [])
        assert modelfit._LOGIT_BOX[0] < co.x0[0] < modelfit._LOGIT_BOX[1]
        back = co.values(co.x0)["pinvar"]
        assert abs(back - p) <= 8 * eps * max(p, 1 - p) and 0 < back < 1
        g = co.chain(co.x0, {"pinvar": back}, {"pinvar": 3.0}, None)
        assert abs(g[0] - 3.0 * p * (1 - p)) <= 1e-14
    gtr, lg = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), SM.LG()
    ig, i = InvariantGammaModel(0.2, 3, 0.5), InvariantSitesModel(0.3)
    assert modelfit.free_parameters(gtr, ig) == ["rates", "freqs", "alpha", "pinvar"]
    assert modelfit.free_parameters(lg, ig) == ["freqs", "alpha", "pinvar"]
    assert modelfit.free_parameters(gtr, i) == ["rates", "freqs", "pinvar"]
    assert modelfit.free_parameters(SM.JC69(), i) == ["pinvar"]
    with pytest.raises(ValueError, match="valid: rates, freqs, pinvar$"):
        G.check_params(gtr, i, ["alpha"])
    m, rm = modelfit.build_models(gtr, ig, dict(pinvar=0.35))
    assert isinstance(rm, InvariantGammaModel) and rm.pinvar == 0.35 and rm.alpha == 0.5
    assert rm.ncat == 4 and m is gtr
    m, rm = modelfit.build_models(gtr, ig, dict(alpha=0.9, pinvar=0.1))
    assert rm.pinvar == 0.1 and rm.alpha == 0.9
    m, rm = modelfit.build_models(gtr, i, dict(pinvar=0.6))
    assert isinstance(rm, InvariantSitesModel) and rm.pinvar == 0.6
    assert modelfit._values(gtr, ig, ["pinvar", "alpha"]) == {"pinvar": 0.2, "alpha": 0.5}
