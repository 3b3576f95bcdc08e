"""Per-edge joint count matrices, the gradients built on them and model fitting on the device
(DESIGN 4.18): the k_counts kernel through pu_counts_sweep and pu_edge_counts against the CPU
restatement (tests/counts_reference.py, itself pinned against finite differences of the oracle's
lnL in tests/test_counts.py).

Each case makes its device calls once (the `run` fixture); the tests below read what it kept."""
import ctypes

import numpy as np
import pytest

import counts_reference as R
import walk_errors as W

from phylo_utils_amd import TreeModel, gradient, modelfit
from phylo_utils_amd import _native as N
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem, random_tree

pytestmark = pytest.mark.gpu


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


def _problem(case):
    prob = R.problem(case)
    if case == "binary-8x70-Cmax":  # the limit of this kernel, not of k_ancestral
        assert prob["rm"].ncat == N.lib().pu_counts_max_cat(2)
    return prob


@pytest.fixture(scope="module", params=sorted(R.CASES))
def run(request, oracle_mod):
    prob = _problem(request.param)
    tr, e, tips, ref = R.restate(oracle_mod, prob)
    tm = _tm(prob)
    nod, par = (int(v) for v in ref["edges"][0])
    before = dict(lnl=tm.likelihood(), site=tm.sitewise_patterns().copy(),
                  parts=tm.node_partials(nod))
    # the single-edge calls on a fresh traversal: the root edge, at its length and at another
    edge = gradient.edge_counts_at(tm, nod, par)
    edge_t = gradient.edge_counts_at(tm, nod, par, length=0.37)
    st = R.state(oracle_mod, tips, tr, e, prob["weights"])
    ref_t = R.counts_of(oracle_mod, st["partials"], st["scale"], nod, par, 0.37, e,
                        np.asarray(prob["weights"], dtype=float))
    first = tm.edge_counts()
    after = dict(lnl=tm.likelihood(), site=tm.sitewise_patterns().copy(),
                 parts=tm.node_partials(nod))
    second = tm.edge_counts()
    return dict(case=request.param, prob=prob, tr=tr, e=e, tips=tips, ref=ref, tm=tm,
                before=before, after=after, first=first, second=second, edge=edge,
                edge_t=edge_t, ref_t=ref_t)


def _rel(got, ref):
    """Per matrix [..., K, K]: the largest error relative to that matrix's largest entry."""
    return np.abs(got - ref).max(axis=(-1, -2)) / np.abs(ref).max(axis=(-1, -2))


def test_sweep_against_the_restatement(run):
    ref, got = run["ref"], run["first"]
    assert got["edges"].tolist() == ref["edges"].tolist()
    assert np.array_equal(got["lengths"], ref["lengths"])
    assert len(got["edges"]) == 2 * len(run["prob"]["names"]) - 3
    assert len(set(tuple(sorted(e)) for e in got["edges"].tolist())) == len(got["edges"])
    worst = _rel(got["counts"], ref["counts"]).max()
    lnl = run["before"]["lnl"]
    worst_lnl = np.abs(got["edge_lnl"] - lnl).max() / abs(lnl)
    print("%s: counts worst relative error %.2e, edge_lnl %.2e" % (run["case"], worst, worst_lnl))
    assert worst <= 1e-10
    assert abs(lnl - ref["lnl"]) <= 1e-10 * abs(lnl)
    assert worst_lnl <= 1e-10


def test_invariant_on_the_device_output(run, oracle_mod):
    """sum_c sum_ij M[c][i][j] pi_j P_c[j][i] = sum pw on every edge."""
    inv = R.invariant(run["first"], run["e"], oracle_mod)
    total = run["prob"]["weights"].sum()
    worst = np.abs(inv / total - 1).max()
    print("%s: invariant worst relative error %.2e" % (run["case"], worst))
    assert worst <= 1e-12


def test_single_edge_call(run):
    (counts, lnl), got = run["edge"], run["first"]
    assert np.array_equal(counts, got["counts"][0])
    assert lnl == got["edge_lnl"][0]
    (counts_t, lnl_t), (ref_counts, ref_lnl) = run["edge_t"], run["ref_t"]
    assert _rel(counts_t, ref_counts).max() <= 1e-10
    assert abs(lnl_t - ref_lnl) <= 1e-10 * abs(ref_lnl)


def test_repeat_is_bitwise_and_state_unchanged(run):
    a, b = run["first"], run["second"]
    for k in ("edges", "lengths", "counts", "edge_lnl"):
        assert np.array_equal(a[k], b[k]), k
    b4, af = run["before"], run["after"]
    assert af["lnl"] == b4["lnl"]
    assert np.array_equal(af["site"], b4["site"])
    for x, y in zip(b4["parts"], af["parts"]):
        assert np.array_equal(x, y)


def test_pendant_root_edge_has_a_tip_end(run):
    if "pendant" not in run["case"]:
        return
    tm = run["tm"]
    nod, par = (int(v) for v in run["first"]["edges"][0])
    assert (nod in tm.names.values()) != (par in tm.names.values())


def test_zero_weight_patterns_add_nothing():
    """Weights 0 at patterns 0 and 64 (the one-lane tile): M is bitwise the M of the alignment
    with other tip codes in those two columns."""
    prob = _problem("dna-8x65-C3")
    prob["weights"] = prob["weights"].copy()
    prob["weights"][[0, 64]] = 0.0
    other = dict(prob, codes=prob["codes"].copy())
    other["codes"][:, [0, 64]] = (other["codes"][:, [0, 64]] + 1 +
                                  np.arange(len(other["codes"]))[:, None]) % 4
    a, b = _tm(prob).edge_counts(), _tm(other).edge_counts()
    assert np.array_equal(a["counts"], b["counts"])
    assert np.array_equal(a["edge_lnl"], b["edge_lnl"])
    assert np.isfinite(a["counts"]).all()


def test_branch_gradient(run, oracle_mod):
    tm, ref, prob, tr = run["tm"], run["ref"], run["prob"], run["tr"]
    got = gradient.branch_gradient(tm, run["first"])
    want = R.branch_gradient(oracle_mod, prob, ref)
    g = np.array([got[(int(a), int(b))] for a, b in ref["edges"]])
    scale = np.abs(want).max()
    worst = np.abs(g - want).max() / scale
    nod, par = (int(v) for v in ref["edges"][0])
    d1 = tm.edge_derivatives(nod, par)[1]
    print("%s: branch gradient worst error %.2e of max |g| = %.3g; root edge %.10g, "
          "edge_derivatives %.10g" % (run["case"], worst, scale, g[0], d1))
    assert worst <= 1e-9
    assert abs(g[0] - d1) <= 1e-9 * scale


def _model_vector(grads, names):
    return np.concatenate([np.atleast_1d(grads[n]) for n in names])


def _check_model_gradient(orc, prob, tr, ref, tm, res, names, label):
    got = _model_vector(gradient.model_gradient(tm, names, res), names)
    K = len(prob["model"].freqs)
    keys = []
    for n in names:
        keys += {"rates": [("rates", k) for k in range(5)],
                 "freqs": [("freqs", k) for k in range(K - 1)]}.get(n, [n])
    want = np.array([R.gradient(orc, prob, tr, ref, k) for k in keys])
    worst = np.abs(got - want).max() / np.abs(want).max()
    print("%s: model gradient %s worst error %.2e of max |g| = %.3g" % (
        label, names, worst, np.abs(want).max()))
    assert worst <= 1e-8


def test_model_gradient(run, oracle_mod):
    kind = R.CASES[run["case"]][0]
    if kind == "binary":
        return  # the two-state test model has no named parameters
    names = ["freqs"] + (["alpha"] if run["prob"]["rm"].ncat > 1 else [])
    if kind != "protein":
        names.append("rates")
    _check_model_gradient(oracle_mod, run["prob"], run["tr"], run["ref"], run["tm"],
                          run["first"], names, run["case"])


def test_model_gradient_kappa(oracle_mod):
    prob = _problem("dna-pendant-root-4x70-C4")
    prob["model"] = SM.HKY85(2.5, CFG2_FREQS)
    tr, e, tips, ref = R.restate(oracle_mod, prob)
    tm = _tm(prob)
    _check_model_gradient(oracle_mod, prob, tr, ref, tm, tm.edge_counts(),
                          ["kappa", "freqs", "alpha"], "HKY85 quartet")


def test_fit_recovers_a_simulated_model():
    """12 taxa x 2000 sites simulated under GTR+G4; the fit starts from JC-like values and
    alpha = 1.  The gradient bound: L-BFGS-B stops when an iteration gains less than lnl_tol,
    and near the optimum that gain is of the order of the remaining gap gap = g' H^-1 g / 2 >=
    |g|^2 / (2 lambda_max), so |g| <= sqrt(2 lambda_max lnl_tol).  lambda_max of -lnL in the log
    coordinates is at most the Fisher information of all the data, and an observed character
    carries at most one unit of it in a log-scale coordinate: lambda_max <= sites x taxa."""
    true_m, true_rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    tree = random_tree(np.random.default_rng(11), 12, lo=0.02, hi=0.3)
    sim = TreeModel(device=0)
    from phylo_utils_amd.tree import Traversal, prepare_tree
    names = sorted(Traversal(prepare_tree(tree)).names)
    sim.set_alignment_codes(np.zeros((12, 1), dtype=np.uint8), np.eye(4), names)
    sim.set_substitution_model(true_m)
    sim.set_rate_model(true_rm)
    sim.set_tree(tree)
    sim.initialise()
    states = sim.simulate(2000, seed=7)  # [taxon][site], rows in `names` order

    def model(m, rm):
        tm = TreeModel(device=0)
        tm.set_alignment_codes(np.asarray(states, dtype=np.uint8), np.eye(4), names)
        tm.set_substitution_model(m)
        tm.set_rate_model(rm)
        tm.set_tree(tree)
        tm.initialise()
        return tm

    at_truth = model(true_m, true_rm)
    at_truth.optimise_branch_lengths(sweeps=3)
    lnl_truth = at_truth.likelihood()
    tm = model(SM.GTR([1.0] * 6, [0.25] * 4), GammaRateModel(4, 1.0))
    lnl_start = tm.likelihood()
    lnl_tol = 1e-6
    fit = tm.optimise_model(("alpha", "rates", "freqs"), branch_lengths=True, lnl_tol=lnl_tol)
    g = modelfit.coordinate_gradient(tm, fit)
    p = fit["params"]
    print("fit: lnL %.6f -> %.6f (truth with optimised lengths %.6f), %d iterations, %d "
          "gradients, |g| = %.3e" % (lnl_start, fit["lnl"], lnl_truth, fit["n_iter"],
                                     fit["n_gradients"], np.linalg.norm(g)))
    print("  alpha %.4f (true 0.5)\n  rates %s (true %s)\n  freqs %s (true %s)" % (
        p["alpha"], np.round(p["rates"], 4), CFG2_GTR_RATES[:5], np.round(p["freqs"], 4),
        CFG2_FREQS))
    assert fit["converged"]
    assert fit["lnl"] >= lnl_truth
    assert tm.likelihood() == fit["lnl"]
    assert np.linalg.norm(g) <= np.sqrt(2.0 * 2000 * 12 * lnl_tol)
    assert isinstance(tm.substitution_model, SM.GTR) and tm.rate_model.alpha == p["alpha"]


def test_refusals():
    lib = N.lib()

    def sweep_rc(tm):
        rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
        K, C, n = tm.alignment.shape[2], tm.rate_model.ncat, 2 * len(tm.names) - 3
        edges, lens = np.zeros((n, 2), dtype=np.int32), np.zeros(n)
        counts, lnl, cnt = np.zeros((n, C, K, K)), np.zeros(n), ctypes.c_int()
        return lib.pu_counts_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(edges), N.ptr(lens),
                                   N.ptr(counts), N.ptr(lnl), ctypes.byref(cnt))

    assert lib.pu_counts_max_cat(3) == N.PU_E_ARG
    kmax = lib.pu_counts_max_cat(20)
    assert 4 <= kmax < 64
    m, rm = SM.LG(), GammaRateModel(kmax + 1, 0.8)
    tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
    prob = dict(tree=tree, names=names, codes=st.astype(np.uint8), table=np.eye(20), model=m,
                rm=rm, compact=True, weights=np.ones(70))
    tm = _tm(prob)
    lnl0 = tm.likelihood()
    assert sweep_rc(tm) == N.PU_E_ARG
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
        tm.edge_counts()
    assert tm.likelihood() == lnl0
    prob = _problem("dna-8x65-C3")
    tm = _tm(prob, keep=False)
    assert sweep_rc(tm) == N.PU_E_STATE
    with pytest.raises(ValueError, match="keep_partials"):
        tm.edge_counts()
    tm = _tm(prob)
    left, right = (int(v) for v in tm.traversal.root_edge)
    K, C = 4, prob["rm"].ncat
    out, lnl = np.zeros((C, K, K)), ctypes.c_double()
    edge = lambda *a: lib.pu_edge_counts(tm._ctx, *a)
    assert edge(left, right, -1.0, N.ptr(out), ctypes.byref(lnl)) == 0
    for bad in (0.0, float("nan"), float("inf")):
        assert edge(left, right, bad, N.ptr(out), ctypes.byref(lnl)) == N.PU_E_ARG
    assert edge(left, 10 ** 6, -1.0, N.ptr(out), ctypes.byref(lnl)) == N.PU_E_ARG
    assert edge(left, right, -1.0, None, ctypes.byref(lnl)) == N.PU_E_ARG
    with pytest.raises(ValueError, match="valid: rates, freqs, alpha"):
        tm.optimise_model(("kappa",))
    tm.set_ascertainment_bias_correction()
    tm.initialise()
    assert sweep_rc(tm) == N.PU_E_STATE
    with pytest.raises(ValueError, match="ascertainment"):
        tm.edge_counts()
    tm = _tm(dict(prob, model=SM.Strsym(), rm=UniformRateModel()))
    assert sweep_rc(tm) == N.PU_E_STATE
    with pytest.raises(ValueError, match="reversible"):
        tm.edge_counts()


def test_cli_fit_end_to_end(tmp_path, capsys):
    from test_cli import _write_case

    from phylo_utils_amd import phy
    nw, fa, _, _ = _write_case(tmp_path)
    spec = "HKY85+G4"
    lnl_of = lambda text: float(text.strip().splitlines()[-1].split("=")[1])
    assert phy.main(["-t", nw, "-s", fa, "-m", spec]) == 0
    plain = capsys.readouterr().out
    assert plain.count("\n") == 1 and plain.startswith("lnL = ")
    out_tree = str(tmp_path / "fit.nwk")
    assert phy.main(["-t", nw, "-s", fa, "-m", spec, "--fit", "-o", out_tree]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("model = HKY85{") and "+G4{" in lines[0]
    lnl_fit = lnl_of(lines[1])
    assert lnl_fit >= lnl_of(plain)
    assert phy.main(["-t", out_tree, "-s", fa, "-m", lines[0][len("model = "):]]) == 0
    back = lnl_of(capsys.readouterr().out)
    assert abs(back - lnl_fit) <= 1e-8 * abs(lnl_fit)
    assert phy.main(["-t", nw, "-s", fa, "-m", spec]) == 0
    assert capsys.readouterr().out == plain
    print("phy --fit: lnL %.6f -> %.6f, read back %.6f, %s" % (lnl_of(plain), lnl_fit, back,
                                                                lines[0]))


def test_an_error_in_mid_walk_puts_the_context_back():
    """pu_counts_sweep on rows whose last edge names a PAR that is not NOD's neighbour
    (walk_errors.py): PU_E_ARG, and the lnL, sitewise lnL and partials are pu_run's again."""
    prob = _problem("dna-8x65-C3")
    tm = _tm(prob)
    tm.likelihood()
    bad = W.rows_with_a_bad_last_edge(tm)
    before = W.snapshot(tm)
    n, C, K = 2 * len(tm.names) - 3, prob["rm"].ncat, 4
    edges, lens, counts, lnl, cnt = (np.zeros((n, 2), dtype=np.int32), np.zeros(n),
                                     np.zeros((n, C, K, K)), np.zeros(n), ctypes.c_int())
    rc = N.lib().pu_counts_sweep(tm._ctx, len(bad), N.ptr(bad), N.ptr(edges), N.ptr(lens),
                                 N.ptr(counts), N.ptr(lnl), ctypes.byref(cnt))
    W.assert_refused_and_put_back(tm, before, rc)
