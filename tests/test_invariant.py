"""The +I yardstick (tests/invariant_reference.py) on the CPU: that its cases can tell a kernel
that mishandles the invariable category from one that does not, that the oracle's own +I lnL
sits orders below the device tolerance from it, and that it is the product formula and the
enumeration.  Needs no device."""
import numpy as np
import pytest

import ancestral_reference as AR
import invariant_reference as IR
import place_reference as PR
import spr_reference as SR


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def case(request, oracle_mod):
    prob = IR.problem(request.param)
    tr, e, tips = IR.setting(prob)
    x = IR.Exact(oracle_mod)
    return dict(name=request.param, prob=prob, tr=tr, e=e, tips=tips, x=x,
                st=IR.state(x, tips, tr, e, prob["weights"]),
                inv=IR.invariant_site_likelihood(tips, tr, e["freqs"]))


def test_constant_and_variable_patterns(case):
    """(a): at least 5 constant and 5 variable patterns of non-zero weight, weights 0..3 with
    zeros, and an ambiguity code and a gap in a constant and in a variable column."""
    w, const = case["prob"]["weights"], case["inv"] > 0
    assert ((w > 0) & const).sum() >= 5 and ((w > 0) & ~const).sum() >= 5
    assert set(np.unique(w)) == {0.0, 1.0, 2.0, 3.0}
    table, codes = case["prob"]["table"], case["prob"]["codes"]
    wide = table[codes].sum(axis=2) > 1           # [taxon][S]: an ambiguity or gap code
    full = table[codes].sum(axis=2) == table.shape[1]
    # only the DNA table has codes between one state and all of them
    has_narrow = ((table.sum(axis=1) > 1) & (table.sum(axis=1) < table.shape[1])).any()
    assert has_narrow == (table.shape[1] == 4)
    for cols in (const, ~const):
        assert (wide & ~full)[:, cols & (w > 0)].any() or not has_narrow
        assert full[:, cols & (w > 0)].any()


def test_dropping_the_invariable_category_moves_the_lnl(case, oracle_mod):
    """(b): by more than 1e-3 relative."""
    e2 = IR.without_category_0(case["e"])
    lnl = case["st"]["lnl"]
    lnl2 = IR.state(oracle_mod, case["tips"], case["tr"], e2, case["prob"]["weights"])["lnl"]
    print("%s: lnL %.6f, without category 0 %.6f" % (case["name"], lnl, lnl2))
    assert abs(lnl2 - lnl) > 1e-3 * abs(lnl)


def test_the_oracles_noise_takes_both_signs(case, oracle_mod):
    """(c): in the oracle's own partials, on some edge of the walk, F_0 < 0 at one variable
    pattern and F_0 > 0 at another -- the masked branch of the mix is taken and not taken.
    Measured on the root edge (F_0 < 0, F_0 > 0, of variable patterns): dna-8x65-I 27, 18 of 45;
    dna-8x65-IG3 14, 15 of 29; dna-coded-14x700-I 244, 257 of 501; dna-coded-14x700-IG3 228, 194
    of 422; protein-8x97-IG3 30, 19 of 49; dna-caterpillar-150x130-IG3 51, 55 of 106.
    The two-state model cannot show a negative F_0: every entry of its U U^-1 is >= 0 (the
    rounding leaves +4e-17 and +2e-17 off the diagonal), so products and sums of its entries are
    too.  There the other half is asserted alone: F_0 > 0 at variable patterns, where the truth
    is 0 -- the noise category takes a weight (binary-8x70-IG3: 32 of 32)."""
    ref = PR.Restated(oracle_mod, case["prob"])
    e, var = case["e"], ~(case["inv"] > 0)
    best = None
    for k, (A_, sA, B_, sB) in enumerate(ref.ends):
        P0 = ref.pm(ref.lengths[k])[0]
        F0 = np.einsum("i,si,ij,sj->s", e["freqs"], A_[:, 0], P0, B_[:, 0])[var]
        if (F0 > 0).any() and ((F0 < 0).any() or len(e["freqs"]) == 2):
            best = (k, int((F0 < 0).sum()), int((F0 > 0).sum()), int(var.sum()))
            break
    print("%s: edge number, F_0 < 0, F_0 > 0, variable patterns: %s" % (case["name"], best))
    assert best is not None
    if len(e["freqs"]) == 2:
        assert (ref.pm(0.3)[0] >= 0).all()


def test_the_oracle_agrees_with_the_yardstick(case, oracle_mod):
    """(d): the oracle's tree_lnl under +I against the exact yardstick, 1e-12 relative in the lnL
    and per site -- two orders below the 1e-10 the device tests allow.  Measured worst relative
    difference (lnL; per site): binary-8x70-IG3 0 and 8.2e-16, dna-8x65-I 3.2e-16 and 7.1e-15,
    dna-8x65-IG3 1.9e-16 and 3.4e-15, dna-coded-14x700-I 3.8e-16 and 3.7e-14, dna-coded-14x700-IG3
    6.1e-16 and 2.2e-14, protein-8x97-IG3 2.9e-15 and 1.3e-13, dna-caterpillar-150x130-IG3 5.2e-16
    and 1.4e-13."""
    st = IR.state(oracle_mod, case["tips"], case["tr"], case["e"], case["prob"]["weights"])
    ex = case["st"]
    d_lnl = abs(st["lnl"] - ex["lnl"]) / abs(ex["lnl"])
    d_site = (np.abs(st["site_lnl"] - ex["site_lnl"]) / np.abs(ex["site_lnl"])).max()
    print("%s: oracle vs yardstick, lnL %.2e, per site %.2e" % (case["name"], d_lnl, d_site))
    assert d_lnl <= 1e-12 and d_site <= 1e-12


def test_category_0_is_the_product_formula(case):
    """Exact's category 0 is the closed form bit for bit with every scaler 0, on the post-order
    partials and (8 x 65) on every directed vector of the tree."""
    cf = IR.closed_form(case["tips"], case["tr"])
    P, S = case["st"]["partials"], case["st"]["scale"]
    for n, v in cf.items():
        assert np.array_equal(P[n][:, 0, :], v)
    assert not S[:, :, 0].any()
    assert np.array_equal(case["st"]["site_lnl"] > -np.inf, np.ones(len(case["inv"]), bool))
    if "8x65" not in case["name"]:
        return
    ref = SR.Restated(case["x"], case["prob"])
    memo = {}
    for a in ref.adj:
        for b in ref.adj[a]:
            v, s = ref.directed(ref.adj, a, b, memo)
            side, todo = {a}, [a]
            while todo:
                for z in ref.adj[todo.pop()]:
                    if z != b and z not in side:
                        side.add(z)
                        todo.append(z)
            want = np.prod([case["tips"][t] for t in side if t in case["tips"]], axis=0)
            assert np.array_equal(v[:, 0, :], want) and not s[:, 0].any()


def test_quartet_against_enumeration(oracle_mod):
    """(e): on four taxa the yardstick's posteriors, category posteriors and per-pattern lnL are
    ancestral_reference.brute_force's with the exact identity for category 0."""
    prob = IR.problem(IR.QUARTET)
    tr, e, tips = IR.setting(prob)
    x = IR.Exact(oracle_mod)
    ref = AR.sweep(x, tips, tr, e, site_weights=prob["weights"])
    bf = AR.brute_force(x, tips, tr, e)
    inv = IR.invariant_site_likelihood(tips, tr, e["freqs"])
    assert (inv > 0).sum() >= 5 and (inv == 0).sum() >= 5
    for n, q in zip(ref["nodes"], ref["posteriors"]):
        assert np.abs(q - bf["posteriors"][int(n)]).max() <= 1e-13
    assert np.abs(ref["cat_post"] - bf["cat_post"]).max() <= 1e-13
    assert (ref["cat_post"][inv == 0, 0] == 0).all()
    assert (ref["cat_post"][inv > 0, 0] > 0.01).all()
    st = IR.state(x, tips, tr, e, prob["weights"])
    assert np.abs(st["site_lnl"] - bf["lnl"]).max() <= 1e-13 * np.abs(bf["lnl"]).max()


def test_fit_surface_has_an_interior_maximum(oracle_mod):
    """The data of the device's pinvar / alpha fit (invariant_reference.fit_problem): the
    oracle's lnL, maximised over (pinvar, alpha) by Nelder-Mead in the fit's coordinates, peaks
    at a pinvar well inside (0, 1) and above the lnL at the generating values, and the best
    alpha at pinvar = 1e-6 stays below it by more than the fit's tolerance.  Measured:
    maximum -3917.083347 at pinvar 0.1834, alpha 0.4737; -3917.102745 at (0.2, 0.5);
    -3918.783441 at pinvar 1e-6 (alpha 0.3277)."""
    from scipy.optimize import minimize

    from phylo_utils_amd.rate_models import InvariantGammaModel
    prob = IR.fit_problem()
    tr, e, tips = IR.setting(prob)

    def lnl(p, a):
        rm = InvariantGammaModel(p, 3, a)
        return IR.state(oracle_mod, tips, tr, IR.eigen(prob["model"], rm))["lnl"]

    both = minimize(lambda z: -lnl(1 / (1 + np.exp(-z[0])), np.exp(z[1])), [np.log(0.05 / 0.95),
                    0.0], method="Nelder-Mead", options=dict(xatol=1e-6, fatol=1e-9))
    p, a = 1 / (1 + np.exp(-both.x[0])), np.exp(both.x[1])
    edge = minimize(lambda z: -lnl(1e-6, np.exp(z[0])), [0.0], method="Nelder-Mead",
                    options=dict(xatol=1e-6, fatol=1e-9))
    print("fit surface: maximum %.6f at pinvar %.4f, alpha %.4f; at the generating values %.6f; "
          "at pinvar 1e-6 %.6f (alpha %.4f)" % (-both.fun, p, a, lnl(0.2, 0.5), -edge.fun,
                                               np.exp(edge.x[0])))
    assert 0.02 < p < 0.9 and 0.05 < a < 50
    assert -both.fun >= lnl(0.2, 0.5)
    assert -both.fun - -edge.fun > 0.1
