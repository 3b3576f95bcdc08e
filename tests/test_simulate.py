"""The simulator's specification on the CPU (tests/sim_reference.py): known
answers of the generator and the choice rule, the distribution the walk produces against the
oracle's pattern probabilities, the binding, and the refusals that need no device."""
import ctypes
import itertools

import numpy as np
import pytest
import scipy.stats

from conftest import has_gpu

import sim_reference as R
from phylo_utils_amd import _native as N
from phylo_utils_amd import phy, simulation
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
from phylo_utils_amd.tree import Traversal, prepare_tree

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = " ".join("%08x" % int(x[0]) for x in R.philox4x32_10(counter, key))
    assert got == want


def test_uniform_is_53_bits_in_unit_interval():
    g = np.concatenate([np.arange(4096), 2 ** 32 - 5 + np.arange(10), [2 ** 63 - 1]])
    for seed, d in ((0, 0), (1, 1), (2 ** 64 - 1, 7), (12345678901234567, 2 ** 32 - 1)):
        u = R.uniform(seed, g, d)
        assert u.dtype == np.float64 and np.all(u >= 0.0) and np.all(u < 1.0)
        assert np.all(u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))
    # the counter's words: (g lo, g hi, d, 0) and the key (seed lo, seed hi)
    x = R.philox4x32_10((5, 1, 9, 0), (3, 4))
    u = R.uniform((4 << 32) | 3, np.uint64((1 << 32) | 5), 9)
    m = ((int(x[1][0]) >> 5) << 26) | (int(x[0][0]) >> 6)
    assert u[0] == m * 2.0 ** -53
    # all-ones output words give the largest u, still below 1
    assert ((0xFFFFFFFF >> 5) * 2.0 ** 26 + (0xFFFFFFFF >> 6)) * 2.0 ** -53 < 1.0


def test_pick_on_hand_made_rows():
    assert R.pick([0.25, 0.25, 0.25, 0.25], 0.0) == 0
    assert R.pick([0.25, 0.25, 0.25, 0.25], 0.25) == 1  # cum_0 > r is strict
    assert R.pick([0.25, 0.25, 0.25, 0.25], 0.999) == 3
    # a zero-weight first entry is never chosen, not even at u = 0
    assert R.pick([0.0, 1.0, 1.0], 0.0) == 1
    assert R.pick([0.0, 0.5, 0.0, 0.5], 0.5) == 3  # zero weight in the middle is skipped
    # the fallback: no cum_j > r (all weights zero) -> n - 1 (the reference returns 0 here)
    assert R.pick([0.0, 0.0, 0.0], 0.3) == 2
    # unnormalised weights: r = u * total
    assert R.pick([1.0, 3.0], 0.2) == 0 and R.pick([1.0, 3.0], 0.25) == 1
    # sums are taken in index order: 0.1 + 0.2 + 0.3 as fp64 adds
    w = [0.1, 0.2, 0.3]
    cum = R.cumulate(w)
    assert cum[1] == 0.1 + 0.2 and cum[2] == (0.1 + 0.2) + 0.3
    np.testing.assert_array_equal(R.pick([0.25] * 4, np.array([0.0, 0.25, 0.5, 0.99])),
                                  [0, 1, 2, 3])


# ---------------------------------------------------------------------------- distribution
NEWICK4 = "((a:0.4,b:0.7):0.3,(c:0.5,d:0.9):0.2);"
N_DIST = 2 ** 18
# seed 1 (the first one tried): chi2 statistics 265.03 (patterns, 255 d.o.f.), 5.83
# (categories, 3) and 2.47 (root state, 3), all below isf(1e-3) = 330.5 / 16.3 / 16.3, so the
# tests at the 1e-6 tail (377.1 / 30.7) do not sit on their edge
SEED_DIST = 1


@pytest.fixture(scope="module")
def dist_case():
    model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    rm = GammaRateModel(4, 0.5)
    tr = Traversal(prepare_tree(NEWICK4))
    rates, weights = np.asarray(rm.rates, float), np.asarray(rm.weights, float)
    a, b = tr.root_edge
    cum = R.cum_rows(model, rates, tr.postorder_traversal, tr.op_lengths(), a, b,
                     tr.root_length(), tr.n_nodes)
    cats, nodes = R.walk(tr.postorder_traversal, a, b, cum, weights, model.freqs, SEED_DIST, 0,
                         N_DIST)
    return dict(model=model, rates=rates, weights=weights, tr=tr, cats=cats, nodes=nodes)


def chi2(observed, expected):
    return float(((observed - expected) ** 2 / expected).sum())


def test_site_patterns_follow_the_oracle(dist_case, oracle_mod):
    """2^18 simulated sites on 4 taxa under GTR+G4 (the cfg2 parameters): the 256 site-pattern
    counts against n * exp(site lnL) of the oracle, Pearson chi-square below the 1e-6 tail."""
    c = dist_case
    tr, model = c["tr"], c["model"]
    tip_nodes = sorted(tr.names.values())
    pats = np.array(list(itertools.product(range(4), repeat=4)))  # [256][4]
    eye = np.eye(4)
    tips = {v: eye[pats[:, i]] for i, v in enumerate(tip_nodes)}
    ev, el, iv = model.engine_eigen()
    _, site = oracle_mod.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                  tr.root_length(), ev, el, iv, model.freqs, c["rates"],
                                  c["weights"], n_nodes=tr.n_nodes)
    prob = np.exp(site)
    assert abs(prob.sum() - 1.0) < 1e-12
    expected = N_DIST * prob
    assert expected.min() > 5.0  # the chi-square approximation holds in every cell
    key = np.zeros(N_DIST, dtype=np.int64)
    for v in tip_nodes:
        key = key * 4 + c["nodes"][v]
    observed = np.bincount(key, minlength=256)
    stat = chi2(observed, expected)
    print("pattern chi2 = %.3f" % stat)
    assert stat < scipy.stats.chi2.isf(1e-6, 255)


def test_categories_and_root_state_follow_their_weights(dist_case):
    c = dist_case
    w = c["weights"] / c["weights"].sum()
    stat_c = chi2(np.bincount(c["cats"], minlength=4), N_DIST * w)
    f = np.asarray(c["model"].freqs, float)
    stat_r = chi2(np.bincount(c["nodes"][c["tr"].root_edge[0]], minlength=4),
                  N_DIST * f / f.sum())
    print("category chi2 = %.3f, root state chi2 = %.3f" % (stat_c, stat_r))
    assert stat_c < scipy.stats.chi2.isf(1e-6, 3)
    assert stat_r < scipy.stats.chi2.isf(1e-6, 3)


def test_walk_column_depends_only_on_its_global_site(dist_case):
    """The restatement itself: [0, 1000) equals [0, 300) and [300, 1000) joined."""
    c = dist_case
    tr = c["tr"]
    a, b = tr.root_edge
    cum = R.cum_rows(c["model"], c["rates"], tr.postorder_traversal, tr.op_lengths(), a, b,
                     tr.root_length(), tr.n_nodes)
    args = (tr.postorder_traversal, a, b, cum, c["weights"], c["model"].freqs, 7)
    _, whole = R.walk(*args, 0, 1000)
    _, lo = R.walk(*args, 0, 300)
    _, hi = R.walk(*args, 300, 700)
    np.testing.assert_array_equal(whole, np.hstack([lo, hi]))


# ---------------------------------------------------------------------------- binding
def test_symbols_are_exported_and_bound():
    lib = N.lib()
    for name in ("pu_evolve_states", "pu_simulate", "pu_simulate_device"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert callable(simulation.evolve_states) and callable(simulation.simulate_alignment)
    from phylo_utils_amd import TreeModel
    assert callable(TreeModel.simulate)


def test_states_to_sequences():
    assert simulation.states_to_sequences([[0, 1, 2, 3], [3, 3, 0, 0]], "dna") == ["ACGT", "TTAA"]
    assert simulation.states_to_sequences(np.array([[0, 19]], dtype=np.uint8),
                                          "protein") == ["AV"]
    with pytest.raises(ValueError):
        simulation.states_to_sequences([[4]], "dna")


# ---------------------------------------------------------------------------- refusals
def test_argument_refusals_need_no_device():
    lib = N.lib()
    p = np.full((1, 4, 4), 0.25)
    par = np.zeros(8, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint8)
    args = lambda **kw: [kw.get("device", 0), kw.get("K", 4), kw.get("C", 1), kw.get("n", 8), 1,
                         kw.get("first", 0), 0, kw.get("probs", N.ptr(p)),
                         kw.get("par", N.ptr(par)), None, kw.get("out", N.ptr(out))]
    assert lib.pu_evolve_states(*args(n=0)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(n=-3)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(first=-1)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(probs=None)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(par=None)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(out=None)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(K=0)) == N.PU_E_ARG
    assert lib.pu_evolve_states(*args(C=2)) == N.PU_E_ARG  # two classes need rate_class
    par[3] = 4  # a parent state outside [0, K)
    assert lib.pu_evolve_states(*args()) == N.PU_E_ARG
    assert "site 3" in N.last_error()
    # no context: refused before anything else
    assert lib.pu_simulate(None, 0, 0, 10, N.ptr(out), None, None, None) == N.PU_E_ARG
    assert lib.pu_simulate_device(None, 0, 0, 10, N.ptr(out), 10, None, None, 0) == N.PU_E_ARG
    with pytest.raises(ValueError):
        simulation.evolve_states(par, None, np.zeros((4, 4)), 0)
    with pytest.raises(ValueError):
        simulation.evolve_states(par, None, p, 0, layout="xyz")


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_no_device_fails_loudly():
    p = np.full((1, 4, 4), 0.25)
    with pytest.raises(N.PhyloHipError):
        simulation.evolve_states(np.zeros(8, dtype=np.uint8), None, p, seed=1)
    with pytest.raises(N.PhyloHipError):
        simulation.simulate_alignment(NEWICK4, SM.GTR(CFG2_GTR_RATES, CFG2_FREQS),
                                      GammaRateModel(4, 0.5), 10)


def test_cli_simulate_needs_a_tree(tmp_path):
    assert phy.main(["--simulate", "10"]) == 1
    assert phy.main(["-t", str(tmp_path / "missing.nwk"), "--simulate", "10"]) == 1
    t = tmp_path / "t.nwk"
    t.write_text(NEWICK4)
    assert phy.main(["-t", str(t), "--simulate", "0"]) == 1
    assert phy.main(["-s", "x.fa"]) == 1  # as before
