"""The device simulator (pu_simulate.hip) against the numpy restatement of its specification
(tests/sim_reference.py): bit-equal states from the device's own cumulative rows,
those rows against the host P, invariance to everything a draw's address leaves out, the
single-branch seam, the untouched context, host matrices, and the round trip through the
likelihood."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden

import sim_reference as R
from twostate import TwoState
from phylo_utils_amd import TreeModel, _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import phy, simulation
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, random_tree
from phylo_utils_amd.tree import Traversal, prepare_tree

pytestmark = pytest.mark.gpu

NEWICK3 = "(a:0.1,b:0.2,c:0.3);"
NEWICK4 = "((a:0.1,b:0.2):0.05,(c:0.15,d:0.3):0.07);"


def gtr_g4():
    return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)


def _tree(n, seed):
    return random_tree(np.random.default_rng(seed), n)


CASES = {
    "gtr3": lambda: (NEWICK3,) + gtr_g4(),
    "gtr4": lambda: (NEWICK4,) + gtr_g4(),
    "gtr17": lambda: (_tree(17, 17),) + gtr_g4(),
    "gtr50": lambda: (_tree(50, 50),) + gtr_g4(),
    "lg8": lambda: (_tree(8, 8), SM.LG(), GammaRateModel(4, 0.8)),
    "jc5": lambda: (_tree(5, 5), SM.JC69(), UniformRateModel()),
    "two6": lambda: (_tree(6, 6), TwoState(0.3), GammaRateModel(4, 0.5)),
}


def dummy_model(tree, model, rm, **kw):
    """A TreeModel on one dummy coded pattern (every tip fully ambiguous)."""
    tm = TreeModel(**kw)
    tm.set_tree(tree)
    names = list(tm.traversal.names)
    K = len(model.freqs)
    tm.set_alignment_codes(np.zeros((len(names), 1), dtype=np.uint8), np.ones((1, K)), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.initialise()
    return tm


@functools.lru_cache(maxsize=None)
def case(name):
    tree, model, rm = CASES[name]()
    return dummy_model(tree, model, rm), model, rm


def restate(tm, model, rm, cum, seed, first_site, n_sites):
    tr = tm.traversal
    a, b = tr.root_edge
    return R.walk(tr.postorder_traversal, a, b, cum, np.asarray(rm.weights, float), model.freqs,
                  seed, first_site, n_sites)


def check_against_restatement(tm, model, rm, seed, first_site, n_sites):
    states, cats, nodes, cum = tm.simulate(n_sites, seed=seed, first_site=first_site,
                                           return_categories=True, return_ancestral=True,
                                           return_cum=True)
    ref_cats, ref_nodes = restate(tm, model, rm, cum, seed, first_site, n_sites)
    np.testing.assert_array_equal(cats, ref_cats)
    np.testing.assert_array_equal(nodes, ref_nodes)
    tr = tm.traversal
    assert states.shape == (len(tr.names), n_sites) and states.dtype == np.uint8
    for name, node in tr.names.items():
        np.testing.assert_array_equal(states[tm.names[name]], ref_nodes[node], err_msg=name)
    # without the optional outputs (the node-state workspace path): the same tips
    np.testing.assert_array_equal(tm.simulate(n_sites, seed=seed, first_site=first_site), states)
    return cum


@pytest.mark.parametrize("n_sites", [1, 65, 1000])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_equal_to_the_restatement(name, n_sites):
    tm, model, rm = case(name)
    check_against_restatement(tm, model, rm, 11 + n_sites, 0, n_sites)


@pytest.mark.parametrize("name", ["gtr17", "lg8"])
def test_counter_high_word(name):
    tm, model, rm = case(name)
    check_against_restatement(tm, model, rm, 2 ** 63 + 5, 2 ** 32 - 10, 20)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cumulative_rows_match_host_p(name):
    """cum_out against the running sums of host Model.p at the schedule's lengths: rtol 1e-12
    (the tolerance of the engine's P against Model.p, test_gpu_parity.py:296) and that test's
    atol of 1e-15 per entry, summed over a row of K entries."""
    tm, model, rm = case(name)
    tr = tm.traversal
    K = len(model.freqs)
    cum = tm.simulate(1, return_cum=True)[1]
    a, b = tr.root_edge
    ref = R.cum_rows(model, np.asarray(rm.rates, float), tr.postorder_traversal, tr.op_lengths(),
                     a, b, tr.root_length(), tr.n_nodes)
    assert cum.shape == ref.shape == (tr.n_nodes, rm.ncat, K, K)
    np.testing.assert_allclose(cum, ref, rtol=1e-12, atol=K * 1e-15)
    assert np.all(cum[a] == 0.0)
    np.testing.assert_allclose(cum[np.arange(tr.n_nodes) != a][..., -1], 1.0, rtol=1e-12)


# ---------------------------------------------------------------------------- invariance
def raw_simulate(tr, model, rm, ops, bl, flags, seed, first_site, n_sites):
    """pu_simulate on a context built by hand over `ops` (any valid post-order of tr's tree):
    (tips in tr.names order, cats, nodes)."""
    lib = N.lib()
    K, C = len(model.freqs), rm.ncat
    ctx = ctypes.c_void_p()
    N.check(lib.pu_ctx_create(ctypes.byref(ctx), 0, tr.n_nodes, len(tr.names), 1, C, K, flags))
    try:
        table = np.ones((1, K))
        N.check(lib.pu_set_code_table(ctx, 1, N.ptr(table)), ctx)
        code = np.zeros(1, dtype=np.uint8)
        for node in tr.names.values():
            N.check(lib.pu_set_tip_codes(ctx, int(node), N.ptr(code)), ctx)
        ev, el, iv = model.engine_eigen()
        N.check(lib.pu_set_model(ctx, N.ptr(ev), N.ptr(el), N.ptr(iv), N.ptr(N.f64(model.freqs)),
                                 N.ptr(N.f64(rm.rates)), N.ptr(N.f64(rm.weights))), ctx)
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        bl = N.f64(bl)
        a, b = tr.root_edge
        N.check(lib.pu_set_schedule(ctx, len(ops), N.ptr(ops), N.ptr(bl), a, b,
                                    tr.root_length()), ctx)
        res = simulation.simulate_on_context(ctx, len(tr.names), tr.n_nodes, C, K, n_sites, seed,
                                             first_site, True, True)
        return res["tips"], res["cats"], res["nodes"]
    finally:
        lib.pu_ctx_destroy(ctx)


def other_postorder(tr):
    """Another valid post-order of the same tree: depth first from the root edge with the
    second child first, and the two children of every op exchanged (with their lengths)."""
    ops = {int(p): (int(c1), int(c2)) for p, c1, c2 in tr.postorder_traversal}
    order, stack = [], [(v, False) for v in tr.root_edge]
    while stack:
        v, done = stack.pop()
        if v not in ops:
            continue
        if done:
            order.append(v)
        else:
            stack.append((v, True))
            stack.extend((c, False) for c in ops[v])  # popped in the other order
    rows = [(p, ops[p][1], ops[p][0]) for p in order]
    bl = [[tr.brlens[(p, x)], tr.brlens[(p, y)]] for p, x, y in rows]
    return np.array(rows, dtype=np.int32), np.array(bl)


def test_invariant_to_planner_order_and_op_order():
    model, rm = gtr_g4()
    tr = Traversal(prepare_tree(_tree(17, 17)))
    ops, bl = tr.postorder_traversal, tr.op_lengths()
    ops2, bl2 = other_postorder(tr)
    assert sorted(map(tuple, ops2[:, :1])) == sorted(map(tuple, ops[:, :1]))
    assert not np.array_equal(ops, ops2)
    base = raw_simulate(tr, model, rm, ops, bl, 0, 3, 0, 500)
    for o, l, flags in ((ops, bl, N.PU_NO_REORDER), (ops2, bl2, 0), (ops2, bl2, N.PU_NO_REORDER),
                        (ops, bl, N.PU_LNL_ONLY)):
        got = raw_simulate(tr, model, rm, o, l, flags, 3, 0, 500)
        for x, y in zip(base, got):
            np.testing.assert_array_equal(x, y)
    # and TreeModel's reorder switch
    t1 = dummy_model(_tree(17, 17), model, rm, reorder=True).simulate(500, seed=3)
    t2 = dummy_model(_tree(17, 17), model, rm, reorder=False).simulate(500, seed=3)
    np.testing.assert_array_equal(t1, t2)


@pytest.mark.parametrize("name", ["gtr17", "lg8"])
def test_site_ranges_join(name):
    tm, _, _ = case(name)
    kw = dict(seed=9, return_categories=True, return_ancestral=True)
    whole = tm.simulate(1000, first_site=0, **kw)
    lo = tm.simulate(300, first_site=0, **kw)
    hi = tm.simulate(700, first_site=300, **kw)
    for w, x, y in zip(whole, lo, hi):
        np.testing.assert_array_equal(w, np.concatenate([x, y], axis=-1))


@pytest.mark.parametrize("name", ["gtr17", "lg8"])
def test_chunking_does_not_change_the_result(name, monkeypatch):
    tm, _, _ = case(name)
    base = tm.simulate(1000, seed=4)
    base_all = tm.simulate(1000, seed=4, return_categories=True, return_ancestral=True)
    monkeypatch.setenv("PU_SIM_CHUNK", "128")  # 8 launches, the last one of 104 sites
    np.testing.assert_array_equal(tm.simulate(1000, seed=4), base)
    got = tm.simulate(1000, seed=4, return_categories=True, return_ancestral=True)
    for x, y in zip(base_all, got):
        np.testing.assert_array_equal(x, y)
    monkeypatch.setenv("PU_SIM_CHUNK", "1")  # every site its own launch
    np.testing.assert_array_equal(tm.simulate(70, seed=4), base[:, :70])


def test_device_buffers_with_a_row_stride():
    torch = pytest.importorskip("torch")
    tm, _, _ = case("gtr17")
    n_nodes, n_tips = tm._ctx_shape[:2]
    S, ld = 1000, 1024
    _, cats, nodes = tm.simulate(S, seed=6, return_categories=True, return_ancestral=True)
    res = simulation.simulate_on_context(tm._ctx, n_tips, n_nodes, *tm._ctx_shape[3:], S, 6)
    dev = torch.device("cuda", 0)
    N.check(N.lib().pu_ctx_set_stream(tm._ctx, ctypes.c_void_p(
        torch.cuda.current_stream(dev).cuda_stream)), tm._ctx)
    try:
        for with_nodes in (False, True):
            d_t = torch.full((n_tips, ld), 255, dtype=torch.uint8, device=dev)
            d_c = torch.full((S,), 255, dtype=torch.uint8, device=dev)
            d_n = torch.full((n_nodes, ld), 255, dtype=torch.uint8, device=dev)
            N.check(N.lib().pu_simulate_device(
                tm._ctx, 6, 0, S, ctypes.c_void_p(d_t.data_ptr()), ld,
                ctypes.c_void_p(d_c.data_ptr()),
                ctypes.c_void_p(d_n.data_ptr()) if with_nodes else None, ld), tm._ctx)
            torch.cuda.synchronize(dev)
            t = d_t.cpu().numpy()
            np.testing.assert_array_equal(t[:, :S], res["tips"])
            assert np.all(t[:, S:] == 255)  # the padding of every row is left alone
            np.testing.assert_array_equal(d_c.cpu().numpy(), cats)
            n = d_n.cpu().numpy()
            if with_nodes:
                np.testing.assert_array_equal(n[:, :S], nodes)
                assert np.all(n[:, S:] == 255)
            else:
                assert np.all(n == 255)
        d_t = torch.zeros((n_tips, ld), dtype=torch.uint8, device=dev)
        rc = N.lib().pu_simulate_device(tm._ctx, 6, 0, S, ctypes.c_void_p(d_t.data_ptr()), S - 1,
                                        None, None, 0)
        assert rc == N.PU_E_ARG
    finally:
        N.check(N.lib().pu_ctx_set_stream(tm._ctx, N.PU_OWN_STREAM), tm._ctx)


# ---------------------------------------------------------------------------- the seam
def seam_case(K, C, rng):
    if K == 2:
        return np.array([[[0.9, 0.1], [0.3, 0.7]]])
    p = rng.random((C, K, K)) + 0.01
    return p / p.sum(axis=2, keepdims=True)


@pytest.mark.parametrize("K,C", [(2, 1), (4, 4), (20, 4)])
def test_evolve_states_matches_pick(K, C):
    rng = np.random.default_rng(100 * K + C)
    probs = seam_case(K, C, rng)
    S = 1000
    parent = rng.integers(0, K, S).astype(np.uint8)
    cls = rng.integers(0, C, S).astype(np.uint8)
    seed, first, draw = 77, 2 ** 32 - 500, 5
    got = simulation.evolve_states(parent, cls, probs, seed, first_site=first, draw=draw)
    u = R.uniform(seed, np.uint64(first) + np.arange(S, dtype=np.uint64), draw)
    ref = R.pick_cum(R.cumulate(probs)[cls, parent], u)
    np.testing.assert_array_equal(got, ref)
    one = np.array([R.pick(probs[cls[s], parent[s]], float(u[s])) for s in range(0, S, 97)])
    np.testing.assert_array_equal(got[::97], one)
    # the reference's [K][K][C] layout gives the same states
    got2 = simulation.evolve_states(parent, cls, np.ascontiguousarray(probs.transpose(1, 2, 0)),
                                    seed, first_site=first, draw=draw, layout="kkc")
    np.testing.assert_array_equal(got2, got)
    if C == 1:
        np.testing.assert_array_equal(
            simulation.evolve_states(parent, None, probs, seed, first_site=first, draw=draw), got)


# ---------------------------------------------------------------------------- the context
def real_model(n_taxa=12, n_sites=300, seed=3):
    from phylo_utils_amd.synthetic import make_problem
    model, rm = gtr_g4()
    tree, names, st = make_problem(n_taxa, n_sites, model, rm.rates, seed=seed)
    tm = TreeModel()
    tm.set_tree(tree)
    tm.set_alignment_codes(st.astype(np.uint8), np.eye(4), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.initialise()
    return tm, model, rm


def test_context_is_untouched():
    tm, model, rm = real_model()
    lnl, site, root = tm.likelihood(), tm.sitewise_patterns().copy(), tm.root_partials.copy()
    dirty, cached = tm._dirty, tm._lnl
    check_against_restatement(tm, model, rm, 21, 0, 777)
    assert (tm._dirty, tm._lnl) == (dirty, cached)
    assert tm.likelihood() == lnl
    assert np.array_equal(tm.sitewise_patterns(), site)
    assert np.array_equal(tm.root_partials, root)
    tm.compute_partials()
    assert tm.likelihood() == lnl and np.array_equal(tm.sitewise_patterns(), site)


def test_lengths_moved_by_the_optimiser_are_used():
    tm, model, rm = real_model()
    a, b = tm.traversal.root_edge
    before = tm.traversal.root_length()
    t, lnl = tm.optimise_edge(a, b)
    assert abs(t - before) > 1e-6
    cum = check_against_restatement(tm, model, rm, 22, 0, 200)
    ref = R.cumulate(model.p(t, np.asarray(rm.rates, float)))
    np.testing.assert_allclose(cum[b], ref, rtol=1e-12, atol=4e-15)
    after = tm.likelihood()
    tm2, _, _ = real_model()
    tm2.optimise_edge(a, b)
    assert tm2.likelihood() == after  # the same lnL as without the simulation in between


# ---------------------------------------------------------------------------- host matrices
def test_host_matrix_context_uses_the_provider():
    model = SM.Unrest(load_golden("nonrev")["unrest_rates"])
    rm = GammaRateModel(4, 0.5)
    tm = dummy_model(_tree(5, 55), model, rm)
    cum = check_against_restatement(tm, model, rm, 31, 0, 1000)
    tr = tm.traversal
    a, b = tr.root_edge
    ref = R.cum_rows(model, np.asarray(rm.rates, float), tr.postorder_traversal, tr.op_lengths(),
                     a, b, tr.root_length(), tr.n_nodes)
    np.testing.assert_array_equal(cum, ref)  # the provider's P, cumulated in index order
    N.check(N.lib().pu_set_pmatrix_provider(tm._ctx, None, None), tm._ctx)
    out = np.zeros((5, 10), dtype=np.uint8)
    rc = N.lib().pu_simulate(tm._ctx, 0, 0, 10, N.ptr(out), None, None, None)
    assert rc == N.PU_E_STATE and "provider" in N.last_error(tm._ctx)


def test_refusals_on_a_context():
    lib = N.lib()
    ctx = ctypes.c_void_p()
    N.check(lib.pu_ctx_create(ctypes.byref(ctx), 0, 4, 3, 1, 4, 4, 0))
    out = np.zeros((3, 10), dtype=np.uint8)
    try:
        assert lib.pu_simulate(ctx, 0, 0, 10, N.ptr(out), None, None, None) == N.PU_E_STATE
        tm, _, _ = case("gtr3")
        assert lib.pu_simulate(tm._ctx, 0, 0, 0, N.ptr(out), None, None, None) == N.PU_E_ARG
        assert lib.pu_simulate(tm._ctx, 0, -1, 10, N.ptr(out), None, None, None) == N.PU_E_ARG
        assert lib.pu_simulate(tm._ctx, 0, 0, 10, None, None, None, None) == N.PU_E_ARG
    finally:
        lib.pu_ctx_destroy(ctx)


# ---------------------------------------------------------------------------- round trip
def test_simulated_alignment_is_valid_tip_input(oracle_mod):
    model, rm = gtr_g4()
    tree = _tree(17, 17)
    names, states = simulation.simulate_alignment(tree, model, rm, 20000, seed=5)
    assert states.shape == (17, 20000) and states.max() < 4
    tm = TreeModel()
    tm.set_tree(tree)
    tm.set_alignment_codes(states, np.eye(4), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.initialise()
    tr = tm.traversal
    eye = np.eye(4)
    tips = {tr.names[n]: eye[states[i]] for i, n in enumerate(names)}
    ev, el, iv = model.engine_eigen()
    ref, _ = oracle_mod.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                 tr.root_length(), ev, el, iv, model.freqs, rm.rates, rm.weights,
                                 n_nodes=tr.n_nodes, nthreads=8)
    assert abs(tm.likelihood() - ref) <= 1e-11 * abs(ref)
    # and the extras of simulate_alignment line up with the plain call
    n2, s2, cats, nodes = simulation.simulate_alignment(tree, model, rm, 500, seed=5,
                                                        return_categories=True,
                                                        return_ancestral=True)
    assert n2 == names and np.array_equal(s2, states[:, :500])
    assert cats.shape == (500,) and nodes.shape == (tr.n_nodes, 500)


def test_cli_writes_a_fasta(tmp_path):
    tree = _tree(6, 6)
    t = tmp_path / "t.nwk"
    t.write_text(tree.as_newick())
    out = tmp_path / "sim.fasta"
    assert phy.main(["-t", str(t), "-m", "GTR+G4{0.5}", "--simulate", "200", "--seed", "3",
                     "-o", str(out)]) == 0
    recs = A.read_fasta(str(out))
    assert sorted(n for n, _ in recs) == sorted("t%d" % i for i in range(6))
    assert all(len(s) == 200 and set(s) <= set("ACGT") for _, s in recs)
    names, states = simulation.simulate_alignment(str(t.read_text()), SM.GTR(),
                                                  GammaRateModel(4, 0.5), 200, seed=3)
    assert dict(recs) == dict(zip(names, simulation.states_to_sequences(states, A.DNA)))
