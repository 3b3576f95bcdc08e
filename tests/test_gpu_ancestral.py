"""Marginal ancestral states and site-rate posteriors on the device: the
k_ancestral kernel through pu_ancestral_sweep, pu_ancestral_edge and pu_site_rates against the
CPU restatement (tests/ancestral_reference.py, itself pinned against enumeration in
tests/test_ancestral.py).  Tolerance 1e-10 absolute on posteriors, that of tests/test_gpu_edges.py
and test_gpu_nni.py for the same per-site quantities, here on values <= 1.

Each case makes its device calls once (the `run` fixture); the tests below read what it kept."""
import ctypes

import numpy as np
import pytest

import ancestral_reference as R
import walk_errors as W

from phylo_utils_amd import TreeModel, ancestral
from phylo_utils_amd import _native as N
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import (CFG2_FREQS, CFG2_GTR_RATES, make_problem, random_tree,
                                       simulate_states)

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


@pytest.fixture(scope="module", params=sorted(R.CASES))
def run(request, oracle_mod):
    prob = R.problem(request.param)
    tr, e, ref = R.restate(oracle_mod, prob)
    tm = _tm(prob)
    left, right = (int(v) for v in tm.traversal.root_edge)
    probe = (left, int(ref["nodes"][-1]))
    before = dict(lnl=tm.likelihood(), site=tm.sitewise_patterns().copy(),
                  parts=[tm.node_partials(v) for v in probe])
    internal = set(ref["nodes"].tolist())
    # the single-edge call on a fresh traversal: the root edge's internal end from the other
    n, o = (left, right) if left in internal else (right, left)
    edge_full = ancestral.ancestral_edge(tm, n, o, full=True)
    edge_map = ancestral.ancestral_edge(tm, n, o)
    scale_root = tm.node_partials(left)[1] + tm.node_partials(right)[1]
    cat, rate = tm.site_rates()
    first = tm.ancestral_states(full=True)
    after = dict(lnl=tm.likelihood(), site=tm.sitewise_patterns().copy(),
                 parts=[tm.node_partials(v) for v in probe])
    second = tm.ancestral_states(full=True)
    brief = tm.ancestral_states()
    return dict(case=request.param, prob=prob, tr=tr, ref=ref, tm=tm, before=before, after=after,
                first=first, second=second, brief=brief, edge=(n, edge_full, edge_map),
                scale_root=scale_root, cat=cat, rate=rate)


def test_posteriors_map_prob_and_site_rates(run):
    ref, got = run["ref"], run["first"]
    assert got["nodes"].tolist() == ref["nodes"].tolist()
    errs = dict(posteriors=np.abs(got["posteriors"] - ref["posteriors"]).max(),
                map_prob=np.abs(got["map_prob"] - ref["posteriors"].max(axis=2)).max(),
                cat_post=np.abs(run["cat"] - ref["cat_post"]).max(),
                mean_rate=np.abs(run["rate"] - ref["mean_rate"]).max())
    print("%s: worst absolute errors %s" % (run["case"], {k: "%.2e" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v <= 1e-10, (k, v)


def test_map_state(run):
    ref, got = run["ref"], run["first"]
    ok = R.decided(ref["posteriors"])
    assert (~ok).mean() <= 0.01
    assert np.array_equal(got["map_state"][ok], ref["posteriors"].argmax(axis=2)[ok])
    # the state reported is the one whose posterior is reported
    q = np.take_along_axis(got["posteriors"], got["map_state"][..., None].astype(np.int64), 2)
    assert np.array_equal(q[..., 0], got["map_prob"])
    assert np.array_equal(got["map_prob"], got["posteriors"].max(axis=2))


def test_node_lnl_is_the_tree_lnl(run):
    lnl = run["before"]["lnl"]
    assert abs(lnl - run["ref"]["lnl"]) <= 1e-10 * abs(lnl)
    worst = np.abs(run["first"]["node_lnl"] - lnl).max() / abs(lnl)
    print("%s: node_lnl worst relative error %.2e" % (run["case"], worst))
    assert worst <= 1e-10


def test_every_internal_node_once(run):
    nodes = run["first"]["nodes"].tolist()
    internal = sorted(set(int(p) for p in run["tr"].postorder_traversal[:, 0]))
    assert sorted(nodes) == internal and len(nodes) == len(run["prob"]["names"]) - 2


def test_state_after_the_call_is_bitwise_unchanged(run):
    b, a = run["before"], run["after"]
    assert a["lnl"] == b["lnl"]
    assert np.array_equal(a["site"], b["site"])
    for (p0, s0), (p1, s1) in zip(b["parts"], a["parts"]):
        assert np.array_equal(p0, p1) and np.array_equal(s0, s1)


def test_single_edge_call_equals_the_sweep_entry(run):
    n, full, brief = run["edge"]
    got = run["first"]
    i = got["nodes"].tolist().index(n)
    assert np.array_equal(full["posteriors"], got["posteriors"][i])
    assert np.array_equal(full["map_state"], got["map_state"][i])
    assert np.array_equal(full["map_prob"], got["map_prob"][i])
    assert full["lnl"] == got["node_lnl"][i]
    assert np.array_equal(brief["map_state"], full["map_state"])
    assert np.array_equal(brief["map_prob"], full["map_prob"])
    assert brief["lnl"] == full["lnl"]


def test_repeat_is_bitwise(run):
    a, b, c = run["first"], run["second"], run["brief"]
    for k in ("nodes", "map_state", "map_prob", "node_lnl", "posteriors"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("nodes", "map_state", "map_prob", "node_lnl"):
        assert np.array_equal(a[k], c[k]), k
    assert "posteriors" not in c


def test_posteriors_sum_to_one(run):
    assert np.abs(run["first"]["posteriors"].sum(axis=2) - 1).max() <= 1e-12
    assert np.abs(run["cat"].sum(axis=1) - 1).max() <= 1e-12


def test_caterpillar_scalers_differ_between_categories(run):
    """The exp(sigma_c - m) path runs: on the device's own scalers at the root edge, at least one
    site has categories with different sigma."""
    if "caterpillar" not in run["case"]:
        return
    sig = run["scale_root"]
    assert (sig != 0).any() and (sig.max(axis=1) != sig.min(axis=1)).any()


def test_pendant_root_edge(run):
    if "pendant" not in run["case"]:
        return
    tm = run["tm"]
    left, right = (int(v) for v in tm.traversal.root_edge)
    assert left in tm.names.values() and right not in tm.names.values()
    assert run["edge"][0] == right
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*is a tip"):
        ancestral.ancestral_edge(tm, left, right)


def test_cherry_parent_takes_the_shared_tip_state():
    """All lengths 0.01: where the two tips of a cherry agree, their parent's MAP state is
    theirs."""
    rng = np.random.default_rng(3)
    m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    tree = random_tree(rng, 10, lo=0.01, hi=0.01)
    sts = simulate_states(rng, tree, m, rm.rates, 200)
    names = sorted(sts, key=lambda s: int(s[1:]))
    codes = np.array([sts[n] for n in names], dtype=np.uint8)
    tm = _tm(dict(tree=tree, names=names, codes=codes, table=np.eye(4), model=m, rm=rm,
                  compact=True, weights=np.ones(200)))
    res = tm.ancestral_states()
    tip_row = {node: names.index(label) for label, node in tm.traversal.names.items()}
    n_cherries = 0
    for p, a, b in tm.traversal.postorder_traversal:
        if int(a) in tip_row and int(b) in tip_row:
            sa, sb = codes[tip_row[int(a)]], codes[tip_row[int(b)]]
            same = sa == sb
            got = res["map_state"][res["nodes"].tolist().index(int(p))]
            assert same.any() and np.array_equal(got[same], sa[same])
            n_cherries += 1
    assert n_cherries >= 1


def test_refusals():
    kmax = N.lib().pu_ancestral_max_cat(20)
    assert kmax < 64
    m, rm = SM.LG(), GammaRateModel(kmax + 1, 0.8)
    tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
    prob = dict(tree=tree, names=names, codes=st.astype(np.uint8), table=np.eye(20), model=m,
                rm=rm, compact=True, weights=np.ones(70))
    tm = _tm(prob)
    lnl0 = tm.likelihood()
    for call in (tm.ancestral_states, tm.site_rates):
        with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
            call()
    assert tm.likelihood() == lnl0
    # one above the binary limit is more than a context holds
    with pytest.raises((N.PhyloHipError, ValueError)):
        two = R.problem("binary-8x70-Cmax")
        two["rm"] = GammaRateModel(N.lib().pu_ancestral_max_cat(2) + 1, 0.5)
        _tm(two).ancestral_states()
    prob = R.problem("dna-8x65-C3")
    tm = _tm(prob, keep=False)
    for call in (tm.ancestral_states, tm.site_rates):
        with pytest.raises(ValueError, match="keep_partials"):
            call()
    tm = _tm(prob)
    inner = sorted(set(int(p) for p in tm.traversal.postorder_traversal[:, 0]))
    left, right = (int(v) for v in tm.traversal.root_edge)
    S = prob["codes"].shape[1]
    st8, pr, lnl = np.zeros(S, dtype=np.uint8), np.zeros(S), ctypes.c_double()
    edge = lambda *a: N.lib().pu_ancestral_edge(tm._ctx, *a)
    good = (left, right, -1.0, N.ptr(st8), N.ptr(pr), None, ctypes.byref(lnl))
    assert edge(*good) == 0
    assert edge(left, right, 0.0, *good[3:]) == N.PU_E_ARG
    assert edge(left, right, float("nan"), *good[3:]) == N.PU_E_ARG
    assert edge(left, right, float("inf"), *good[3:]) == N.PU_E_ARG
    assert edge(left, 10 ** 6, -1.0, *good[3:]) == N.PU_E_ARG
    assert edge(left, right, -1.0, None, N.ptr(pr), None, ctypes.byref(lnl)) == N.PU_E_ARG
    far = next(v for v in inner if v not in (left, right) and
               tuple(sorted((v, left))) not in tm.traversal.brlens)
    assert edge(left, far, -1.0, *good[3:]) == N.PU_E_ARG
    assert N.lib().pu_site_rates(tm._ctx, None, None) == N.PU_E_ARG
    tm.set_ascertainment_bias_correction()
    for call in (tm.ancestral_states, tm.site_rates):
        with pytest.raises(ValueError, match="ascertainment"):
            call()
    un = dict(prob, model=SM.Unrest(), rm=UniformRateModel())
    tm = _tm(un)
    for call in (tm.ancestral_states, tm.site_rates):
        with pytest.raises(ValueError, match="reversible"):
            call()


def test_an_error_in_mid_walk_puts_the_context_back():
    """pu_ancestral_sweep on rows whose last edge names a PAR that is not NOD's neighbour
    (walk_errors.py): PU_E_ARG, and the lnL, sitewise lnL and partials are pu_run's again."""
    prob = R.problem("dna-8x65-C3")
    tm = _tm(prob)
    tm.likelihood()
    bad = W.rows_with_a_bad_last_edge(tm)
    before = W.snapshot(tm)
    n, S = len(tm.names) - 2, prob["codes"].shape[1]
    nodes, st8, pr, lnl, cnt = (np.zeros(n, dtype=np.int32), np.zeros((n, S), dtype=np.uint8),
                                np.zeros((n, S)), np.zeros(n), ctypes.c_int())
    rc = N.lib().pu_ancestral_sweep(tm._ctx, len(bad), N.ptr(bad), N.ptr(nodes), N.ptr(st8),
                                    N.ptr(pr), None, N.ptr(lnl), ctypes.byref(cnt))
    W.assert_refused_and_put_back(tm, before, rc)
