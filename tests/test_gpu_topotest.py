"""Topology tests on the device: the scaled weights (pu_boot_weights_scaled) and
the counts (pu_topology_tests) against the CPU restatement (tests/topotest_reference.py), bit for
bit, and ``topology_tests`` on small TreeModels."""
import os
import re

import numpy as np
import pytest

import topotest_reference as TR

from phylo_utils_amd import TreeModel, bootstrap, support, topotest
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, InvariantGammaModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem, random_tree
from phylo_utils_amd.tree import apply_nni, internal_edges, prepare_tree

pytestmark = pytest.mark.gpu

SCALES3 = [0.5, 1.25, 2.0]  # below and above 1


def _w(S, seed=0):
    """Non-unit integer weights with zeros among them."""
    w = np.random.default_rng(100 + S + seed).integers(0, 5, S)
    if S > 2:
        w[1] = 0
    w[-1] = 3
    return w.astype(np.float64)


# ---- scaled weights ----------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 63, 2049])
def test_scaled_weights(S):
    w = _w(S)
    Nw = int(w.sum())
    R = 3 if S > 1000 else 5
    draws = sorted({1, max(1, Nw // 2), Nw, Nw + Nw // 3 + 1})
    for n in draws:
        got = topotest.scaled_bootstrap_weights(w, n, R, seed=5, first_replicate=7)
        assert got.dtype == np.uint32 and got.shape == (R, S)
        assert (got.sum(axis=1) == n).all() and not got[:, w == 0].any()
        assert np.array_equal(got, TR.scaled_weights(w, n, R, seed=5, first_rep=7)), n
    full = topotest.scaled_bootstrap_weights(w, Nw, R, seed=5, first_replicate=7)
    assert np.array_equal(full, bootstrap.bootstrap_weights(w, R, seed=5, first_replicate=7))
    # unit weights by a site count
    assert np.array_equal(topotest.scaled_bootstrap_weights(S, S + 2, 2, seed=1),
                          TR.scaled_weights(S, S + 2, 2, seed=1))
    # a range straddling two blocks (one n_draw per row) is the two calls, row for row
    lo, hi = draws[1], draws[-1]
    rows = topotest.scaled_bootstrap_weights(w, [lo, lo, hi, hi, hi][:R], R, seed=5,
                                             first_replicate=7)
    a = topotest.scaled_bootstrap_weights(w, lo, 2, seed=5, first_replicate=7)
    b = topotest.scaled_bootstrap_weights(w, hi, R - 2, seed=5, first_replicate=9)
    assert np.array_equal(rows, np.vstack([a, b]))


# ---- counts ------------------------------------------------------------------------------------

def _L(T, S, seed=0):
    """Per-pattern lnL of T trees that are close to each other: a common row plus small
    differences, so that every count sees wins and losses."""
    rng = np.random.default_rng(7 * T + S + seed)
    return -rng.gamma(2.0, 3.0, S)[None, :] + 0.3 * rng.standard_normal((T, S))


def _reference(L, w, R, scales, seed, first_rep=0):
    """The restatement with B from the existing RELL product on the restated weights."""
    return TR.topology_tests(L, w, R, scales, seed, first_rep,
                             sums=lambda W, L: support.rell_sums(L, W))


def _check(raw, ref):
    assert np.array_equal(raw["n_draw"], ref["n_draw"])
    assert np.array_equal(raw["lnl"], ref["lnl"], equal_nan=True)
    assert np.array_equal(raw["rell"], ref["B"], equal_nan=True)
    assert np.array_equal(raw["counts"], ref["counts"])


CASES = [  # T, R, S, scales: T crosses the 48-vector tile, R the 128-replicate tile (and the
           # kernel's 256 rows), S a RELL segment
    (2, 1, 63, []), (3, 129, 63, SCALES3), (49, 300, 63, []), (3, 300, 2049, []),
    (49, 129, 2049, SCALES3), (2, 300, 63, SCALES3),
]


@pytest.fixture(scope="module")
def shared():
    """One call and its restatement for the tests that vary how the call is made."""
    T, R, S = 5, 130, 63
    L, w = _L(T, S), _w(S)
    ref = _reference(L, w, R, SCALES3, seed=11)
    raw = topotest.topology_counts(L, w, R, SCALES3, seed=11, return_rell=True)
    return L, w, R, ref, raw


@pytest.mark.parametrize("T,R,S,scales", CASES)
def test_counts_vs_restatement(T, R, S, scales):
    L, w = _L(T, S), _w(S)
    raw = topotest.topology_counts(L, w, R, scales, seed=3, first_replicate=2, return_rell=True)
    ref = _reference(L, w, R, scales, seed=3, first_rep=2)
    _check(raw, ref)
    cnt = raw["counts"]
    assert (cnt[:, 0].sum(axis=1) == R).all() and not cnt[1:, 1:].any()
    assert cnt[0, 2].max() == R  # the best tree by l is never rejected by SH
    # block 0 draws bootstrap_weights' rows: its sums are those of the SH-aLRT rows
    W0 = bootstrap.bootstrap_weights(w, R, seed=3, first_replicate=2)
    assert np.array_equal(raw["rell"][0], support.rell_sums(L, W0))
    # without the sums the counts are the same
    lean = topotest.topology_counts(L, w, R, scales, seed=3, first_replicate=2)
    assert "rell" not in lean and np.array_equal(lean["counts"], cnt)


def test_counts_do_not_depend_on_the_ranges(shared):
    L, w, R, ref, raw = shared
    _check(raw, ref)
    old = os.environ.get("PU_TOPO_REP_CHUNK")
    try:
        for cap in ("1", "7"):
            os.environ["PU_TOPO_REP_CHUNK"] = cap
            got = topotest.topology_counts(L, w, R, SCALES3, seed=11, return_rell=True)
            for f in ("counts", "lnl", "n_draw", "rell"):
                assert np.array_equal(got[f], raw[f]), (cap, f)
    finally:
        if old is None:
            os.environ.pop("PU_TOPO_REP_CHUNK", None)
        else:
            os.environ["PU_TOPO_REP_CHUNK"] = old


def test_counts_permute_with_the_trees(shared):
    L, w, R, ref, raw = shared
    # no ties: every comparison the rule makes is strict on these data
    B = ref["B"]
    assert all(len(set(row)) == len(row) for row in B.reshape(-1, B.shape[2]))
    perm = np.array([3, 0, 4, 2, 1])
    got = topotest.topology_counts(L[perm], w, R, SCALES3, seed=11, return_rell=True)
    assert np.array_equal(got["counts"], raw["counts"][:, :, perm])
    assert np.array_equal(got["lnl"], raw["lnl"][perm])
    assert np.array_equal(got["rell"], raw["rell"][:, :, perm])


def test_first_replicate_continues_a_series(shared):
    L, w, R, ref, raw = shared
    # K = 0: rows first_rep .. first_rep + R - 1 are one block, so two calls tile one
    one = topotest.topology_counts(L, w, R, (), seed=11, return_rell=True)
    a = topotest.topology_counts(L, w, 50, (), seed=11, return_rell=True)
    b = topotest.topology_counts(L, w, R - 50, (), seed=11, first_replicate=50, return_rell=True)
    assert np.array_equal(np.concatenate([a["rell"][0], b["rell"][0]]), one["rell"][0])
    assert np.array_equal(a["counts"] + b["counts"], one["counts"])
    assert np.array_equal(one["rell"][0], raw["rell"][0])
    # with scales, block k of a call is block 0's rule at replicate numbers first_rep + k R + i
    n1 = int(raw["n_draw"][1])
    W1 = topotest.scaled_bootstrap_weights(w, n1, R, seed=11, first_replicate=R)
    assert np.array_equal(raw["rell"][1], support.rell_sums(L, W1))


def test_an_impossible_tree_is_excluded(shared):
    L, w, R, ref, raw = shared
    p = int(np.nonzero(w > 0)[0][3])
    z = int(np.nonzero(w == 0)[0][0])
    bad = L[2].copy()
    bad[p] = -np.inf
    L2 = np.vstack([L[:2], bad[None, :], L[2:]])
    L2[:, z] = -np.inf  # a pattern of weight 0 at -inf excludes nobody
    got = topotest.topology_counts(L2, w, R, SCALES3, seed=11, return_rell=True)
    keep = [0, 1, 3, 4, 5]
    assert got["lnl"][2] == -np.inf and not got["counts"][:, :, 2].any()
    assert np.array_equal(got["counts"][:, :, keep], raw["counts"])
    assert np.array_equal(got["lnl"][keep], raw["lnl"])
    _check(got, _reference(L2, w, R, SCALES3, seed=11))
    fin = topotest.finish(got, R)
    assert fin["bp"][2] == 0 and fin["p_sh"][2] == 0 and fin["c_elw"][2] == 0 and fin["p_au"][2] == 0
    # all but one excluded: that one wins every replicate and no test rejects it
    L3 = np.vstack([bad, L[1], bad])
    got = topotest.topology_counts(L3, w, R, (), seed=11, return_rell=True)
    assert got["counts"][0].tolist() == [[0, R, 0]] * 3
    _check(got, _reference(L3, w, R, (), 11))


def test_exact_ties_go_to_the_lowest_index(shared):
    L, w, R, ref, raw = shared
    L2 = L[[1, 0, 1, 0, 1]]
    got = topotest.topology_counts(L2, w, R, SCALES3, seed=11, return_rell=True)
    _check(got, _reference(L2, w, R, SCALES3, seed=11))
    cnt = got["counts"]
    assert not cnt[:, 0, 2:].any() and (cnt[:, 0, :2].sum(axis=1) == R).all()
    assert np.array_equal(cnt[0, 1:, 0], cnt[0, 1:, 2]) and np.array_equal(cnt[0, 1:, 1], cnt[0, 1:, 3])
    same = topotest.topology_counts(np.stack([L[0]] * 3), w, R, (), seed=11)
    assert same["counts"][0].tolist() == [[R, 0, 0], [R] * 3, [R] * 3]


def test_refusals(shared):
    L, w, R, ref, raw = shared
    lib = N.lib()
    T, S = L.shape
    sc = np.array(SCALES3)
    cnt = np.zeros((4, 3, T), dtype=np.uint32)
    lnl, nd = np.zeros(T), np.zeros(4, dtype=np.int64)

    def call(T=T, S=S, L=L, w=w, first=0, R=R, K=3, sc=sc, cnt=cnt, lnl=lnl, nd=nd):
        # device 99 does not exist: an argument error must come first
        return lib.pu_topology_tests(99, T, S, N.ptr(L), N.ptr(w), 11, first, R, K, N.ptr(sc),
                                     N.ptr(cnt), N.ptr(lnl), N.ptr(nd), None)

    w_frac, w_neg, w_zero, w_big = w.copy(), w.copy(), np.zeros(S), w.copy()
    w_frac[0], w_neg[0], w_big[:] = 0.5, -1.0, 2.0 ** 30
    for kw, msg in ((dict(L=None), "null buffer"), (dict(w=None), "null buffer"),
                    (dict(cnt=None), "null buffer"), (dict(lnl=None), "null buffer"),
                    (dict(nd=None), "null buffer"), (dict(sc=None), "scales"),
                    (dict(T=1), "T = 1"), (dict(T=1025), "T = 1025"), (dict(S=0), "S = 0"),
                    (dict(R=0), "R = 0"), (dict(K=-1), "K = -1"),
                    (dict(sc=np.array([0.5, 0.0, 2.0])), r"scales\[1\]"),
                    (dict(sc=np.array([0.5, 1.0, np.inf])), r"scales\[2\]"),
                    (dict(sc=np.array([np.nan, 1.0, 2.0])), r"scales\[0\]"),
                    (dict(sc=np.array([1e-9, 1.0, 2.0])), r"scales\[0\]"),
                    (dict(sc=np.array([0.5, 1.0, 1e12])), r"scales\[2\]"),
                    (dict(w=w_frac), r"site_weights\[0\]"), (dict(w=w_neg), r"site_weights\[0\]"),
                    (dict(w=w_zero), "site_weights sum"), (dict(w=w_big), "site_weights sum"),
                    (dict(first=-1), "first_rep"), (dict(first=2 ** 32 - 4 * R + 1), "first_rep")):
        assert call(**kw) == N.PU_E_ARG, kw
        err = N.last_error()
        assert "pu_topology_tests" in err and re.search(msg, err), (kw, err)
    # the last replicate is 2^32 - 1: accepted, and only then is the device looked at
    assert call(first=2 ** 32 - 4 * R) == N.PU_E_ARG and "device 99" in N.last_error()
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*n_draw"):
        topotest.scaled_bootstrap_weights(w, 0, 2)
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*n_draws\[1\]"):
        topotest.scaled_bootstrap_weights(w, [3, 2 ** 31], 2)
    # a later valid call still works
    again = topotest.topology_counts(L, w, R, SCALES3, seed=11, return_rell=True)
    assert all(np.array_equal(again[f], raw[f]) for f in ("counts", "lnl", "n_draw", "rell"))


def test_profile_records_the_three_stages(shared):
    import ctypes
    L, w, R, ref, raw = shared
    lib = N.lib()
    ms = [ctypes.c_double(-1.0) for _ in range(3)]
    N.check(lib.pu_topotest_profile(0, 1), None, "pu_topotest_profile")
    try:
        assert lib.pu_topotest_kernel_ms(0, *map(ctypes.byref, ms)) == N.PU_E_STATE
        got = topotest.topology_counts(L, w, R, SCALES3, seed=11)
        N.check(lib.pu_topotest_kernel_ms(0, *map(ctypes.byref, ms)), None, "pu_topotest_kernel_ms")
    finally:
        N.check(lib.pu_topotest_profile(0, 0), None, "pu_topotest_profile")
    assert all(0.0 < x.value < 1e4 for x in ms)
    assert np.array_equal(got["counts"], raw["counts"])


# ---- topology_tests on a TreeModel -------------------------------------------------------------

def _model(kind, n_taxa, n_sites, seed, pinvar=None):
    if kind == "dna":
        m, alphabet = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), "ACGT"
    else:
        m, alphabet = SM.LG(), "ARNDCQEGHILKMFPSTWYV"
    rm = GammaRateModel(4, 0.5) if pinvar is None else InvariantGammaModel(pinvar, 4, 0.5)
    tree, names, st = make_problem(n_taxa, n_sites, m, rm.rates, seed=seed)
    tm = TreeModel(device=0)
    tm.set_alignment([(n, "".join(alphabet[x] for x in row)) for n, row in zip(names, st)],
                     A.DNA if kind == "dna" else A.PROTEIN)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    true = prepare_tree(tree)
    nod, par = internal_edges(true)[0]
    trees = [true, apply_nni(true, nod, par, 1),
             random_tree(np.random.default_rng(50 + seed), n_taxa)]
    return tm, trees


def _state(tm):
    return (tm.tree.as_newick(), dict(tm.traversal.brlens), tm.likelihood(),
            tm.sitewise_patterns().copy())


def _same_state(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("case", ["gtr-g4-8x200", "lg-g4-6x120", "gtr-g4-i-8x200"])
def test_topology_tests_on_a_tree_model(case):
    kind, n_taxa, n_sites, pinvar = {"gtr-g4-8x200": ("dna", 8, 200, None),
                                     "lg-g4-6x120": ("protein", 6, 120, None),
                                     "gtr-g4-i-8x200": ("dna", 8, 200, 0.2)}[case]
    tm, trees = _model(kind, n_taxa, n_sites, seed=4, pinvar=pinvar)
    before = _state(tm)
    R, scales = 200, [0.5, 0.75, 1.0, 1.5]
    res = tm.topology_tests(trees, n_replicates=R, scales=scales, seed=2)
    _same_state(_state(tm), before)
    assert all(res[f].shape == (3,) for f in topotest.FIELDS) and len(res["trees"]) == 3
    # the rows the call used are the model's sitewise_patterns() of every tree at the lengths used
    w = np.asarray(tm.siteweights, dtype=np.float64)
    assert w.max() > 1 or kind == "protein"
    for nwk, row in zip(res["trees"], res["site_lnl"]):
        tm.set_tree(nwk)
        tm.initialise()
        assert np.allclose(tm.sitewise_patterns(), row, rtol=1e-10, atol=0)
    tm.set_tree(trees[0])
    tm.initialise()
    # the restatement fed with those rows
    ref = _reference(res["site_lnl"], w, R, scales, seed=2)
    assert np.array_equal(res["counts"], ref["counts"])
    assert np.array_equal(res["n_draw"], ref["n_draw"]) and np.array_equal(res["lnl"], ref["lnl"])
    for f in ("bp", "p_kh", "p_sh"):
        assert np.array_equal(res[f], ref[f]), f
    assert np.allclose(res["c_elw"], ref["c_elw"], rtol=1e-12, atol=0)
    assert np.array_equal(res["au_scales"], ref["au_scales"])
    assert np.allclose(res["p_au"], ref["p_au"], rtol=0, atol=1e-9, equal_nan=True)
    assert res["delta"][int(np.argmax(res["lnl"]))] == 0.0
    # optimised lengths: every tree's lnL is at least what its given lengths reach
    plain = tm.topology_tests(trees, n_replicates=R, scales=(), seed=2, optimise=False)
    assert (res["lnl"] >= plain["lnl"] - 1e-6).all()
    assert np.isnan(plain["p_au"]).sum() + (plain["p_au"] == 0).sum() + (plain["p_au"] == 1).sum() == 3


def test_the_model_is_restored_after_an_error():
    tm, trees = _model("dna", 8, 200, seed=4)
    before = _state(tm)
    with pytest.raises(ValueError):
        tm.topology_tests([trees[1], "((t0,t1),(t2,;"], n_replicates=10)
    _same_state(_state(tm), before)
    with pytest.raises(ValueError, match="taxa differ"):
        tm.topology_tests([trees[1], "((t0,t1),(t2,x9));"], n_replicates=10)
    _same_state(_state(tm), before)
    with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
        tm.topology_tests(trees, n_replicates=0)
    _same_state(_state(tm), before)
    # after optimisation too: the lengths and the lnL that the optimiser left come back
    tm.optimise_branch_lengths()
    tm.compute_partials()
    before = _state(tm)
    tm.topology_tests(trees[1:], n_replicates=10, scales=())
    _same_state(_state(tm), before)
