"""Branch supports on the device: the per-pattern lnL of the quartet kernel
(pu_quartet_site_lnl) against the oracle, the RELL product (pu_rell_sums) against exact sums,
and the pass (pu_branch_support) against the CPU restatement (tests/support_reference.py)."""
import ctypes
import math

import numpy as np
import pytest

import nni_reference as R
import support_reference as SR
import test_gpu_nni as G
from test_cli import _write_case

from phylo_utils_amd import TreeModel, phy, support
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import make_problem, simulate_states
from phylo_utils_amd.tree import apply_nni, internal_edges, prepare_tree

pytestmark = pytest.mark.gpu


def _check_site(tm, oracle_mod, P, S, e, nodes):
    w = np.asarray(tm.siteweights, dtype=np.float64)
    worst = 0.0
    for t in (None, (1e-6, 0.05, 3.0)):
        site, out9 = tm.quartet_site_lnl(nodes, G.LENS, t)
        ref = SR.site_lnl(oracle_mod, P, S, nodes, G.LENS, t, e)
        assert site.shape == ref.shape
        err = np.abs(site - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert (err <= 1e-10).all(), float(err.max())
        assert np.array_equal(out9, tm.quartet_derivatives(nodes, G.LENS, t))
        for k in range(3):
            tot = math.fsum(w * site[k])
            assert abs(tot - out9[k, 0]) <= 1e-11 * abs(out9[k, 0]), (tot, out9[k, 0])
    return worst


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_site_lnl_vs_oracle(oracle_mod, case):
    kind, n_taxa, n_sites, C, compact = G.CASES[case]
    tm, tree, e, tips = G._setup(kind, n_taxa, n_sites, C, seed=2, compact=compact)
    st = R.state(oracle_mod, tips, tm.traversal, e)
    lnl0 = tm.likelihood()
    worst = max(_check_site(tm, oracle_mod, st["partials"], st["scale"], e, nodes)
                for nodes in G._node_sets(tm.traversal))
    print("%s: max error relative to max(1, |v|) %.2e" % (case, worst))
    assert tm.likelihood() == lnl0


def test_site_lnl_on_rescaled_nodes(oracle_mod):
    """The 150-taxon caterpillar of test_gpu_nni: the scaler term enters s_k."""
    rng = np.random.default_rng(5)
    m, rm = G.GTR(), G.rates_of(4)
    tree = G._caterpillar(150, rng)
    sts = simulate_states(rng, tree, m, rm.rates, 130)
    names = sorted(sts)
    codes = np.array([sts[n] for n in names], dtype=np.uint8)
    tm = G._tm(tree, names, codes, np.eye(4), m, rm)
    tr = tm.traversal
    e = R.eigen(m, rm)
    tips = {tr.names[n]: np.eye(4)[codes[i]] for i, n in enumerate(names)}
    st = R.state(oracle_mod, tips, tr, e)
    inner = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    nodes = (inner[-2], inner[-3], inner[-5], inner[len(inner) // 2])
    assert all((st["scale"][v] != 0).any() for v in nodes[:3])
    _check_site(tm, oracle_mod, st["partials"], st["scale"], e, nodes)


# ---- RELL ------------------------------------------------------------------------------------

def _rell_case(S, n_rep, n_vec, seed=0):
    rng = np.random.default_rng(1000 * S + 10 * n_rep + n_vec + seed)
    L = -rng.gamma(2.0, 3.0, (n_vec, S))
    W = rng.poisson(1.0, (n_rep, S)).astype(np.uint32)
    if S > 2:  # zero weights on a -inf and a NaN entry of every vector
        L[:, 0], L[:, S - 2] = -np.inf, np.nan
        W[:, 0] = W[:, S - 2] = 0
    return L, W


def _rell_check(L, W, got):
    S = L.shape[1]
    assert np.isfinite(got).all()
    Lf = np.where(W.any(axis=0)[None, :], L, 0.0)  # columns no replicate weighs
    for r in range(len(W)):
        for v in range(len(L)):
            ref = SR.rell(W[r], L[v])
            bound = S * 2.0 ** -53 * float(np.sum(W[r] * np.abs(Lf[v])))
            assert abs(got[r, v] - ref) <= bound, (r, v, got[r, v], ref, bound)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1000])
def test_rell_vs_exact_sum(S):
    full = {}
    L0, W0 = _rell_case(S, 100, 21)
    for n_rep in (1, 17, 100):
        for n_vec in (1, 3, 21):
            L, W = L0[:n_vec], W0[:n_rep]
            got = support.rell_sums(L, W)
            assert got.shape == (n_rep, n_vec)
            if n_rep == 17:
                _rell_check(L, W, got)
            full[n_rep, n_vec] = got
    _rell_check(L0, W0[[0, 99]], full[100, 21][[0, 99]])
    # out[r][v] depends on (W[r], L[v], S) alone: every call is a corner of the largest
    big = full[100, 21]
    for (n_rep, n_vec), got in full.items():
        assert np.array_equal(got, big[:n_rep, :n_vec]), (n_rep, n_vec)


def test_rell_layout_independence():
    S = 4500  # three segments, the last one partial
    L, W = _rell_case(S, 100, 21)
    big = support.rell_sums(L, W)
    _rell_check(L[:2], W[:3], big[:3, :2])
    # one vector alone against the same vector among 21, wherever it stands
    for v in (0, 7, 20):
        assert np.array_equal(support.rell_sums(L[v], W)[:, 0], big[:, v])
    # one call of 100 replicates against calls of 1 and 33
    assert np.array_equal(support.rell_sums(L, W[41]), big[41:42])
    for r0 in (0, 33, 66, 99):
        assert np.array_equal(support.rell_sums(L, W[r0:r0 + 33]), big[r0:r0 + 33])
    # a weight of 0 against -inf and NaN; a positive weight on -inf gives -inf
    W2 = W[:2].copy()
    W2[1, 0] = 1
    got = support.rell_sums(L, W2)
    assert np.isfinite(got[0]).all() and np.isneginf(got[1]).all()


def test_rell_device_form_with_padded_rows():
    import torch
    S, n_rep, n_vec = 1000, 37, 5
    L, W = _rell_case(S, n_rep, n_vec)
    want = support.rell_sums(L, W)
    dev = torch.device("cuda", 0)
    ldl, ldw, ldo = S + 24, S + 7, n_vec + 3
    d_L = torch.full((n_vec, ldl), float("nan"), dtype=torch.float64, device=dev)
    d_L[:, :S] = torch.from_numpy(L).to(dev)
    d_W = torch.full((n_rep, ldw), 9, dtype=torch.int32, device=dev)
    d_W[:, :S] = torch.from_numpy(W.astype(np.int32)).to(dev)
    d_out = torch.full((n_rep, ldo), -7.0, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    N.check(N.lib().pu_rell_sums_device(0, stream, n_vec, S, p(d_L), ldl, n_rep, p(d_W), ldw,
                                        p(d_out), ldo), None, "pu_rell_sums_device")
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:, :n_vec], want)
    assert (out[:, n_vec:] == -7.0).all()
    # refused before anything is queued: strides below their rows
    for bad in ((S - 1, ldw, ldo), (ldl, S - 1, ldo), (ldl, ldw, n_vec - 1)):
        rc = N.lib().pu_rell_sums_device(0, stream, n_vec, S, p(d_L), bad[0], n_rep, p(d_W),
                                         bad[1], p(d_out), bad[2])
        assert rc == N.PU_E_ARG
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_out.cpu().numpy(), out)


def test_rell_refusals():
    L, W, out = np.zeros((2, 8)), np.ones((3, 8), dtype=np.uint32), np.zeros((3, 2))
    lib = N.lib()
    # device 99 does not exist: an argument error must come first
    for args in ((0, 8, N.ptr(L), 3, N.ptr(W), N.ptr(out)), (2, 0, N.ptr(L), 3, N.ptr(W), N.ptr(out)),
                 (2, 8, N.ptr(L), 0, N.ptr(W), N.ptr(out)), (2, 8, None, 3, N.ptr(W), N.ptr(out)),
                 (2, 8, N.ptr(L), 3, None, N.ptr(out)), (2, 8, N.ptr(L), 3, N.ptr(W), None)):
        assert lib.pu_rell_sums(99, *args) == N.PU_E_ARG
        assert "pu_rell_sums" in N.last_error()
    with pytest.raises(ValueError):
        support.rell_sums(np.zeros((2, 8)), np.ones((3, 9), dtype=np.uint32))


# ---- the pass --------------------------------------------------------------------------------

def _compare_pass(got, ref, n_rep):
    """got: branch_support(full=True); ref: SR.branch_support's per-edge dicts.  The restatement
    alone first shows that no replicate of any edge sits on the threshold."""
    quartets, scores, sup, rell = got
    for x in ref:
        assert (np.abs(x["d"] - (x["gaps"] + 0.05)) >= 1e-6).all()
    assert rell.shape == (len(ref), n_rep + 1, 3)
    for i, x in enumerate(ref):
        want = np.vstack([x["l"][None, :], x["B"]])
        assert (np.abs(rell[i] - want) <= 1e-9 * np.maximum(1.0, np.abs(want))).all()
        G._close(sup["lrt"][i], x["lrt"], 1e-9)
        G._close(sup["abayes"][i], x["abayes"], 1e-9)
        G._close(sup["alrt_chi2"][i], x["alrt_chi2"], 1e-9)
        cnt = sup["sh_alrt"][i] * n_rep
        assert abs(cnt - round(cnt)) < 1e-9 and round(cnt) == x["count"], (i, cnt, x["count"])


@pytest.mark.parametrize("kind", ["dna", "protein"])
def test_pass_vs_restatement(oracle_mod, kind):
    tm, tree, e, tips = G._setup(kind, 10, 600, 4, seed=4)
    lnl0, site0, bl0 = tm.likelihood(), tm.sitewise_patterns().copy(), G._branch_lengths(tm)
    q0, s0 = tm.nni_scores(tol=1e-8, max_iter=50)
    got = tm.branch_support(n_replicates=100, seed=7, full=True)
    quartets, scores, sup, rell = got
    assert np.array_equal(quartets, q0) and np.array_equal(scores, s0)
    assert len(quartets) == 10 - 3
    # the context is where a traversal leaves it, bit for bit, and no length moved
    assert tm.likelihood() == lnl0
    assert np.array_equal(tm.sitewise_patterns(), site0)
    bl1 = G._branch_lengths(tm)
    assert np.array_equal(bl1[0], bl0[0]) and bl1[1] == bl0[1]
    again = tm.branch_support(n_replicates=100, seed=7, full=True)
    assert np.array_equal(again[0], quartets) and np.array_equal(again[1], scores)
    assert all(np.array_equal(again[2][f], sup[f]) for f in support.FIELDS)
    assert np.array_equal(again[3], rell)
    tail = tm.branch_support(n_replicates=60, seed=7, first_replicate=40, full=True)
    assert np.array_equal(tail[3][:, 1:], rell[:, 41:]) and np.array_equal(tail[3][:, 0], rell[:, 0])
    assert all(np.array_equal(tail[2][f], sup[f]) for f in ("lrt", "alrt_chi2", "abayes"))
    w = np.asarray(tm.siteweights, dtype=np.float64)
    rq, rs, ref, W = SR.branch_support(oracle_mod, tips, tm.traversal, e, w, 100, seed=7)
    assert np.array_equal(rq, quartets)
    _compare_pass(got, ref, 100)


def test_compressed_patterns(oracle_mod):
    """Duplicated columns through the normal path (weights above 1) give the supports of the
    same alignment, column by column with unit weights, in the restatement."""
    m, rm = G.GTR(), G.rates_of(4)
    tree, names, st = make_problem(8, 150, m, rm.rates, seed=6)
    st = np.concatenate([st, st[:, :90], st[:, :40]], axis=1)  # 280 columns
    seqs = [(n, "".join("ACGT"[x] for x in row)) for n, row in zip(names, st)]
    tm = TreeModel(device=0)
    tm.set_alignment(seqs, A.DNA)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    w = np.asarray(tm.siteweights)
    assert w.max() >= 3 and w.sum() == 280 and len(w) < 280
    got = tm.branch_support(n_replicates=100, seed=7, full=True)
    tr = tm.traversal
    e = R.eigen(m, rm)
    # the restatement on the patterns with their weights: bit-exact W, so exact counts
    tips = {tr.names[n]: np.asarray(tm.alignment[i]) for n, i in tm.names.items()}
    _, _, ref, W = SR.branch_support(oracle_mod, tips, tr, e, w, 100, seed=7)
    _compare_pass(got, ref, 100)
    # and column by column with unit weights, the columns in pattern order: column c of a
    # replicate then falls to the pattern the prefix sums of w give it, so the counts are equal
    cols = np.repeat(np.arange(len(w)), w.astype(int))
    tips1 = {k: v[cols] for k, v in tips.items()}
    _, _, ref1, W1 = SR.branch_support(oracle_mod, tips1, tr, e, np.ones(280), 100, seed=7)
    assert np.array_equal(np.array([np.bincount(cols, u, len(w)) for u in W1]), W)
    _compare_pass(got, ref1, 100)


def _edge_split(tm, nod):
    """The split of the edge above node `nod`, as nni_reference.splits writes it."""
    node = {i: n for n, i in tm.traversal.node_dict.items()}[int(nod)]
    side = frozenset(x.label for x in node.leaves())
    every = frozenset(tm.names)
    return every - side if min(every) in side else side


def test_meaning():
    m, rm, tree, start, names, codes = G._search_problem()
    tm = G._tm(tree, names, codes, np.eye(4), m, rm)
    tm.optimise_branch_lengths()
    quartets, scores, sup = tm.branch_support(n_replicates=100, seed=1)
    assert len(quartets) == 9 - 3
    assert (sup["abayes"] > 0.5).all() and (sup["sh_alrt"] > 0).all()
    assert (sup["lrt"] > 0).all() and (sup["alrt_chi2"] > 0).all()
    nod, par = internal_edges(tree)[2]
    tm = G._tm(apply_nni(tree, nod, par, 1), names, codes, np.eye(4), m, rm)
    tm.optimise_branch_lengths()
    quartets, scores, sup = tm.branch_support(n_replicates=100, seed=1)
    wrong = [i for i, q in enumerate(quartets) if _edge_split(tm, q[0]) not in R.splits(tree)]
    assert len(wrong) == 1  # the moved edge
    i = wrong[0]
    assert sup["lrt"][i] == 0.0 and sup["alrt_chi2"][i] == 0.0 and sup["sh_alrt"][i] == 0.0
    assert sup["abayes"][i] < 0.5


def test_refusals():
    kmax = N.lib().pu_quartet_max_cat(20)
    if kmax < 64:
        rm = GammaRateModel(kmax + 1, 0.8)
        m = SM.LG()
        tree, names, st = make_problem(6, 70, m, rm.rates, seed=3)
        tm = G._tm(tree, names, st.astype(np.uint8), np.eye(20), m, rm)
        lnl0 = tm.likelihood()
        with pytest.raises(N.PhyloHipError, match=r"\(-1\).*exceed the LDS"):
            tm.branch_support(n_replicates=10)
        inner = sorted(set(int(p) for p in tm.traversal.postorder_traversal[:, 0]))
        with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
            tm.quartet_site_lnl(inner[:4], G.LENS)
        assert tm.likelihood() == lnl0
    tm, tree, e, tips = G._setup("dna", 8, 70, 4, seed=1, keep=False)
    for call in (tm.branch_support, lambda: tm.quartet_site_lnl((8, 9, 10, 11), G.LENS)):
        with pytest.raises(ValueError, match="keep_partials"):
            call()
    tree, names, st = make_problem(8, 70, G.GTR(), [1.0], seed=1)
    tm = G._tm(tree, names, st.astype(np.uint8), np.eye(4), SM.Unrest(), UniformRateModel())
    with pytest.raises(ValueError, match="reversible"):
        tm.branch_support()
    tm, tree, e, tips = G._setup("dna", 8, 70, 1, seed=1)
    tm.set_ascertainment_bias_correction()
    with pytest.raises(ValueError, match="ascertainment"):
        tm.branch_support()
    tm, tree, e, tips = G._setup("dna", 8, 70, 4, seed=1)
    lnl0 = tm.likelihood()
    for kw in (dict(n_replicates=0), dict(epsilon=-1.0), dict(epsilon=float("nan")),
               dict(first_replicate=-1), dict(first_replicate=2 ** 32 - 5, n_replicates=10),
               dict(tol=0.0)):
        with pytest.raises(N.PhyloHipError, match=r"\(-1\)"):
            tm.branch_support(**kw)
        assert tm.likelihood() == lnl0
    # non-integer pattern weights
    m, rm = G.GTR(), G.rates_of(4)
    tree, names, st = make_problem(8, 70, m, rm.rates, seed=1)
    tm = TreeModel(device=0)
    tm.set_alignment_codes(st.astype(np.uint8), np.eye(4), names,
                           siteweights=np.linspace(0.5, 2.0, 70))
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    lnl0 = tm.likelihood()
    with pytest.raises(N.PhyloHipError, match=r"\(-1\).*not an integer"):
        tm.branch_support(n_replicates=10)
    assert tm.likelihood() == lnl0
    tm.compute_partials()
    assert tm.likelihood() == lnl0
    assert len(tm.nni_scores()[0]) == 8 - 3  # the context is still usable


def test_cli_support(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    spec = "HKY{2.0}+G4{0.7}"
    assert phy.main(["-s", fa, "-m", spec, "--nj", "nj", "--nni"]) == 0
    plain = capsys.readouterr().out
    out = tmp_path / "out.nwk"
    assert phy.main(["-s", fa, "-m", spec, "--nj", "nj", "--nni", "--support", "50", "-o",
                     str(out)]) == 0
    assert capsys.readouterr().out == plain and plain.startswith("lnL = ")
    t = prepare_tree(out.read_text())
    assert len(t.leaf_nodes()) == 9
    labels = [n.label for n in t.seed_node.postorder() if not n.is_leaf() and n.label is not None]
    assert len(labels) == 9 - 3
    for lab in labels:
        a, b = lab.split("/")
        assert 0.0 <= float(a) <= 100.0 and 0.0 <= float(b) <= 1.0
