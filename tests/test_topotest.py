"""Topology tests without a device: the AU fit of ``topotest.au_pvalue`` on exact
synthetic proportions, the CPU restatement (tests/topotest_reference.py) on hand-built and
simulated cases, the host finish on restated counts, the table and the CLI flags."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import nni_reference as NR
import topotest_reference as TR

from phylo_utils_amd import phy, topotest
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem, random_tree
from phylo_utils_amd.tree import Traversal, apply_nni, internal_edges, prepare_tree

ND = NormalDist()


def test_default_scales():
    assert list(topotest.DEFAULT_SCALES) == TR.DEFAULT_SCALES
    assert TR.n_draws(1000, TR.DEFAULT_SCALES).tolist() == [1000] + list(range(500, 1500, 100))
    assert TR.n_draws(7, [0.5, 0.08, 1.5]).tolist() == [7, 4, 1, 11]  # 3.5 + 0.5, 0.56 + 0.5, 11.0


@pytest.mark.parametrize("d,c", [(0.0, 0.5), (1.0, 0.3), (-0.7, 0.2), (2.0, 1.0), (1.5, -0.4),
                                 (0.3, 0.0)])
def test_au_fit_is_exact_on_exact_proportions(d, c):
    """bp_k = Phi(-(d sqrt(rho_k) + c / sqrt(rho_k))) lies on the model, so the weighted fit
    returns (d, c) whatever the weights are; 1e-9 leaves room for the rounding of the inverse
    normal alone.  Measured here: at most 8e-15 on d, c and p."""
    rho = np.array(topotest.DEFAULT_SCALES)
    bp = np.array([ND.cdf(-(d * math.sqrt(r) + c / math.sqrt(r))) for r in rho])
    p, dd, cc, n = topotest.au_pvalue(bp, rho, 10000)
    print("d %.3g c %.3g: errors %.2e %.2e %.2e" % (d, c, abs(dd - d), abs(cc - c),
                                                   abs(p - (1.0 - ND.cdf(d - c)))))
    assert n == 10
    assert abs(dd - d) <= 1e-9 and abs(cc - c) <= 1e-9
    assert abs(p - (1.0 - ND.cdf(d - c))) <= 1e-9
    rp, rd, rc, rn = TR.au(bp, rho, 10000, bp[5])
    assert rn == 10 and abs(rd - d) <= 1e-9 and abs(rc - c) <= 1e-9 and abs(rp - p) <= 1e-9
    # realised scales that are not the nominal ones, and a subset of them
    rho2 = TR.n_draws(137, rho)[1:] / 137.0
    bp2 = np.array([ND.cdf(-(d * math.sqrt(r) + c / math.sqrt(r))) for r in rho2])
    p2, d2, c2, n2 = topotest.au_pvalue(bp2[::3], rho2[::3], 500)
    assert n2 == 4 and abs(d2 - d) <= 1e-9 and abs(c2 - c) <= 1e-9


def test_au_degenerate_scales():
    rho = np.array(topotest.DEFAULT_SCALES)
    nan = math.isnan
    # every count 0, every count R
    p, d, c, n = topotest.au_pvalue(np.zeros(10), rho, 100, bp0=0.0)
    assert (p, n) == (0.0, 0) and nan(d) and nan(c)
    p, d, c, n = topotest.au_pvalue(np.ones(10), rho, 100, bp0=1.0)
    assert (p, n) == (1.0, 0) and nan(d) and nan(c)
    # one usable scale: block 0 decides, and an interior block-0 count gives NaN
    bp = np.zeros(10)
    bp[0] = 0.01
    assert topotest.au_pvalue(bp, rho, 100, bp0=0.0)[::3] == (0.0, 1)
    assert topotest.au_pvalue(1.0 - bp, rho, 100, bp0=1.0)[::3] == (1.0, 1)
    assert nan(topotest.au_pvalue(bp, rho, 100, bp0=0.02)[0])
    # without bp0 the scale nearest 1 stands in for block 0
    assert topotest.au_pvalue(bp, rho, 100)[0] == 0.0
    # the dropped scales do not enter the fit: the rest still gives (d, c) exactly
    dd, cc = 1.0, 0.3
    bp = np.array([ND.cdf(-(dd * math.sqrt(r) + cc / math.sqrt(r))) for r in rho])
    bp[[0, 9]] = (1.0, 0.0)
    p, d, c, n = topotest.au_pvalue(bp, rho, 100)
    assert n == 8 and abs(d - dd) <= 1e-9 and abs(c - cc) <= 1e-9
    # no scales at all (--no-au), and two usable proportions at one and the same scale
    assert nan(topotest.au_pvalue([], [], 100, bp0=0.5)[0])
    assert topotest.au_pvalue([], [], 100, bp0=1.0)[0] == 1.0
    assert nan(topotest.au_pvalue([0.3, 0.4], [1.0, 1.0], 100, bp0=0.3)[0])
    for args in ((np.zeros(10), rho, 100, 0.0), (bp, rho, 100, bp[5])):
        got, ref = topotest.au_pvalue(*args[:3], bp0=args[3]), TR.au(*args)
        assert got[3] == ref[3] and (got[0] == ref[0] or abs(got[0] - ref[0]) <= 1e-9)


def test_scaled_weights_restatement():
    w = np.array([3, 0, 1, 5, 0, 2])
    N = int(w.sum())
    full = TR.scaled_weights(w, N, 4, seed=9, first_rep=2)
    assert np.array_equal(full, TR.BR.weights(w, 4, 9, 2))
    for n in (1, 5, 17):
        W = TR.scaled_weights(w, n, 4, seed=9, first_rep=2)
        assert (W.sum(axis=1) == n).all() and not W[:, [1, 4]].any()
        if n < N:  # the first n columns of the full row's draws
            assert (W <= full).all()
    rows = TR.scaled_weights(w, [5, 17, 11, 1], 4, seed=9, first_rep=2)
    assert np.array_equal(rows[1], TR.scaled_weights(w, 17, 1, seed=9, first_rep=3)[0])
    assert rows.sum(axis=1).tolist() == [5, 17, 11, 1]
    W, n = TR.block_weights(w, 3, [0.5, 2.0], seed=9, first_rep=2)
    assert n.tolist() == [11, 6, 22] and W.sum(axis=1).tolist() == [11] * 3 + [6] * 3 + [22] * 3
    assert np.array_equal(W[:3], TR.BR.weights(w, 3, 9, 2))
    assert np.array_equal(W[3:6], TR.scaled_weights(w, 6, 3, seed=9, first_rep=5))


def test_counts_on_a_hand_built_case():
    inf = math.inf
    lnl = np.array([-10.0, -12.0, -inf, -10.5])
    # c = B - l:   tree 0      1      (2)     3
    B = np.array([[-10.0, -12.0, -1.0, -10.5],    # c = 0, 0, 0: the weights themselves
                  [-11.0, -10.0, -1.0, -10.75],   # c = -1, 2, -0.25
                  [-9.0, -13.0, -1.0, -9.0],      # c = 1, -1, 1.5; B ties 0 and 3: the lowest
                  [-20.0, -20.0, -1.0, -30.0]])   # a scaled block's only row
    cnt = TR.counts(B[:3], lnl, 3)
    assert cnt.shape == (1, 3, 4)
    assert cnt[0, 0].tolist() == [2, 1, 0, 0]
    # KH: tree 0 against u* = 3 (d = -0.5): c_3 - c_0 = 0, 0.75, 0.5, all >= -0.5
    #     tree 1 against 0 (d = 2): 0, -3, 2;  tree 3 against 0 (d = 0.5): 0, -0.75, -0.5
    assert cnt[0, 1].tolist() == [3, 1, 0, 0]
    # SH: max c = 0, 2, 1.5; D = 0, 2, -, 0.5: tree 0: 0, 3, 0.5; tree 1: 0, 0, 2.5; tree 3: 0,
    # 2.25, 0
    assert cnt[0, 2].tolist() == [3, 1, 0, 1]
    two = TR.counts(np.vstack([B[:3], B[3:], B[3:], B[3:]]), lnl, 3)
    assert two.shape == (2, 3, 4) and np.array_equal(two[0], cnt[0])
    assert two[1].tolist() == [[3, 0, 0, 0], [0] * 4, [0] * 4]
    # one included tree: it wins everything and no test rejects it; none: all zero
    one = TR.counts(B[:3], np.array([-inf, -12.0, math.nan, -inf]), 3)
    assert one[0].tolist() == [[0, 3, 0, 0]] * 3
    assert not TR.counts(B[:3], np.full(4, -inf), 3).any()


def test_identical_trees():
    rng = np.random.default_rng(2)
    row = -rng.gamma(2.0, 3.0, 120)
    w = rng.integers(0, 4, 120)
    res = TR.topology_tests(np.stack([row] * 4), w, 50, scales=[0.5, 1.5], seed=3)
    assert res["bp"].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert res["p_kh"].tolist() == [1.0] * 4 and res["p_sh"].tolist() == [1.0] * 4
    assert np.allclose(res["c_elw"], 0.25, rtol=0, atol=1e-15)
    assert res["p_au"].tolist() == [1.0, 0.0, 0.0, 0.0]  # counts R and 0 at every scale
    assert res["counts"][1:, 0].tolist() == [[50, 0, 0, 0]] * 2


def _site_lnl(orc, tree, names, st, m, rm):
    tr = Traversal(prepare_tree(tree))
    e = NR.eigen(m, rm)
    eye = np.eye(len(m.freqs))
    tips = {tr.names[n]: eye[st[i]] for i, n in enumerate(names)}
    _, site = orc.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                           tr.root_length(), e["evecs"], e["evals"], e["ivecs"], e["freqs"],
                           e["rates"], e["weights"], n_nodes=tr.n_nodes)
    return np.asarray(site)


def test_meaning_on_a_simulated_alignment(oracle_mod):
    """8 taxa, 300 GTR+G4 sites down a known tree: that tree, its NNI neighbour across its
    shortest internal edge and a random topology, each with the lengths it comes with.  The data
    reject the random tree in every test and keep the generating tree in every test."""
    m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    tree, names, st = make_problem(8, 300, m, rm.rates, seed=3)
    true = prepare_tree(tree)
    tr = Traversal(true)
    nod, par = min(internal_edges(true), key=lambda e: tr.brlens[e])
    trees = [true, apply_nni(true, nod, par, 1), random_tree(np.random.default_rng(103), 8)]
    assert len({frozenset(NR.splits(t)) for t in trees}) == 3
    L = np.stack([_site_lnl(oracle_mod, t, names, st, m, rm) for t in trees])
    R = 400
    res = TR.topology_tests(L, np.ones(300), R, seed=1)
    print({f: res[f] for f in ("lnl", "bp", "p_kh", "p_sh", "c_elw", "p_au")})
    assert res["bp"][2] == 0.0 and res["p_sh"][2] < 0.05 and res["p_au"][2] < 0.05
    assert res["p_kh"][2] < 0.05 and res["c_elw"][2] < 1e-6
    assert res["p_kh"][0] > 0.05 and res["p_sh"][0] > 0.05 and res["p_au"][0] > 0.05
    assert res["bp"][0] > 0.5 and res["c_elw"][0] > 0.5
    assert abs(res["c_elw"].sum() - 1.0) <= 1e-12 and res["bp"].sum() == 1.0
    # the host finish of the package on the restated counts and sums: the same numbers
    raw = dict(counts=res["counts"], lnl=res["lnl"], n_draw=res["n_draw"], rell=res["B"])
    fin = topotest.finish(raw, R)
    for f in ("bp", "p_kh", "p_sh"):
        assert np.array_equal(fin[f], res[f]), f
    assert np.allclose(fin["c_elw"], res["c_elw"], rtol=1e-12, atol=0)
    assert np.array_equal(fin["au_scales"], res["au_scales"])
    assert np.allclose(fin["p_au"], res["p_au"], rtol=0, atol=1e-9)
    assert np.allclose(fin["delta"], res["lnl"].max() - res["lnl"], rtol=0, atol=0)
    # the table: the random tree is rejected everywhere, the generating tree nowhere
    lines = topotest.format_table(fin)
    assert lines[0].startswith("#") and [x.split(":")[0] for x in lines[1:]] == \
        ["tree 0", "tree 1", "tree 2"]
    assert lines[1].split()[5::2] == ["+"] * 5 and lines[3].split()[5::2] == ["-"] * 5
    assert topotest.format_table(fin, au=False)[1].split()[-1] == "-"
    assert len(topotest.format_table(fin, au=False)[1].split()) == len(lines[1].split()) - 1


def test_finish_with_an_excluded_tree():
    lnl = np.array([-5.0, -math.inf, -6.0])
    B = np.array([[[-5.0, -1.0, -6.5]], [[-4.0, -1.0, -3.0]]])
    cnt = TR.counts(B.reshape(2, 3), lnl, 1)
    fin = topotest.finish(dict(counts=cnt, lnl=lnl, n_draw=np.array([10, 5]), rell=B), 1)
    assert fin["bp"].tolist() == [1.0, 0.0, 0.0] and fin["c_elw"][1] == 0.0
    assert fin["delta"].tolist() == [0.0, math.inf, 1.0]
    assert fin["p_au"].tolist() == [1.0, 0.0, 0.0]
    want = math.exp(-1.5) / (1.0 + math.exp(-1.5))
    assert abs(fin["c_elw"][2] - want) <= 1e-15
    assert topotest.confidence_set([0.5, 0.46, 0.04, 0.0]).tolist() == [True, True, False, False]


def test_python_refusals_need_no_device():
    with pytest.raises(ValueError, match="share S"):
        topotest.topology_counts(np.zeros((2, 5)), np.ones(4))
    with pytest.raises(ValueError, match="one n_draw per replicate"):
        topotest.scaled_bootstrap_weights(5, [3, 4], 3)
    with pytest.raises(ValueError, match="one scale per proportion"):
        topotest.au_pvalue([0.5], [1.0, 2.0], 10)

    class Stub(object):
        alignment, ascbias, _ctx = None, False, None
    with pytest.raises(ValueError, match="at least two trees"):
        topotest.topology_tests(Stub(), ["(a,b);"])
    with pytest.raises(ValueError, match="No alignment"):
        topotest.topology_tests(Stub(), ["(a,b);", "(a,b);"])


def test_cli_has_the_test_trees_flags(tmp_path, capsys):
    with pytest.raises(SystemExit):
        phy.parse_cli(["--help"])
    text = capsys.readouterr().out
    assert "--test-trees FILE" in text and "--test-replicates R" in text and "--no-au" in text
    args = phy.parse_cli(["-t", "x", "-s", "y", "--test-trees", "z"])
    assert args.test_trees == "z" and args.test_replicates == 10000 and not args.no_au
    assert phy.parse_cli(["-t", "x", "-s", "y"]).test_trees is None
    with pytest.raises(FileNotFoundError, match="does not exist"):
        phy.validate_args(args)
    cand = tmp_path / "cand.nwk"
    cand.write_text("(a,b,(c,d));\n")
    aln = tmp_path / "a.fasta"
    aln.write_text(">a\nAC\n>b\nAC\n>c\nAG\n>d\nAG\n")
    ok = phy.parse_cli(["-s", str(aln), "--test-trees", str(cand)])
    phy.validate_args(ok)  # no tree of the run's own: the candidates alone
    for extra, msg in ((["--test-replicates", "0"], "--test-replicates"),
                       (["--distances"], "--test-trees excludes"),
                       (["--ascertainment", "weighted"], "not implemented"),
                       (["--nni"], "--nni needs a tree"), (["--optimise", "2"], "needs a tree")):
        with pytest.raises(ValueError, match=msg):
            phy.validate_args(phy.parse_cli(["-s", str(aln), "--test-trees", str(cand)] + extra))
