"""Neighbour joining and BIONJ on the CPU: the ABI is exported and bound, every
refused argument is refused before a device is touched, the numpy restatement
(tests/nj_reference.py) recovers additive trees, joins_to_tree round-trips through Newick, and
the CLI's --nj argument rules."""
import ctypes

import numpy as np
import pytest

from conftest import has_gpu

import nj_reference as NR
from phylo_utils_amd import _native as N
from phylo_utils_amd import nj, phy
from phylo_utils_amd.synthetic import random_tree
from phylo_utils_amd.tree import parse_newick

NJ_SYMBOLS = ("pu_nj", "pu_nj_device", "pu_nj_max_lds_n", "pu_pair_matrix_device")


def test_symbols_exported_and_bound():
    lib = N.lib()
    for s in NJ_SYMBOLS:
        assert s in N.SIGNATURES, s
        assert hasattr(lib, s), s


def test_module_imports():
    import phylo_utils_amd
    assert phylo_utils_amd.nj is nj
    for f in ("nj_joins", "joins_to_tree", "neighbour_joining", "nj_device",
              "pair_matrix_device"):
        assert callable(getattr(nj, f))
    assert callable(phylo_utils_amd.TreeModel.set_nj_tree)


def test_tier_a_capacity():
    """The largest n of the one-workgroup kernel: the triangle(s) of n (n - 1) / 2 doubles, the
    row sums, 16 reduction slots and three integer lists within 160 KiB."""
    def fits(n, v):
        return ((1 + v) * (n * (n - 1) // 2 + n) + 16) * 8 + (3 * n + 16) * 4 <= 160 * 1024
    for name, v in (("nj", 0), ("bionj", 1)):
        m = nj.max_lds_n(name)
        assert fits(m, v) and not fits(m + 1, v)
    assert nj.max_lds_n("nj") == 200 and nj.max_lds_n("bionj") == 141
    assert N.lib().pu_nj_max_lds_n(2) == N.PU_E_ARG


# ------------------------------------------------------------------ refused arguments
def _valid(n=5, n_mat=2):
    return dict(device=0, method=0, n_mat=n_mat, n=n, D=np.ones((n_mat, n, n)),
                joins=np.zeros((n_mat, n - 2, 2), dtype=np.int32), lens=np.zeros((n_mat, n - 2, 2)),
                root=np.zeros((n_mat, 2), dtype=np.int32), root_len=np.zeros(n_mat),
                q=np.zeros((n_mat, n - 3)), ld=n)


def _call(a):
    return N.lib().pu_nj(a["device"], a["method"], a["n_mat"], a["n"], N.ptr(a["D"]),
                         N.ptr(a["joins"]), N.ptr(a["lens"]), N.ptr(a["root"]),
                         N.ptr(a["root_len"]), N.ptr(a["q"]))


def _call_device(a):
    """The _device form with made-up device addresses: refused before any is read."""
    fake = lambda k: None if a[k] is None else ctypes.c_void_p(0x1000)
    return N.lib().pu_nj_device(a["device"], None, a["method"], a["n_mat"], a["n"], fake("D"),
                                a["ld"], fake("joins"), fake("lens"), fake("root"),
                                fake("root_len"), fake("q"))


def _with(i, j, x):
    D = np.ones((2, 5, 5))
    D[1, i, j] = x
    return dict(D=D)


BAD = {
    "null D": dict(D=None), "null joins": dict(joins=None), "null lens": dict(lens=None),
    "null root": dict(root=None), "null root length": dict(root_len=None),
    "n = 2": dict(n=2), "n = 0": dict(n=0), "n above the cap": dict(n=8193),
    "no matrix": dict(n_mat=0), "negative count": dict(n_mat=-1),
    "method 2": dict(method=2), "method -1": dict(method=-1),
}
BAD_HOST = {
    "negative entry": _with(1, 3, -0.1), "nan entry": _with(0, 4, np.nan),
    "inf entry": _with(2, 3, np.inf),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_arguments_are_refused_without_a_device(name):
    a = dict(_valid(), **BAD[name])
    assert _call(a) == N.PU_E_ARG, name
    assert "pu_nj" in N.last_error()
    assert _call_device(a) == N.PU_E_ARG, name
    assert "pu_nj_device" in N.last_error()


@pytest.mark.parametrize("name", sorted(BAD_HOST))
def test_bad_entries_are_refused_by_the_host_form(name):
    a = dict(_valid(), **BAD_HOST[name])
    assert _call(a) == N.PU_E_ARG, name
    assert "matrix 1 entry" in N.last_error()


def test_row_stride_is_checked():
    a = dict(_valid(), ld=4)
    assert _call_device(a) == N.PU_E_ARG
    assert "row stride" in N.last_error()


def test_pair_matrix_refusals():
    fake = ctypes.c_void_p(0x1000)
    f = N.lib().pu_pair_matrix_device
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    assert f(0, None, 4, 6, None, None, fake, 4) == N.PU_E_ARG
    assert f(0, None, 4, 6, None, fake, None, 4) == N.PU_E_ARG
    assert f(0, None, 1, 0, None, fake, fake, 4) == N.PU_E_ARG
    assert f(0, None, 4, 5, None, fake, fake, 4) == N.PU_E_ARG   # not all pairs, no list
    assert f(0, None, 4, 6, None, fake, fake, 3) == N.PU_E_ARG   # ld < n
    for bad in ([[0, 4]], [[-1, 2]], [[2, 2]]):
        p = i32(bad)
        assert f(0, None, 4, 1, N.ptr(p), fake, fake, 4) == N.PU_E_ARG
        assert "pu_pair_matrix_device" in N.last_error()
    p = i32([[0, 1]])
    assert f(0, None, 4, 0, N.ptr(p), fake, fake, 4) == N.PU_E_ARG


def test_lower_triangle_and_diagonal_are_not_looked_at():
    """Only the upper triangle is read: garbage below it is not an argument error (the call
    then goes on to the device)."""
    a = _valid()
    a["D"][0][np.tril_indices(5)] = np.nan
    assert _call(a) != N.PU_E_ARG


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_valid_call_fails_loudly_without_a_device():
    a = _valid()
    rc = _call(a)
    assert rc != 0 and rc != N.PU_E_ARG
    with pytest.raises(N.PhyloHipError):
        nj.nj_joins(np.ones((4, 4)))
    with pytest.raises(N.PhyloHipError):
        nj.neighbour_joining(np.ones((4, 4)), list("abcd"))


def test_python_argument_checks():
    with pytest.raises(ValueError):
        nj.nj_joins(np.ones((4, 5)))
    with pytest.raises(ValueError):
        nj.nj_joins(np.ones(4))
    with pytest.raises(ValueError):
        nj.nj_joins(np.ones((4, 4)), method="upgma")
    with pytest.raises(ValueError):
        nj.neighbour_joining(np.ones((4, 4)), list("abc"))
    with pytest.raises(ValueError):
        nj.neighbour_joining(np.ones((1, 1)), ["a"])


def test_two_taxa_need_no_library():
    D = np.array([[0.0, 0.3], [0.3, 0.0]])
    t = nj.neighbour_joining(D, ["x", "y"])
    assert NR.split_lengths(t) == {frozenset(["y"]): 0.3}
    ts = nj.neighbour_joining(np.stack([D, 2 * D]), ["x", "y"], method="bionj")
    assert [NR.patristic(x, ["x", "y"])[0, 1] for x in ts] == [0.3, 0.6]
    assert nj.neighbour_joining(0 * D, ["x", "y"], min_length=1e-8).as_newick() == \
        "(x:1e-08,y:0.0);"


# ------------------------------------------------------------------ the restatement itself
def _tree_of(res, names, min_length=None):
    return nj.joins_to_tree(names, res["joins"], res["lens"], res["root"], res["root_len"],
                            min_length)


@pytest.mark.parametrize("n", [4, 5, 8, 33])
@pytest.mark.parametrize("method", ["nj", "bionj"])
def test_restatement_recovers_additive_trees(n, method):
    """On the patristic matrix of a tree both methods return that tree: RF = 0 and every branch
    within 1e-12 max D."""
    true = random_tree(np.random.default_rng(100 + n), n, 0.02, 0.3)
    names = ["t%d" % i for i in range(n)]
    D = NR.patristic(true, names)
    res = NR.nj(D, method)
    got = _tree_of(res, names)
    assert NR.robinson_foulds(got, true) == 0
    want, have = NR.split_lengths(true), NR.split_lengths(got)
    assert set(want) == set(have)
    tol = 1e-12 * D.max()
    for s in want:
        assert abs(want[s] - have[s]) <= tol, (sorted(s), want[s], have[s])
    np.testing.assert_allclose(NR.patristic(got, names), D, rtol=0, atol=4 * n * tol)
    # cluster ids: join m makes n + m from two live clusters, smaller id first
    seen = set()
    for m, (a, b) in enumerate(res["joins"]):
        assert 0 <= a < b < n + m and not {a, b} & seen
        seen |= {int(a), int(b)}
    assert res["root"][0] == 2 * n - 3 and set(range(2 * n - 2)) - seen == set(res["root"])


def test_restatement_three_taxa_and_ties():
    D = np.array([[0, 0.3, 0.5], [0.3, 0, 0.6], [0.5, 0.6, 0]])
    res = NR.nj(D)
    assert res["joins"].tolist() == [[0, 1]] and res["root"].tolist() == [3, 2]
    np.testing.assert_allclose(res["lens"], [[0.1, 0.2]], rtol=0, atol=1e-16)
    assert abs(res["root_len"] - 0.4) <= 1e-16
    # exact ties: the smallest (a, b) by id
    E = np.ones((6, 6)) - np.eye(6)
    for method in ("nj", "bionj"):
        res = NR.nj(E, method)
        assert res["joins"].tolist() == [[0, 1], [2, 3], [4, 5], [6, 7]]
        assert res["root"].tolist() == [9, 8]
        assert np.all(res["gap"] == 0.0)


def test_rf_and_patristic_helpers():
    a = parse_newick("((a:1,b:2):0.5,(c:1,d:1):0.25,e:3);")
    b = parse_newick("((a:1,c:2):0.5,(b:1,d:1):0.25,e:3);")
    assert NR.robinson_foulds(a, a) == 0 and NR.robinson_foulds(a, b) == 4
    P = NR.patristic(a, list("abcde"))
    assert P[0, 1] == 3.0 and P[0, 2] == 2.75 and P[3, 4] == 4.25 and P[2, 2] == 0.0
    # a rooted and an unrooted writing of one tree
    c = parse_newick("(((a:1,b:2):0.5,e:3):0.1,(c:1,d:1):0.15);")
    assert NR.robinson_foulds(a, c) == 0
    assert NR.split_lengths(c)[frozenset("cd")] == 0.25


def test_joins_to_tree_round_trips_through_newick():
    n = 9
    names = ["taxon %d" % i if i == 3 else "t%d" % i for i in range(n)]  # one quoted label
    D = NR.perturbed_additive(5, n)
    res = NR.nj(D, "bionj")
    tree = _tree_of(res, names)
    back = parse_newick(tree.as_newick())
    assert back.as_newick() == tree.as_newick()
    assert sorted(x.label for x in back.leaf_nodes()) == sorted(names)
    assert NR.robinson_foulds(tree, back) == 0
    assert NR.split_lengths(tree) == NR.split_lengths(back)
    # the raw lengths are kept, negative ones too; min_length raises them
    raw = sorted(x.length for x in tree.seed_node.postorder() if x.length is not None)
    assert sorted(list(res["lens"].ravel()) + [res["root_len"], 0.0]) == raw
    res["lens"][0, 0] = -0.25
    assert min(x.edge_length for x in _tree_of(res, names).leaf_nodes()) == -0.25
    clamped = _tree_of(res, names, 1e-8)
    lengths = [x.length for x in clamped.seed_node.postorder() if x.length is not None]
    assert min(lengths) == 0.0 and sorted(lengths)[1] >= 1e-8  # the root edge's second half
    # a TreeModel takes the tree as it is
    from phylo_utils_amd.tree import Traversal, prepare_tree
    tr = Traversal(prepare_tree(clamped))
    assert tr.n_nodes == 2 * n - 2 and set(tr.names) == set(names)
    with pytest.raises(ValueError):
        nj.joins_to_tree(names, res["joins"][:-1], res["lens"][:-1], res["root"], 0.1)
    bad = res["joins"].copy()
    bad[3] = bad[0]
    with pytest.raises(ValueError):
        nj.joins_to_tree(names, bad, res["lens"], res["root"], 0.1)


# ------------------------------------------------------------------ CLI
def test_cli_nj_argument_rules(tmp_path, capsys):
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n>c\nAGGA\n")
    nwk = tmp_path / "t.nwk"
    nwk.write_text("(a:0.1,b:0.1,c:0.1);")
    args = phy.parse_cli(["-s", str(fa), "--nj", "bionj", "-o", str(tmp_path / "o.nwk")])
    phy.validate_args(args)  # no -t needed
    assert args.nj == "bionj" and args.tree is None
    assert phy.parse_cli(["-s", str(fa)]).nj is None
    for extra in (["--distances"], ["--simulate", "10"], ["-t", str(nwk)]):
        assert phy.main(["-s", str(fa), "--nj", "nj"] + extra) == 1
        assert "--nj excludes" in capsys.readouterr().err
    assert phy.main(["--nj", "nj"]) == 1
    assert "Alignment file not specified" in capsys.readouterr().err
    assert phy.main(["--nj", "nj", "-s", str(tmp_path / "missing.fa")]) == 1
    assert "does not exist" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        phy.parse_cli(["-s", str(fa), "--nj", "upgma"])
    capsys.readouterr()
    # without --nj the tree is still required
    assert phy.main(["-s", str(fa)]) == 1
    assert "Tree file not specified" in capsys.readouterr().err
