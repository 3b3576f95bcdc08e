"""Host side of the NNI search (phylo_utils_amd.nni): the new C symbols, the
category limit, the tree moves, the move selection and the CLI's argument rules.  No device."""
import collections

import pytest

from nni_reference import splits

from phylo_utils_amd import TreeModel, nni, phy
from phylo_utils_amd import _native as N
from phylo_utils_amd.tree import (Traversal, apply_nni, apply_nni_moves, internal_edges,
                                  parse_newick, prepare_tree, select_moves)

SIX = "((a:0.11,b:0.12):0.05,((c:0.13,d:0.14):0.07,e:0.15):0.04,f:0.16);"
fs = lambda s: frozenset(s)


def test_symbols_exported_and_bound():
    lib = N.lib()
    for name in ("pu_quartet_max_cat", "pu_quartet_derivs", "pu_nni_sweep"):
        assert name in N.SIGNATURES
        assert getattr(lib, name).argtypes is not None
    for name in ("quartet_derivatives", "nni_scores", "nni_search"):
        assert callable(getattr(TreeModel, name))
    assert nni.apply_nni is apply_nni and nni.select_moves is select_moves


def test_quartet_max_cat():
    for K in (2, 4, 20):
        assert N.lib().pu_quartet_max_cat(K) >= 8
        assert nni.quartet_max_cat(K) == N.lib().pu_quartet_max_cat(K)
    assert N.lib().pu_quartet_max_cat(7) < 0
    with pytest.raises(ValueError):
        nni.quartet_max_cat(7)


def test_internal_edges_of_six_taxa():
    assert internal_edges(SIX) == [(2, 9), (7, 9), (5, 7)]
    tr = Traversal(prepare_tree(SIX))
    assert len(internal_edges(SIX)) == len(tr.names) - 3


def test_apply_nni_gives_the_expected_splits():
    base = {fs("cdef"), fs("cde"), fs("cd")}
    assert splits(SIX) == base
    expect = {
        (2, 9, 1): {fs("bf"), fs("cde"), fs("cd")},       # (a, cde | b, f)
        (2, 9, 2): {fs("bcde"), fs("cde"), fs("cd")},     # (a, f | b, cde)
        (7, 9, 1): {fs("cdef"), fs("cdf"), fs("cd")},     # (cd, f | e, ab)
        (7, 9, 2): {fs("cdef"), fs("ef"), fs("cd")},      # (cd, ab | e, f)
        (5, 7, 1): {fs("cdef"), fs("cde"), fs("ce")},     # (c, e | d, rest)
        (5, 7, 2): {fs("cdef"), fs("cde"), fs("de")},     # (c, rest | d, e)
    }
    for (nod, par, which), want in expect.items():
        got = splits(apply_nni(SIX, nod, par, which))
        assert got == want, (nod, par, which)
        assert len(got ^ base) == 2  # exactly one split exchanged
    assert splits(SIX) == base  # the input is not changed


def _edge_lengths(tree):
    """{split or leaf label: length} of the unrooted tree."""
    t = prepare_tree(tree)
    tr = Traversal(t)
    leaves = fs(tr.names)
    first = min(leaves)
    below, out = {}, {}
    for n in t.seed_node.postorder():
        below[n] = fs([n.label]) if n.is_leaf() else frozenset().union(*(below[c]
                                                                         for c in n.children))
    for n, i in tr.node_dict.items():
        nb = [c for c in t.seed_node.children if c is not n][0] if n.parent is t.seed_node \
            else n.parent
        key = n.label if n.is_leaf() else (leaves - below[n] if first in below[n] else below[n])
        out[key] = tr.brlens[i, tr.node_dict[nb]]
    return out


def _edge_with_split(tree, split):
    """(NOD, PAR) of the internal edge of `tree` that carries `split`."""
    t = prepare_tree(tree)
    tr = Traversal(t)
    leaves = fs(tr.names)
    for nod, par in internal_edges(t):
        node = next(n for n, i in tr.node_dict.items() if i == nod)
        s = fs(x.label for x in node.leaves())
        if s == split or leaves - s == split:
            return nod, par
    raise AssertionError(split)


@pytest.mark.parametrize("which", [1, 2])
def test_apply_nni_inverse_restores_splits_and_lengths(which):
    base, lens = splits(SIX), _edge_lengths(SIX)
    for nod, par in internal_edges(SIX):
        moved = apply_nni(SIX, nod, par, which)
        (new,) = splits(moved) - base
        back = apply_nni(moved, *_edge_with_split(moved, new), which)
        assert splits(back) == base
        got = _edge_lengths(back)
        assert got.keys() == lens.keys()
        assert all(abs(got[k] - lens[k]) <= 1e-15 for k in lens), (nod, par)


def test_apply_nni_keeps_leaves_and_pendant_lengths():
    pend = lambda t: collections.Counter(round(v, 12) for k, v in _edge_lengths(t).items()
                                         if isinstance(k, str))
    every = lambda t: collections.Counter(round(v, 12) for v in _edge_lengths(t).values())
    for nod, par in internal_edges(SIX):
        for which in (1, 2):
            t = apply_nni(SIX, nod, par, which)
            assert sorted(n.label for n in t.leaf_nodes()) == list("abcdef")
            assert pend(t) == pend(SIX)
            assert every(t) == every(SIX)  # the central length too, unless replaced
            t2 = apply_nni(SIX, nod, par, which, length=0.5)
            assert pend(t2) == pend(SIX)
            (new,) = splits(t2) - splits(SIX)
            assert _edge_lengths(t2)[new] == 0.5
            assert sum(every(t2).values()) == sum(every(SIX).values())
    with pytest.raises(ValueError):
        apply_nni(SIX, 0, 2, 1)  # a pendant edge
    with pytest.raises(ValueError):
        apply_nni(SIX, 5, 7, 3)
    with pytest.raises(ValueError):
        apply_nni(SIX, 7, 5, 1)  # NOD must be the child end
    with pytest.raises(ValueError):
        apply_nni_moves(SIX, [(7, 9, 1, None), (5, 7, 1, None)])  # share node 7


def test_apply_two_moves_at_once_equals_one_after_the_other():
    both = apply_nni_moves(SIX, [(2, 9, 1, 0.3), (5, 7, 2, 0.2)])
    one = apply_nni(SIX, 2, 9, 1, 0.3)
    two = apply_nni(one, *_edge_with_split(one, fs("cd")), 2, 0.2)
    assert splits(both) == splits(two) == {fs("bf"), fs("cde"), fs("de")}
    assert _edge_lengths(both) == _edge_lengths(two)


def test_select_moves_order_ties_and_exclusion():
    c = lambda nod, par, gain: dict(nod=nod, par=par, which=1, gain=gain, t=0.1)
    cands = [c(5, 7, 2.0), c(7, 9, 3.0), c(12, 11, 3.0), c(2, 9, 1.0), c(20, 21, 0.5),
             c(21, 30, 0.7)]
    got = [(m["nod"], m["par"]) for m in select_moves(cands)]
    # 3.0 twice: (7, 9) before (11, 12) by the sorted pair; (5, 7) and (2, 9) share a node with
    # (7, 9); (21, 30) beats (20, 21), which shares node 21 with it
    assert got == [(7, 9), (12, 11), (21, 30)]
    assert select_moves([]) == []
    assert [m["gain"] for m in select_moves(cands[::-1])] == [3.0, 3.0, 0.7]


def test_candidates_take_the_better_alternative_above_min_gain():
    import numpy as np
    q = np.array([[5, 7, 0, 1, 2, 3], [7, 9, 5, 6, 8, 2]], dtype=np.int32)
    s = np.zeros((2, 3, 4))
    s[0, :, 1] = (-100.0, -99.0, -98.5)
    s[0, :, 0] = (0.1, 0.2, 0.3)
    s[1, :, 1] = (-100.0, -99.9995, -101.0)
    got = nni.candidates(q, s, -100.0, 1e-3)
    assert got == [dict(nod=5, par=7, which=2, gain=1.5, t=0.3)]


def test_cli_nni_validation(tmp_path, capsys):
    t = tmp_path / "t.nwk"
    t.write_text(SIX)
    fa = tmp_path / "a.fa"
    fa.write_text("".join(">%s\nACGT\n" % n for n in "abcdef"))
    assert phy.parse_cli(["-t", str(t), "-s", str(fa)]).nni is None
    assert phy.parse_cli(["-t", str(t), "-s", str(fa), "--nni"]).nni == 50
    assert phy.parse_cli(["-t", str(t), "-s", str(fa), "--nni", "3"]).nni == 3
    phy.validate_args(phy.parse_cli(["-t", str(t), "-s", str(fa), "--nni"]))
    phy.validate_args(phy.parse_cli(["-s", str(fa), "--nj", "nj", "--nni", "2"]))
    assert phy.main(["-t", str(t), "--simulate", "10", "--nni"]) == 1
    assert "--nni excludes" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--distances", "--nni"]) == 1
    assert "--nni excludes" in capsys.readouterr().err
    assert phy.main(["-t", str(t), "-s", str(fa), "--nni", "-1"]) == 1
    assert "non-negative" in capsys.readouterr().err


def test_search_refuses_what_it_cannot_do():
    tm = TreeModel(keep_partials=False)
    with pytest.raises(ValueError, match="keep_partials"):
        tm.nni_search()
    with pytest.raises(ValueError, match="keep_partials"):
        tm.nni_scores()
    tm = TreeModel()
    tm.substitution_model = type("M", (), {"reversible": True})()
    tm.set_alignment_codes([[0, 1], [1, 0], [0, 0]], [[1.0, 0.0], [0.0, 1.0]], "abc")
    with pytest.raises(ValueError, match="4 taxa"):
        tm.nni_search()
