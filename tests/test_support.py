"""Branch supports without a device: the CPU restatement on a hand-built case, the
tree labels and the CLI flag."""
import math

import numpy as np
import pytest

import support_reference as SR

from phylo_utils_amd import phy, support
from phylo_utils_amd.synthetic import make_problem
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.tree import Traversal, internal_edges, prepare_tree


def test_restatement_on_a_hand_built_case():
    inf = math.inf
    w = np.array([2, 1, 0, 3])
    # pattern 2 has weight 0 and sits at -inf under arrangement 0: it must not show
    s3 = np.array([[-1.0, -2.0, -inf, -1.5], [-1.25, -2.5, -9.0, -2.0], [-2.0, -2.0, -1.0, -1.75]])
    W = np.array([[2, 1, 0, 3],   # the weights themselves: every centred sum is 0
                  [6, 0, 0, 0],
                  [0, 0, 0, 6]], dtype=np.uint32)
    r = SR.supports(s3, w, W, epsilon=0.05)
    assert list(r["l"]) == [-8.5, -11.0, -11.25]
    assert r["B"][0].tolist() == r["l"].tolist() and r["gaps"][0] == 0.0
    assert r["B"][1].tolist() == [-6.0, -7.5, -12.0]
    assert r["d"] == 2.5 and r["lrt"] == 5.0
    # replicate 1: c = (2.5, 3.5, -0.75), gap 1.0; replicate 2: c = (-0.5, -1.0, 0.75), gap 1.25
    assert r["gaps"].tolist() == [0.0, 1.0, 1.25]
    assert r["count"] == 3 and r["sh_alrt"] == 1.0
    assert r["alrt_chi2"] == math.erf(math.sqrt(2.5))
    assert r["abayes"] == 1.0 / (1.0 + math.exp(-2.5) + math.exp(-2.75))
    assert SR.supports(s3, w, W, epsilon=2.0)["count"] == 1  # 2.5 > 0 + 2 only
    # a standing arrangement that loses: every support is exactly 0
    lost = SR.supports(s3[[1, 0, 2]], w, W)
    assert lost["d"] == -2.5
    assert lost["lrt"] == 0.0 and lost["alrt_chi2"] == 0.0 and lost["sh_alrt"] == 0.0
    assert 0.0 < lost["abayes"] < 0.5
    # l_0 at -inf (the pattern now has weight): all NaN; an alternative at -inf never wins
    w2 = np.array([2, 1, 1, 3])
    assert all(math.isnan(SR.supports(s3, w2, W)[f]) for f in support.FIELDS)
    alt = SR.supports(s3[[1, 0, 2]], w2, W)
    assert alt["l"][1] == -inf and math.isfinite(alt["d"]) and alt["d"] == -7.75
    assert alt["abayes"] == 1.0 / (1.0 + math.exp(alt["l"][2] - alt["l"][0]))


def test_label_tree_round_trips():
    tree, names, _ = make_problem(9, 10, SM.GTR(), [1.0], seed=11)
    t = prepare_tree(tree)
    edges = internal_edges(t)
    assert len(edges) == 9 - 3
    quartets = np.array([(n, p, 0, 0, 0, 0) for n, p in edges], dtype=np.int32)
    values = [(0.125 * i, 1.0 / (i + 1)) for i in range(len(edges))]
    lab = support.label_tree(t, quartets, values, lambda v: support.support_label(*v))
    assert all(n.label is None for n in t.seed_node.postorder() if not n.is_leaf())
    node = {i: n for n, i in Traversal(lab).node_dict.items()}
    want = {}
    for (nod, _), v in zip(edges, values):
        assert node[nod].label == "%.1f/%.3f" % (100 * v[0], v[1])
        side = frozenset(x.label for x in node[nod].leaves())
        want[min(side, frozenset(names) - side, key=sorted)] = node[nod].label
    back = prepare_tree(lab.as_newick())
    assert len(back.leaf_nodes()) == 9
    got = {}
    for n in back.seed_node.postorder():
        if n.is_leaf() or n.label is None:
            continue
        side = frozenset(x.label for x in n.leaves())
        got[min(side, frozenset(names) - side, key=sorted)] = n.label
        a, b = n.label.split("/")
        assert 0.0 <= float(a) <= 100.0 and 0.0 <= float(b) <= 1.0
    assert got == want
    with pytest.raises(ValueError):
        support.label_tree(t, quartets, values[:-1])


def test_cli_has_the_support_flag(capsys):
    with pytest.raises(SystemExit):
        phy.parse_cli(["--help"])
    assert "--support [R]" in capsys.readouterr().out
    args = phy.parse_cli(["-t", "x", "-s", "y", "--support"])
    assert args.support == 1000
    assert phy.parse_cli(["-t", "x", "-s", "y", "--support", "50"]).support == 50
    assert phy.parse_cli(["-t", "x", "-s", "y"]).support is None
    args = phy.parse_cli(["-t", "x", "-s", "y", "--support", "0"])
    with pytest.raises(ValueError, match="--support"):
        phy.validate_args(args)
