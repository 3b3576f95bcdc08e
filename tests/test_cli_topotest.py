"""phy --test-trees on the GPU (phylo_utils_amd.phy): the table against
``topotest.topology_tests`` for the same seed."""
import numpy as np
import pytest

from test_cli import _write_case

from phylo_utils_amd import TreeModel, phy, topotest
from phylo_utils_amd import alignment as A
from phylo_utils_amd.synthetic import random_tree
from phylo_utils_amd.tree import apply_nni, internal_edges, parse_newick, prepare_tree

pytestmark = pytest.mark.gpu

SPEC = "HKY{2.0}+G4{0.7}"
COLUMNS = ("bp", "p_kh", "p_sh", "c_elw", "p_au")


def _candidates(tmp_path, nw):
    tree = prepare_tree(parse_newick(open(nw).read()))
    nod, par = internal_edges(tree)[1]
    trees = [apply_nni(tree, nod, par, 2), random_tree(np.random.default_rng(5), 9)]
    path = tmp_path / "cand.nwk"
    path.write_text("".join(t.as_newick() + "\n\n" for t in trees))  # blank lines are skipped
    return str(path), tree, trees


def _rows(text):
    return [x.split(":")[1].split() for x in text.splitlines() if x.startswith("tree ")]


def _model(nw, fa):
    tm = TreeModel(device=0)
    tm.set_tree(parse_newick(open(nw).read()))
    tm.set_alignment(A.read_fasta(fa), A.DNA)
    desc = phy.parse_model_string(SPEC)
    tm.set_rate_model(phy.build_rate_model(desc))
    tm.set_substitution_model(phy.build_model(desc))
    tm.initialise()
    return tm


def test_cli_test_trees(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    cand, tree, trees = _candidates(tmp_path, nw)
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC]) == 0
    plain = capsys.readouterr().out
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--test-trees", cand, "--test-replicates",
                     "300", "--seed", "4"]) == 0
    text = capsys.readouterr().out
    assert text.startswith(plain) and plain.startswith("lnL = ")  # nothing else changes
    rows = _rows(text)
    assert len(rows) == 3 and [x for x in text.splitlines() if x.startswith("#")]
    # tree 0 is the run's tree; the values are topology_tests' for the same seed
    tm = _model(nw, fa)
    res = tm.topology_tests([tm.tree] + trees, n_replicates=300, seed=4)
    best = int(np.argmax(res["lnl"]))
    for t, row in enumerate(rows):
        assert abs(float(row[0]) - res["lnl"][t]) <= 5.1e-5 and \
            abs(float(row[1]) - res["delta"][t]) <= 5.1e-5
        for i, f in enumerate(COLUMNS):
            assert abs(float(row[2 + 2 * i]) - res[f][t]) <= 5.1e-5, (t, f)
            assert row[3 + 2 * i] in "+-"
    # the random tree is out of every set; KH and SH cannot reject the best tree
    assert rows[2][3::2] == ["-"] * 5 and rows[best][5] == "+" and rows[best][7] == "+"
    assert rows == [x.split(":")[1].split() for x in topotest.format_table(res)[1:]]


def test_cli_no_au_and_candidates_alone(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    cand, tree, trees = _candidates(tmp_path, nw)
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--test-trees", cand, "--test-replicates",
                     "100", "--no-au"]) == 0
    rows = _rows(capsys.readouterr().out)
    assert len(rows) == 3 and all(r[-1] == "-" and len(r) == 11 for r in rows)
    tm = _model(nw, fa)
    res = tm.topology_tests([tm.tree] + trees, n_replicates=100, scales=())
    assert rows == [x.split(":")[1].split() for x in topotest.format_table(res, au=False)[1:]]
    # no tree of the run's own: the file's trees alone, and no lnL line
    assert phy.main(["-s", fa, "-m", SPEC, "--test-trees", cand, "--test-replicates", "100",
                     "--no-au"]) == 0
    text = capsys.readouterr().out
    assert "lnL = " not in text and len(_rows(text)) == 2
    # a single candidate cannot be tested
    one = tmp_path / "one.nwk"
    one.write_text(trees[0].as_newick() + "\n")
    assert phy.main(["-s", fa, "-m", SPEC, "--test-trees", str(one)]) == 1
    assert "at least two trees" in capsys.readouterr().err
