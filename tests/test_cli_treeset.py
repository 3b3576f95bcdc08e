"""phy CLI on tree sets: --bootstrap R --consensus FILE and --compare-trees FILE, on the small
alignment tests/test_cli.py uses."""
import io
import re

import numpy as np
import pytest

from phylo_utils_amd import phy, treeset
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.tree import parse_newick

MODEL = "GTR{1.0,2.0,3.0,4.0,5.0,6.0}+F{0.1,0.2,0.3,0.4}+G4{0.7}"


def write_case(tmp_path, seed=3):
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem
    m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    rm = GammaRateModel(4, 0.7)
    tree, names, st = make_problem(9, 240, m, rm.rates, seed=seed)
    seqs = ["".join("ACGT"[x] for x in row) for row in st]
    seqs[0] = "N-R" + seqs[0][3:]  # ambiguity codes and gaps
    fa = tmp_path / "aln.fasta"
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)))
    nw = tmp_path / "tree.nwk"
    nw.write_text(tree.as_newick())
    return str(nw), str(fa), tree, list(names)


def test_cli_validation(tmp_path, capsys):
    nw, fa, _, _ = write_case(tmp_path)
    assert phy.main(["-s", fa, "--nj", "nj", "--consensus", str(tmp_path / "c.nwk")]) == 1
    assert "--consensus needs --bootstrap" in capsys.readouterr().err
    assert phy.main(["-s", fa, "--nj", "nj", "--bootstrap", "5", "--consensus",
                     str(tmp_path / "c.nwk"), "--consensus-threshold", "0.3"]) == 1
    assert "[0.5, 1]" in capsys.readouterr().err
    assert phy.main(["-t", nw, "-s", fa, "--compare-trees", str(tmp_path / "none.nwk")]) == 1
    assert "does not exist" in capsys.readouterr().err


@pytest.mark.gpu
def test_cli_bootstrap_consensus(tmp_path):
    _, fa, _, names = write_case(tmp_path)
    cons = tmp_path / "consensus.nwk"
    out = io.StringIO()
    args = phy.parse_cli(["-s", fa, "-m", MODEL, "--nj", "bionj", "--bootstrap", "20",
                          "--consensus", str(cons), "--seed", "4"])
    phy.validate_args(args)
    phy.run(args, out)
    assert out.getvalue().startswith("lnL = ")
    text = cons.read_text().strip()
    tree = parse_newick(text)
    assert sorted(x.label for x in tree.leaf_nodes()) == sorted(names)
    assert ":" not in text  # no branch lengths
    labels = [x.label for x in tree.seed_node.postorder()
              if x.children and x is not tree.seed_node]
    assert labels and len(labels) <= len(names) - 3
    for lab in labels:
        assert re.fullmatch(r"\d+", lab) and 51 <= int(lab) <= 100
    # the strict consensus holds no more splits, all at 100
    args = phy.parse_cli(["-s", fa, "-m", MODEL, "--nj", "bionj", "--bootstrap", "20",
                          "--consensus", str(cons), "--consensus-threshold", "1.0", "--seed", "4"])
    phy.validate_args(args)
    phy.run(args, io.StringIO())
    strict = parse_newick(cons.read_text())
    sl = [x.label for x in strict.seed_node.postorder()
          if x.children and x is not strict.seed_node]
    assert len(sl) <= len(labels) and all(lab == "100" for lab in sl)


@pytest.mark.gpu
def test_cli_compare_trees(tmp_path):
    nw, fa, tree, names = write_case(tmp_path)
    other = "((t0,t3),(t1,(t2,t4)),((t5,t6),(t7,t8)));"
    if sorted(names) != ["t%d" % i for i in range(9)]:
        pytest.fail("the case's names changed: %r" % names)
    listed = [tree.as_newick(), other, other]
    cand = tmp_path / "cand.nwk"
    cand.write_text("\n".join(listed) + "\n")
    out = io.StringIO()
    args = phy.parse_cli(["-t", nw, "-s", fa, "-m", MODEL, "--compare-trees", str(cand)])
    phy.validate_args(args)
    phy.run(args, out)
    lines = out.getvalue().strip().split("\n")
    assert lines[0].startswith("lnL = ")
    rf = np.array([[int(x) for x in re.fullmatch(r"rf %d: ([\d ]+)" % i, lines[1 + i]).group(1).split()]
                   for i in range(4)])
    want = treeset.rf_distances([tree] + listed, sorted(names))
    assert np.array_equal(rf, want)
    assert rf[0, 1] == 0 and rf[2, 3] == 0 and rf[0, 2] > 0
    k = len(set(tuple(row) for row in (want == 0)))
    assert k == 2 and lines[5] == "topologies = 2 distinct of 4" and len(lines) == 6
