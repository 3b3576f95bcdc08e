"""phy --parsimony R --parsimony-spr on the GPU (phylo_utils_amd.phy): the printed
length and the written tree against the numpy restatement (tests/parsimony_spr_reference.py)."""
import numpy as np
import pytest

import parsimony_reference as PR
import parsimony_spr_reference as SR
from phylo_utils_amd import parsimony, phy
from phylo_utils_amd.tree import parse_newick
from test_cli_parsimony import _line, _uncompressed, sequences

pytestmark = pytest.mark.gpu


def test_cli_parsimony_spr(tmp_path, capsys):
    recs = sequences()
    fa, out = tmp_path / "aln.fasta", tmp_path / "out.nwk"
    fa.write_text("".join(">%s\n%s\n" % r for r in recs))
    assert phy.main(["-s", str(fa), "-m", "HKY85{2.0}", "--parsimony", "4", "--parsimony-spr",
                     "--seed", "1", "-o", str(out)]) == 0
    text = capsys.readouterr().out
    # the search on the compressed patterns is the search on the columns
    S, names = _uncompressed(recs)
    runs = [SR.search(PR.stepwise(S, o)["edges"], S)
            for o in parsimony.random_orders(len(names), 4, 1)]
    lengths = [r["length"] for r in runs]
    best = runs[lengths.index(min(lengths))]  # ties: the lowest replicate
    assert int(_line(text, "parsimony")) == best["length"]
    assert text.index("parsimony = ") < text.index("lnL = ")
    assert np.isfinite(float(_line(text, "lnL")))
    got = parse_newick(out.read_text())
    ops, root, _ = parsimony.tree_schedule(got, names)
    want = parsimony.tree_schedule(parsimony.edges_to_tree(best["edges"], names), names)
    assert np.array_equal(ops, want[0]) and np.array_equal(root, want[1])
    assert PR.lengths(PR.schedule_edges(ops, root), S) == best["length"]
    # a bound on the rounds and a radius reach the search
    assert phy.main(["-s", str(fa), "-m", "JC", "--parsimony", "4", "--parsimony-spr", "1",
                     "--parsimony-radius", "1", "--seed", "1"]) == 0
    text = capsys.readouterr().out
    one = [SR.search(PR.stepwise(S, o)["edges"], S, radius=1, max_rounds=1)["length"]
           for o in parsimony.random_orders(len(names), 4, 1)]
    assert int(_line(text, "parsimony")) == min(one)


def test_cli_parsimony_spr_argument_errors(tmp_path, capsys):
    fa, nw = tmp_path / "aln.fasta", tmp_path / "t.nwk"
    fa.write_text("".join(">%s\n%s\n" % r for r in sequences()))
    nw.write_text("((a,b),(c,d),(e,(f,g)));\n")
    assert phy.main(["-s", str(fa), "--nj", "bionj", "--parsimony-spr"]) == 1
    assert "--parsimony-spr needs --parsimony" in capsys.readouterr().err
    assert phy.main(["-t", str(nw), "-s", str(fa), "--parsimony-spr", "2"]) == 1
    assert "--parsimony-spr needs --parsimony" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--parsimony", "2", "--parsimony-radius", "2"]) == 1
    assert "--parsimony-radius needs --parsimony-spr" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--parsimony", "2", "--parsimony-spr", "-1"]) == 1
    assert "--parsimony-spr" in capsys.readouterr().err
