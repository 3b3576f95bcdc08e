"""phy --spr on the GPU (phylo_utils_amd.phy): the search fixture of
tests/test_gpu_spr.py (tests/spr_reference.py: 10 taxa x 2000 DNA sites down a tree G, the start
tree one far SPR move away) through the command line."""
import pytest

import spr_reference as R

from phylo_utils_amd import phy
from phylo_utils_amd.tree import parse_newick

pytestmark = pytest.mark.gpu

SPEC = "GTR+G4{0.5}"


def _lnl(text):
    (line,) = [x for x in text.splitlines() if x.startswith("lnL = ")]
    return float(line.split("=")[1])


def test_cli_spr_finds_the_generating_topology(tmp_path, capsys):
    sp = R.search_problem()
    states = R.simulated_on_host(sp)
    fa, nw, out = tmp_path / "aln.fasta", tmp_path / "start.nwk", tmp_path / "out.nwk"
    fa.write_text("".join(">%s\n%s\n" % (n, "".join("ACGT"[x] for x in row))
                          for n, row in sorted(states.items())))
    nw.write_text(sp["start"].as_newick() + "\n")
    assert phy.main(["-t", str(nw), "-s", str(fa), "-m", SPEC]) == 0
    plain = _lnl(capsys.readouterr().out)
    assert phy.main(["-t", str(nw), "-s", str(fa), "-m", SPEC, "--spr", "-o", str(out)]) == 0
    found = _lnl(capsys.readouterr().out)
    print("without --spr %.6f, with %.6f" % (plain, found))
    assert found >= plain
    got = parse_newick(out.read_text())
    assert R.splits(got) == R.splits(sp["G"]) != R.splits(sp["start"])
    # a radius that holds the move back finds it too; --nni first is accepted
    assert phy.main(["-t", str(nw), "-s", str(fa), "-m", SPEC, "--nni", "--spr", "3",
                     "--spr-radius", str(sp["move"][4] + 1), "-o", str(out)]) == 0
    assert _lnl(capsys.readouterr().out) >= plain
    assert R.splits(parse_newick(out.read_text())) == R.splits(sp["G"])


def test_cli_spr_argument_errors(tmp_path, capsys):
    nw, fa = tmp_path / "t.nwk", tmp_path / "a.fasta"
    nw.write_text("((a:0.1,b:0.1):0.1,(c:0.1,d:0.1):0.1,e:0.1);\n")
    fa.write_text("".join(">%s\nACGTACGT\n" % n for n in "abcde"))
    assert phy.main(["-t", str(nw), "-s", str(fa), "--spr-radius", "2"]) == 1
    assert "--spr" in capsys.readouterr().err
    assert phy.main(["-t", str(nw), "-s", str(fa), "--spr", "-1"]) == 1
    assert "non-negative" in capsys.readouterr().err
    assert phy.main(["-t", str(nw), "-s", str(fa), "--spr", "--spr-radius", "0"]) == 1
    assert "radius" in capsys.readouterr().err
    assert phy.main(["-t", str(nw), "-s", str(fa), "--spr", "--ascertainment", "weighted"]) == 1
    assert "ascertainment" in capsys.readouterr().err
