"""phy --ancestral / --site-rates on the GPU (phylo_utils_amd.phy)."""
import re

import pytest

from test_cli import _write_case

from phylo_utils_amd import alignment as A
from phylo_utils_amd import phy
from phylo_utils_amd.tree import parse_newick

pytestmark = pytest.mark.gpu

SPEC = "HKY{2.0}+G4{0.7}"


def test_cli_ancestral_and_site_rates(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC]) == 0
    plain = capsys.readouterr().out
    anc, tsv = tmp_path / "anc.fasta", tmp_path / "rates.tsv"
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--ancestral", str(anc), "--site-rates",
                     str(tsv)]) == 0
    # the existing output is what it was, and a run without the options still prints it
    assert capsys.readouterr().out == plain
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC]) == 0
    assert capsys.readouterr().out == plain
    n_cols = len(A.read_fasta(fa)[0][1])
    recs = A.read_fasta(str(anc))
    assert len(recs) == 9 - 2
    assert all(len(s) == n_cols and set(s) <= set("ACGT") for _, s in recs)
    tree = parse_newick((tmp_path / "anc.fasta.nwk").read_text())  # (as written: not derooted)
    labels = [n.label for n in tree.seed_node.postorder()
              if n.children and n is not tree.seed_node]
    assert sorted(labels) == sorted(name for name, _ in recs)
    assert all(re.fullmatch(r"N\d+", name) for name in labels)
    assert len(tree.leaf_nodes()) == 9
    lines = tsv.read_text().splitlines()
    assert lines[0].split("\t") == ["site", "mean_rate", "map_category"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == n_cols
    assert [int(r[0]) for r in rows] == list(range(1, n_cols + 1))
    assert all(float(r[1]) > 0 and 1 <= int(r[2]) <= 4 for r in rows)


def test_cli_ancestral_after_optimise(tmp_path, capsys):
    nw, fa, m, rm = _write_case(tmp_path)
    anc = tmp_path / "anc.fasta"
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--optimise", "1"]) == 0
    plain = capsys.readouterr().out
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--optimise", "1", "--ancestral",
                     str(anc)]) == 0
    assert capsys.readouterr().out == plain
    assert len(A.read_fasta(str(anc))) == 7
