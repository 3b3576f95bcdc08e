"""phy --parsimony / --parsimony-score on the GPU (phylo_utils_amd.phy): the
starting tree and the printed length against the numpy restatement (tests/parsimony_reference.py)."""
import numpy as np
import pytest

import parsimony_reference as PR
from phylo_utils_amd import alignment as A
from phylo_utils_amd import parsimony, phy
from phylo_utils_amd.tree import parse_newick

pytestmark = pytest.mark.gpu

NEWICK = "((a:0.1,b:0.2):0.05,(c:0.1,d:0.3):0.1,(e:0.2,(f:0.1,g:0.1):0.1):0.2);"


def sequences():
    rng = np.random.default_rng(8)
    n, S = 7, 300
    base = rng.integers(4, size=S)
    rows = np.where(rng.random((n, S)) < 0.3, rng.integers(4, size=(n, S)), base[None])
    chars = np.array(list("ACGT"))[rows]
    amb = rng.random((n, S)) < 0.03
    chars[amb] = rng.choice(list("-NR"), size=int(amb.sum()))
    return [(name, "".join(row)) for name, row in zip("abcdefg", chars)]


def _line(text, key):
    (line,) = [x for x in text.splitlines() if x.startswith(key + " = ")]
    return line.split("=")[1].strip()


def _uncompressed(recs):
    codes, table, names = A.char_codes(recs, A.DNA)
    return PR.tip_sets(codes, table), sorted(names, key=names.get)


def test_cli_parsimony_tree(tmp_path, capsys):
    recs = sequences()
    fa, out = tmp_path / "aln.fasta", tmp_path / "out.nwk"
    fa.write_text("".join(">%s\n%s\n" % r for r in recs))
    assert phy.main(["-s", str(fa), "-m", "HKY85{2.0}", "--parsimony", "3", "--seed", "1",
                     "-o", str(out)]) == 0
    text = capsys.readouterr().out
    # stepwise addition on the compressed patterns is stepwise addition on the columns
    S, names = _uncompressed(recs)
    runs = [PR.stepwise(S, o) for o in parsimony.random_orders(len(names), 3, 1)]
    lengths = [r["length"] for r in runs]
    best = runs[lengths.index(min(lengths))]
    assert int(_line(text, "parsimony")) == best["length"]
    assert text.index("parsimony = ") < text.index("lnL = ")
    assert np.isfinite(float(_line(text, "lnL")))
    got = parse_newick(out.read_text())
    ops, root, _ = parsimony.tree_schedule(got, names)
    want = parsimony.tree_schedule(parsimony.edges_to_tree(best["edges"], names), names)
    assert np.array_equal(ops, want[0]) and np.array_equal(root, want[1])
    assert PR.lengths(PR.schedule_edges(ops, root), S) == best["length"]


def test_cli_parsimony_score(tmp_path, capsys):
    recs = sequences()
    fa, nw = tmp_path / "aln.fasta", tmp_path / "t.nwk"
    fa.write_text("".join(">%s\n%s\n" % r for r in recs))
    nw.write_text(NEWICK + "\n")
    assert phy.main(["-t", str(nw), "-s", str(fa), "-m", "JC"]) == 0
    plain = capsys.readouterr().out
    assert "parsimony" not in plain
    assert phy.main(["-t", str(nw), "-s", str(fa), "-m", "JC", "--parsimony-score"]) == 0
    text = capsys.readouterr().out
    S, names = _uncompressed(recs)
    edges = PR.schedule_edges(*parsimony.tree_schedule(NEWICK, names)[:2])
    assert int(_line(text, "parsimony")) == PR.lengths(edges, S)
    assert _line(text, "lnL") == _line(plain, "lnL")  # nothing else changes


def test_cli_parsimony_argument_errors(tmp_path, capsys):
    fa, nw = tmp_path / "aln.fasta", tmp_path / "t.nwk"
    fa.write_text("".join(">%s\n%s\n" % r for r in sequences()))
    nw.write_text(NEWICK + "\n")
    assert phy.main(["-t", str(nw), "-s", str(fa), "--parsimony"]) == 1
    assert "--parsimony excludes" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--nj", "bionj", "--parsimony", "2"]) == 1
    assert "--parsimony excludes" in capsys.readouterr().err
