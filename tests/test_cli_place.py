"""phy --place / --jplace on the GPU (phylo_utils_amd.phy)."""
import json
import re

import pytest

from test_cli import _write_case

from phylo_utils_amd import alignment as A
from phylo_utils_amd import phy
from phylo_utils_amd.tree import Traversal, parse_newick, prepare_tree

pytestmark = pytest.mark.gpu

SPEC = "HKY{2.0}+G4{0.7}"


def test_cli_place_writes_a_jplace(tmp_path, capsys):
    nw, fa, _, _ = _write_case(tmp_path)
    recs = A.read_fasta(fa)
    copied = recs[4][0]  # a taxon without the ambiguity codes _write_case puts into the first
    queries = tmp_path / "queries.fasta"
    queries.write_text(">copy\n%s\n>gaps\n%s\n" % (recs[4][1], "-" * len(recs[4][1])))
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC]) == 0
    plain = capsys.readouterr().out
    out, trees = tmp_path / "out.jplace", tmp_path / "placed.nwk"
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--place", str(queries), "--keep", "3",
                     "--jplace", str(out), "--placed-trees", str(trees), "-o",
                     str(tmp_path / "o.nwk")]) == 0
    assert not (tmp_path / "o.nwk").exists()  # --place leaves -o to the other options
    assert capsys.readouterr().out == plain  # the lnL line is what it was
    doc = json.loads(out.read_text())
    assert doc["version"] == 3
    assert doc["fields"] == ["edge_num", "likelihood", "like_weight_ratio", "distal_length",
                             "pendant_length"]
    nums = [int(v) for v in re.findall(r"\{(\d+)\}", doc["tree"])]
    assert sorted(nums) == list(range(2 * 9 - 3))
    assert [e["n"] for e in doc["placements"]] == [["copy"], ["gaps"]]
    for entry in doc["placements"]:
        assert len(entry["p"]) == 3
        assert abs(sum(p[2] for p in entry["p"]) - 1) <= 1e-12
        assert all(a[1] >= b[1] for a, b in zip(entry["p"], entry["p"][1:]))
    # the tip copy's best edge is that tip's edge, on a pendant branch at the lower bound
    best = doc["placements"][0]["p"][0]
    (tip_edge,) = re.findall(r"[(,]%s:[0-9.eE+-]+\{(\d+)\}" % re.escape(copied), doc["tree"])
    assert best[0] == int(tip_edge)
    assert best[4] <= 1e-7
    # the all-gap query's likelihood is the tree's on every edge
    lnl = float(plain.split("=")[1])
    assert all(abs(p[1] - lnl) <= 1e-9 * abs(lnl) for p in doc["placements"][1]["p"])
    # --placed-trees: one tree per query, the query beside the copied tip
    lines = trees.read_text().splitlines()
    assert len(lines) == 2
    t = prepare_tree(parse_newick(lines[0]))
    assert sorted(Traversal(t).names) == sorted([n for n, _ in recs] + ["copy"])
    # the query and the copied tip are at distance t + pendant, through the new node only
    tr = Traversal(t)
    q, c = tr.names["copy"], tr.names[copied]
    (x,) = set(a + b - q for a, b in tr.brlens if q in (a, b)) & \
        set(a + b - c for a, b in tr.brlens if c in (a, b))
    assert tr.brlens[q, x] == best[4] and tr.brlens[c, x] == best[3]


def test_cli_place_argument_errors(tmp_path, capsys):
    nw, fa, _, _ = _write_case(tmp_path)
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--place", fa]) == 1
    assert "--jplace" in capsys.readouterr().err
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--placed-trees", fa]) == 1
    assert "--jplace" in capsys.readouterr().err
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--place", str(tmp_path / "none.fasta"),
                     "--jplace", str(tmp_path / "x.jplace")]) == 1
    short = tmp_path / "short.fasta"
    short.write_text(">q\nACGT\n")
    assert phy.main(["-t", nw, "-s", fa, "-m", SPEC, "--place", str(short), "--jplace",
                     str(tmp_path / "x.jplace")]) == 1
    assert "columns" in capsys.readouterr().err
