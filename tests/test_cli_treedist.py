"""phy CLI on trees with branch lengths: --compare-trees FILE --tree-metric M, on the small
alignment tests/test_cli_treeset.py uses."""
import io
import re

import numpy as np
import pytest

from phylo_utils_amd import phy, treeset
from test_cli_treeset import MODEL, write_case

OTHER = "((t0:0.1,t3:0.2):0.05,(t1:0.1,(t2:0.3,t4:0.1):0.02):0.04,((t5:0.1,t6:0.1):0.03,(t7:0.2,t8:0.1):0.25):0.5);"


def test_cli_validation(tmp_path, capsys):
    nw, fa, _, _ = write_case(tmp_path)
    assert phy.main(["-t", nw, "-s", fa, "--tree-metric", "kf"]) == 1
    assert "--tree-metric needs --compare-trees" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        phy.parse_cli(["-t", nw, "-s", fa, "--compare-trees", nw, "--tree-metric", "rf"])
    capsys.readouterr()


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["wrf", "kf", "path", "wpath"])
def test_cli_tree_metric(tmp_path, metric):
    nw, fa, tree, names = write_case(tmp_path)
    listed = [tree.as_newick(), OTHER]
    cand = tmp_path / "cand.nwk"
    cand.write_text("\n".join(listed) + "\n")
    plain, out = io.StringIO(), io.StringIO()
    base = ["-t", nw, "-s", fa, "-m", MODEL, "--compare-trees", str(cand)]
    for argv, stream in ((base, plain), (base + ["--tree-metric", metric], out)):
        args = phy.parse_cli(argv)
        phy.validate_args(args)
        phy.run(args, stream)
    before, lines = plain.getvalue().strip().split("\n"), out.getvalue().strip().split("\n")
    # lnL, three rf lines, three metric lines, topologies: the rest is what it was
    assert len(before) == 5 and lines[:4] == before[:4] and lines[7] == before[4] and len(lines) == 8
    got = np.array([[float(x) for x in re.fullmatch(r"%s %d: (.+)" % (metric, i),
                                                    lines[4 + i]).group(1).split()]
                    for i in range(3)])
    want = treeset.distances([tree] + listed, metric, sorted(names))
    assert np.array_equal(got, want)
    assert got[0, 1] == 0.0 and got[0, 2] > 0.0 and np.array_equal(got, got.T)
