"""phy CLI on concordance factors: --scf [Q], --gcf FILE and --cf-table FILE, on the small
alignment tests/test_cli.py uses."""
import io
import re

import numpy as np
import pytest

from phylo_utils_amd import phy
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.tree import parse_newick

MODEL = "GTR{1.0,2.0,3.0,4.0,5.0,6.0}+F{0.1,0.2,0.3,0.4}+G4{0.7}"
OTHER = "((t0,t3),(t1,(t2,t4)),((t5,t6),(t7,t8)));"


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
    assert phy.main(["-t", nw, "-s", fa, "--cf-table", str(tmp_path / "cf.tsv")]) == 1
    assert "--cf-table needs --scf or --gcf" in capsys.readouterr().err
    assert phy.main(["-t", nw, "-s", fa, "--scf", "0"]) == 1
    assert "--scf needs at least one quartet" in capsys.readouterr().err
    assert phy.main(["-t", nw, "-s", fa, "--gcf", str(tmp_path / "none.nwk")]) == 1
    assert "does not exist" in capsys.readouterr().err
    assert phy.main(["-s", fa, "--distances", "--scf"]) == 1
    assert "exclude --simulate and --distances" in capsys.readouterr().err
    cand = tmp_path / "cand.nwk"
    cand.write_text(OTHER + "\n")
    assert phy.main(["-s", fa, "--test-trees", str(cand), "--scf"]) == 1
    assert "--scf needs a tree" in capsys.readouterr().err
    args = phy.parse_cli(["-t", nw, "-s", fa, "--scf"])
    assert args.scf == 100 and args.gcf is None and args.cf_table is None
    phy.validate_args(args)


def internal_labels(text):
    tree = parse_newick(text)
    return [x.label for x in tree.seed_node.postorder()
            if x.children and x is not tree.seed_node and x.label is not None]


def run(argv):
    out = io.StringIO()
    args = phy.parse_cli(argv)
    phy.validate_args(args)
    phy.run(args, out)
    return out.getvalue()


@pytest.mark.gpu
def test_cli_label_order_and_table(tmp_path):
    nw, fa, tree, names = write_case(tmp_path)
    genes = tmp_path / "genes.nwk"
    genes.write_text("\n".join([tree.as_newick(), OTHER, tree.as_newick()]) + "\n")
    base = ["-t", nw, "-s", fa, "-m", MODEL, "--seed", "4"]
    num = r"(\d+\.\d|NA)"

    # --support alone prints what it printed before
    plain = tmp_path / "plain.nwk"
    first = run(base + ["--support", "100", "-o", str(plain)])
    sup = internal_labels(plain.read_text())
    assert len(sup) == len(names) - 3
    assert all(re.fullmatch(r"\d+\.\d/\d\.\d{3}", s) for s in sup)

    # all four, in the fixed order SH-aLRT, aBayes, gCF, sCF
    out_nw, table = tmp_path / "all.nwk", tmp_path / "cf.tsv"
    text = run(base + ["--support", "100", "--scf", "20", "--gcf", str(genes), "-o", str(out_nw),
                       "--cf-table", str(table)])
    assert text == first  # the lnL line is untouched
    labs = internal_labels(out_nw.read_text())
    assert len(labs) == len(names) - 3
    for s in labs:
        assert re.fullmatch(r"\d+\.\d/\d\.\d{3}/%s/%s" % (num, num), s), s
    assert sorted("/".join(s.split("/")[:2]) for s in labs) == sorted(sup)
    gcf = sorted(s.split("/")[2] for s in labs)
    assert set(gcf) <= {"66.7", "100.0"} and "66.7" in gcf  # OTHER lacks some of the tree's splits

    # the table: one row per internal edge, the columns of the issue, the labels' values
    rows = [line.split("\t") for line in table.read_text().strip().split("\n")]
    assert rows[0] == ["id", "gCF", "gDF1", "gDF2", "gDFP", "gN", "sCF", "sDF1", "sDF2", "sN",
                       "length"]
    assert len(rows) == 1 + len(names) - 3 and all(len(r) == 11 for r in rows)
    assert len(set(r[0] for r in rows[1:])) == len(rows) - 1
    body = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert (body[:, 4] == 3).all() and (body[:, 10 - 1] > 0).all()
    np.testing.assert_allclose(body[:, :4].sum(axis=1), 100.0, atol=1e-7)
    np.testing.assert_allclose(body[:, 5:8].sum(axis=1), 100.0, atol=1e-7)
    assert sorted("%.1f" % v for v in body[:, 0]) == gcf
    assert sorted("%.1f" % v for v in body[:, 5]) == sorted(s.split("/")[3] for s in labs)

    # one of them alone: a single value per node; --scf without a number takes 100 quartets
    run(base + ["--scf", "-o", str(out_nw)])
    assert all(re.fullmatch(num, s) for s in internal_labels(out_nw.read_text()))
    run(base + ["--gcf", str(genes), "-o", str(out_nw), "--cf-table", str(table)])
    assert sorted(internal_labels(out_nw.read_text())) == gcf
    rows = [line.split("\t") for line in table.read_text().strip().split("\n")]
    assert all(r[6:10] == ["NA"] * 4 for r in rows[1:])
    # gCF and sCF without --support
    run(base + ["--scf", "20", "--gcf", str(genes), "-o", str(out_nw)])
    two = internal_labels(out_nw.read_text())
    assert all(re.fullmatch(r"%s/%s" % (num, num), s) for s in two)
    assert sorted(two) == sorted("/".join(s.split("/")[2:]) for s in labs)


@pytest.mark.gpu
def test_cli_scf_after_a_tree_search(tmp_path):
    """On the tree --nj builds, with --optimise: the labels sit on the final tree."""
    _, fa, _, names = write_case(tmp_path)
    out_nw = tmp_path / "nj.nwk"
    text = run(["-s", fa, "-m", MODEL, "--nj", "bionj", "--optimise", "1", "--scf", "10", "-o",
                str(out_nw)])
    assert text.startswith("lnL = ")
    tree = parse_newick(out_nw.read_text())
    assert sorted(x.label for x in tree.leaf_nodes()) == sorted(names)
    assert len(internal_labels(out_nw.read_text())) == len(names) - 3
