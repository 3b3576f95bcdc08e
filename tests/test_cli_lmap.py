"""The command line of likelihood mapping (``phy -s -m --lmap``): what the parser takes and what
``validate_args`` refuses, with no device."""
import pytest

from phylo_utils_amd import phy


@pytest.fixture
def fasta(tmp_path):
    p = tmp_path / "a.fasta"
    p.write_text(">a\nACGT\n>b\nACGA\n>c\nACTT\n>d\nAGGT\n")
    return str(p)


def test_parser_defaults_and_values(fasta):
    a = phy.parse_cli(["-s", fasta, "-m", "JC"])
    assert a.lmap is None and a.lmap_clusters is None and a.lmap_table is None and a.lmap_svg is None
    a = phy.parse_cli(["-s", fasta, "-m", "JC", "--lmap"])
    assert a.lmap == phy.LMAP_DEFAULT  # the default number: min(C(n, 4), 25 n)
    phy.validate_args(a)  # no -t needed
    a = phy.parse_cli(["-s", fasta, "--lmap", "50", "--lmap-table", "t.tsv", "--lmap-svg", "t.svg",
                       "--seed", "7"])
    assert (a.lmap, a.lmap_table, a.lmap_svg, a.seed) == (50, "t.tsv", "t.svg", 7)
    phy.validate_args(a)


def test_refusals(fasta, tmp_path):
    def refused(argv, exc=ValueError):
        with pytest.raises(exc):
            phy.validate_args(phy.parse_cli(argv))

    refused(["--lmap"])                                       # no alignment
    refused(["-s", str(tmp_path / "none.fasta"), "--lmap"], FileNotFoundError)
    refused(["-s", fasta, "--lmap", "-3"])
    refused(["-s", fasta, "--lmap", "-t", fasta])
    refused(["-s", fasta, "--lmap", "0"])
    refused(["-s", fasta, "--lmap", "--distances"])
    refused(["-s", fasta, "--lmap", "--nj", "bionj"])                  # would be ignored: refused
    refused(["-s", fasta, "--lmap", "--parsimony"])
    refused(["-s", fasta, "--nj", "nj", "--lmap-table", "x.tsv"])      # needs --lmap
    refused(["-s", fasta, "--parsimony", "--lmap-svg", "x.svg"])
    refused(["-s", fasta, "-t", fasta, "--lmap-table", "x.tsv"])   # needs --lmap
    refused(["-s", fasta, "-t", fasta, "--lmap-svg", "x.svg"])
    refused(["-s", fasta, "-t", fasta, "--lmap-clusters", fasta])
    refused(["-s", fasta, "--lmap", "--lmap-clusters", str(tmp_path / "none.txt")],
            FileNotFoundError)


def test_cluster_file(tmp_path):
    p = tmp_path / "c.txt"
    p.write_text("a b\n\nc, d\ne\nf g h\n")
    assert phy.read_clusters(str(p)) == [["a", "b"], ["c", "d"], ["e"], ["f", "g", "h"]]
    p.write_text("a b\nc\nd\n")
    with pytest.raises(ValueError, match="not four"):
        phy.read_clusters(str(p))
