"""``phy`` -- lnL of an alignment on a tree (counterpart of the reference's ``bin/phy.py``,
SURVEY 8(f) N2).

    python -m phylo_utils_amd.phy -t tree.nwk -s aln.fasta -m 'GTR{1.0,2.0,1.0,1.0,2.0,1.0}+G4{0.5}'

Same options and output as ``bin/phy.py:13-19, 146`` (``lnL = <value>``).  The model
string grammar is ``bin/phy.py:41-56``: a model name, optional ``{parameters}``, then up to
two of ``+F{freqs}`` and ``+G<ncat>{alpha}``.  Differences, all deliberate:

* the reference passes every model ``(rates=..., freqs=...)`` (``:128``), which only
  ``GTR`` accepts -- the others raise TypeError; here each model gets its parameters in
  its own constructor's order (K80/HKY85/F84: kappa; TN93: alpha_y, alpha_r[, beta]);
* ``JC``/``JC69`` runs (the reference's ``JC69.p`` has no ``rates`` argument and cannot go
  through TreeModel);
* parameters may be written as integers (``{2}``) as well as ``{2.0}``, and model names
  may contain digits (the reference's ``Word(alphas)`` reads ``HKY85{2.0}`` as ``HKY`` and
  drops the rest of the string);
* Newick and FASTA are read without dendropy / Biopython (``tree.parse_newick``,
  ``alignment.read_fasta``).
Extensions: ``--optimise`` runs branch-length optimisation passes on the GPU first
(``--optimiser newton|brent|dbrent``)
(SURVEY 8(f) N1); ``--ascertainment`` applies the Lewis correction (N3); ``--device``;
``--simulate N [--seed S] [-o out.fasta]`` needs no ``-s``: it simulates N columns down the
tree under the model on the GPU (``phylo_utils_amd.simulation``, the reference's
``src/simulation.pyx``) and writes them as FASTA, to stdout without ``-o``;
``-s aln.fasta -m MODEL --distances [-o FILE]`` needs no ``-t``: it writes the square PHYLIP
matrix of the pairwise ML distances (``phylo_utils_amd.distance``, the reference's
``likelihood.py:226-236`` per pair), names in alignment order, ``%.10g``;
``-s aln.fasta -m MODEL --nj {nj,bionj} [-o tree.nwk]`` needs no ``-t`` either: the tree is the
neighbour-joining (or BIONJ) tree of those distances (``phylo_utils_amd.nj``; the reference has
no tree builder), written as Newick to ``-o`` when given, and the ``lnL = `` line is that tree's,
after ``--optimise`` when asked; with ``--bootstrap R`` (and the seed of ``--seed``) the Newick
carries, as internal node labels, the support in percent of every split over R bootstrap
replicates (``phylo_utils_amd.bootstrap``);
``-s aln.fasta -m MODEL --parsimony [R] [-o tree.nwk]`` needs no ``-t`` either and excludes
``--nj``: the tree is the shortest of R (default 1) randomised stepwise-addition trees under Fitch
parsimony (``phylo_utils_amd.parsimony``, the seed of ``--seed``; the reference has no tree
builder), written to ``-o`` when given; one extra line ``parsimony = <length>`` comes before the
``lnL = `` line, and ``--nni``, ``--spr``, ``--optimise``, ``--support`` and ``-o`` follow as they do
after ``--nj``.  With ``--parsimony-spr [ROUNDS]`` (and ``--parsimony-radius R``), valid only with
``--parsimony``, all R trees are refined by parsimony SPR before the shortest is kept
(``parsimony.spr_search``: at most ROUNDS rounds each, default until no move shortens the tree) and
the ``parsimony = `` line is the refined length.  ``--parsimony-score`` (after ``-t`` or ``--nj``) prints the same line for that tree
and changes nothing else;
``--nni [ROUNDS]`` (after ``-t`` or ``--nj``) improves the topology by nearest-neighbour
interchanges on the GPU before the ``lnL = `` line (``phylo_utils_amd.nni``, at most ROUNDS
rounds, default 50); ``-o`` then receives the final Newick;
``--spr [ROUNDS]`` (after ``-t`` or ``--nj``, and after ``--nni`` when both are given) improves the
topology by subtree pruning and regrafting on the GPU before the ``lnL = `` line
(``phylo_utils_amd.spr``, at most ROUNDS rounds, default 50; ``--spr-radius R`` scores only the
regraft edges within R edges of the pruned subtree's old place, default: all); ``-o`` then
receives the final Newick;
``--support [R]`` (after ``-t`` or ``--nj``, and after ``--nni`` when given) labels every internal
edge of the final tree with ``SH-aLRT/aBayes`` -- percent with one decimal over R RELL replicates
(default 1000, the seed of ``--seed``) and probability with three (``phylo_utils_amd.support``)
-- on optimised branch lengths (one pass of ``--optimiser`` where neither ``--optimise`` nor
``--nni`` has optimised them), and writes that Newick to ``-o``;
``--ancestral FILE`` writes the marginal reconstruction of the N - 2 internal nodes as FASTA
(records ``N<node index>``, one most probable state per alignment column) and ``FILE.nwk``, the
tree with those names on its internal nodes; ``--site-rates FILE`` writes a TSV with a header and
one row per alignment column: site (from 1), posterior mean rate, most probable rate category
(from 1) (``phylo_utils_amd.ancestral``).  Both run on the final tree, after ``--optimise`` /
``--nni``;
``--fit [LIST]`` (after ``--nj`` / ``--nni`` / ``--optimise``, before ``--support`` / ``--ancestral``
/ ``--site-rates``) fits the model parameters in the comma-separated LIST -- default: every free
parameter of the ``-m`` model (``rates``, ``kappa``, ``alpha_y``, ``alpha_r``, ``freqs``,
``alpha``) -- jointly with all branch lengths on the exact gradient
(``phylo_utils_amd.modelfit``), prints one extra line ``model = <string>`` before ``lnL = ``, the
fitted model in the grammar above (``%.10g``) so that ``-m`` reads it back, and writes the tree
with the fitted lengths to ``-o``;
``--place QUERIES.fasta [--keep K] --jplace OUT.jplace`` (after ``-t`` or ``--nj``, and after
``--nni`` / ``--fit`` when given) places the query sequences of QUERIES.fasta -- aligned to ``-s``,
of its full length -- on the final tree without rebuilding it (``phylo_utils_amd.place``): every
query is scored at every edge, its K best edges (default 5) are refined on the pendant length,
and OUT.jplace receives them in jplace version 3 (``edge_num, likelihood, like_weight_ratio,
distal_length, pendant_length``); ``--placed-trees FILE`` receives one Newick per query, the tree
with that query joined at its best placement (``-o`` stays what the other options make it);
``--test-trees FILE [--test-replicates R] [--no-au]`` tests the candidate topologies of FILE, one
Newick per line, against each other (``phylo_utils_amd.topotest``): the final tree of the run --
when ``-t``, ``--nj`` or ``--parsimony`` gave one; ``-s`` and ``-m`` alone do -- is tree 0, the
trees of FILE follow, every tree's branch lengths are optimised (``--optimise`` passes, at least
one), and after the ``lnL = `` line come a header and one line per tree, ``tree i: lnL deltaL
bp-RELL p-KH p-SH c-ELW p-AU`` over R RELL replicates (default 10000, the seed of ``--seed``),
every value from bp-RELL on followed by ``+`` (the tree stays in the 95 % set of that test) or
``-`` (rejected); ``--no-au`` skips the multiscale replicates and prints p-AU as ``-``;
``--bootstrap R --consensus FILE [--consensus-threshold P]`` (with ``--nj``) also writes the
majority-rule consensus of the R replicate trees to FILE (``phylo_utils_amd.treeset``): the splits
held by more than the share P of the replicates (default 0.5; 1.0: by all of them, the strict
consensus), every internal node labelled with its split's share in percent, no branch lengths;
``--compare-trees FILE`` compares the run's final tree (tree 0) with the Newick trees of FILE, one
per line (trees 1, 2, ...): after the ``lnL = `` line (and the ``--test-trees`` table) come one line
``rf i: d_0 d_1 ...`` per tree, its Robinson-Foulds distances to all of them, and ``topologies = k
distinct of m``; with ``--tree-metric {wrf,kf,path,wpath}`` one line ``<metric> i: d_0 d_1 ...``
per tree follows the ``rf`` lines: the weighted Robinson-Foulds, branch-score, path-difference or
weighted path-difference distances (``treeset.distances``; tree 0 with the run's final lengths,
every tree of FILE needs a length on every edge), printed with ``repr``;
``-s aln.fasta -m MODEL --lmap [Q]`` needs no ``-t`` either: likelihood mapping
(``phylo_utils_amd.lmap``) of Q quartets (default min(C(n,4), 25 n), the seed of
``--seed``; with ``--lmap-clusters FILE``, four lines of taxon names, one taxon of each line per
quartet).  It prints ``lmap: quartets = ...``, one ``lmap: region k = count (pct %)`` line per
region 1-7 (the three corners, the three edges, the centre) and a ``lmap: resolved ... partly ...
unresolved ...`` line; ``--lmap-table FILE`` writes a TSV with one row per quartet, ``--lmap-svg
FILE`` the two triangles.

``--scf [Q]`` and ``--gcf FILE`` (after ``-t``, ``--nj`` or ``--parsimony``, on the final tree, after
``--support``) label every internal edge with concordance factors (``phylo_utils_amd.concordance``):
the site concordance factor over up to Q quartets per branch (default 100, the seed of ``--seed``)
and the gene concordance factor in the Newick trees of FILE, one per line, all over the
alignment's taxa.  The labels of an internal node are joined by ``/`` in the fixed order SH-aLRT,
aBayes, gCF, sCF, of those asked for (concordance factors in percent with one decimal, ``NA`` where
no quartet has a decisive site), and ``-o`` receives that Newick; ``--cf-table FILE`` writes a TSV
with a header and one row per internal edge: ``id gCF gDF1 gDF2 gDFP gN sCF sDF1 sDF2 sN length``,
``id`` the edge's number in the tree's op order, ``NA`` for what was not asked for.
"""
from __future__ import annotations

import argparse
import os
import re
import sys

from . import alignment as A
from . import rate_models as RM
from . import substitution_models as SM
from .tree import parse_newick
from .tree_model import TreeModel

PROTEIN_MODELS = ("JTT", "Dayhoff", "WAG", "LG")
_PART = re.compile(r"\+(F|G(\d+))(\{[^}]*\})?")
_HEAD = re.compile(r"([A-Za-z][A-Za-z0-9]*)(\{[^}]*\})?")


def _reals(braces):
    if braces is None:
        return None
    body = braces[1:-1].strip()
    if not body:
        raise ValueError("empty parameter list {}")
    return [float(x) for x in body.split(",")]


def parse_model_string(text):
    """bin/phy.py:41-56 -> dict(subs_model, model_params, freq_params, rate_model,
    rate_cats, rate_param); absent parts are None."""
    text = text.strip().replace(" ", "")
    m = _HEAD.match(text)
    if not m:
        raise ValueError("model string %r does not start with a model name" % text)
    out = dict(subs_model=m.group(1), model_params=_reals(m.group(2)), freq_params=None,
               rate_model=None, rate_cats=None, rate_param=None)
    rest, n = text[m.end():], 0
    while rest:
        p = _PART.match(rest)
        if not p or n == 2:
            raise ValueError("cannot parse %r in model string %r" % (rest, text))
        if p.group(1) == "F":
            out["freq_params"] = _reals(p.group(3))
        else:
            out["rate_model"] = "G"
            out["rate_cats"] = int(p.group(2))
            vals = _reals(p.group(3))
            out["rate_param"] = vals
        rest, n = rest[p.end():], n + 1
    return out


def _one(vals):
    """bin/phy.py:83-91 unpack: a single value is a scalar."""
    if vals is None:
        return None
    return vals[0] if len(vals) == 1 else vals


def build_model(desc):
    """Substitution model from a parsed model string (bin/phy.py:59-80, 119-128)."""
    name, p, f = desc["subs_model"], desc["model_params"], desc["freq_params"]
    freqs = None if f is None else list(f)
    try:
        if name == "GTR":
            return SM.GTR(rates=p, freqs=freqs)
        if name in ("JC", "JC69"):
            return SM.JC69()
        if name == "K80":
            return SM.K80(*(p or [2.0]))
        if name in ("HKY", "HKY85"):
            return SM.HKY85((p or [2.0])[0], freqs if freqs else [0.25] * 4)
        if name == "F81":
            return SM.F81(freqs if freqs else [0.25] * 4)
        if name == "F84":
            return SM.F84((p or [2.0])[0], freqs if freqs else [0.25] * 4)
        if name == "TN93":
            q = list(p or [2.0, 2.0])
            return SM.TN93(*q, freqs=freqs if freqs else [0.25] * 4)
        if name in PROTEIN_MODELS:
            return getattr(SM, name)(freqs=freqs)
    except TypeError as e:
        raise ValueError("bad parameters for model %s: %s" % (name, e))
    raise ValueError("Unrecognised model %s; valid options are GTR, HKY, HKY85, K80, F81, F84, "
                     "JC, JC69, TN93, LG, WAG, JTT, Dayhoff" % name)


def build_rate_model(desc):
    """bin/phy.py:130-138: +G<ncat>{alpha} -> Gamma (defaults 4, 0.5), else uniform."""
    if desc["rate_model"] == "G":
        ncat = desc["rate_cats"] if desc["rate_cats"] is not None else 4
        alpha = _one(desc["rate_param"])
        return RM.GammaRateModel(ncat, alpha if alpha is not None else 0.5)
    return RM.UniformRateModel()


LMAP_DEFAULT = ("default",)  # --lmap without a number: min(C(n, 4), 25 n) quartets (no string: argparse would convert it)


def parse_cli(argv=None):
    ap = argparse.ArgumentParser("phy - calculate likelihood of an alignment given a "
                                 "phylogenetic model")
    ap.add_argument("-t", "--tree", type=str, help="File path to a tree in newick format")
    ap.add_argument("-s", "--alignment", type=str, help="File path to an alignment in fasta "
                    "format")
    ap.add_argument("-m", "--model", type=str, default="JC", help="Model specification string")
    ap.add_argument("--device", type=int, default=0, help="HIP device")
    ap.add_argument("--optimise", type=int, default=0, metavar="PASSES",
                    help="optimise branch lengths first (passes of the optimising traversal)")
    ap.add_argument("--optimiser", default="newton", choices=["newton", "brent", "dbrent"],
                    help="per-edge method of --optimise (brent / dbrent: the reference's "
                         "src/optimisation.pyx minimisers)")
    ap.add_argument("--ascertainment", choices=["reference", "weighted"], default=None,
                    help="Lewis ascertainment-bias correction")
    ap.add_argument("--simulate", type=int, default=None, metavar="N",
                    help="simulate N alignment columns down the tree (no -s) and write FASTA")
    ap.add_argument("--seed", type=int, default=0, help="seed of --simulate")
    ap.add_argument("--distances", action="store_true",
                    help="write the PHYLIP matrix of pairwise ML distances of -s (no -t)")
    ap.add_argument("--nj", choices=["nj", "bionj"], default=None,
                    help="take the tree from neighbour joining (or BIONJ) on the pairwise ML "
                         "distances of -s (no -t); -o receives its Newick")
    ap.add_argument("--parsimony", type=int, nargs="?", const=1, default=None, metavar="R",
                    help="take the tree from randomised stepwise addition under Fitch parsimony, "
                         "the shortest of R addition orders (default 1; seed: --seed; no -t, no "
                         "--nj); prints a 'parsimony = ' line; -o receives its Newick")
    ap.add_argument("--parsimony-spr", type=int, nargs="?", const=0, default=None,
                    dest="parsimony_spr", metavar="ROUNDS",
                    help="with --parsimony: refine all R stepwise-addition trees by parsimony "
                         "SPR before the shortest is kept, at most ROUNDS rounds each (default "
                         "0: until no move shortens the tree); the 'parsimony = ' line is the "
                         "refined length")
    ap.add_argument("--parsimony-radius", type=int, default=None, dest="parsimony_radius",
                    metavar="R",
                    help="with --parsimony-spr: regraft at most R edges away from where the "
                         "subtree was pruned (default: no limit)")
    ap.add_argument("--parsimony-score", action="store_true", dest="parsimony_score",
                    help="after -t or --nj: print the tree's Fitch parsimony length as a "
                         "'parsimony = ' line before the lnL line")
    ap.add_argument("--bootstrap", type=int, default=None, metavar="R",
                    help="with --nj: label the tree's splits with their support in percent "
                         "over R bootstrap replicates (seed: --seed)")
    ap.add_argument("--nni", type=int, nargs="?", const=50, default=None, metavar="ROUNDS",
                    help="after -t or --nj: nearest-neighbour-interchange search (at most ROUNDS "
                         "rounds, default 50) before the lnL line; -o receives the final Newick")
    ap.add_argument("--spr", type=int, nargs="?", const=50, default=None, metavar="ROUNDS",
                    help="after -t or --nj (and --nni): subtree-pruning-and-regrafting search (at "
                         "most ROUNDS rounds, default 50) before the lnL line; -o receives the "
                         "final Newick")
    ap.add_argument("--spr-radius", type=int, default=None, metavar="R", dest="spr_radius",
                    help="with --spr: score only the regraft edges within R edges of the pruned "
                         "subtree's old place (default: every edge)")
    ap.add_argument("--support", type=int, nargs="?", const=1000, default=None, metavar="R",
                    help="after -t or --nj (and --nni): label the internal edges of the final "
                         "tree with SH-aLRT/aBayes supports over R RELL replicates (default "
                         "1000; seed: --seed); -o receives the labelled Newick")
    ap.add_argument("--ancestral", type=str, default=None, metavar="FILE",
                    help="write the marginal ancestral sequences of the internal nodes as FASTA "
                         "to FILE and the tree that names them to FILE.nwk")
    ap.add_argument("--site-rates", type=str, default=None, metavar="FILE", dest="site_rates",
                    help="write a TSV of site, posterior mean rate and most probable rate "
                         "category per alignment column to FILE")
    ap.add_argument("--fit", type=str, nargs="?", const="", default=None, metavar="LIST",
                    help="fit the model parameters in the comma-separated LIST (default: every "
                         "free parameter of the -m model) jointly with all branch lengths, "
                         "after --optimise / --nni; prints a 'model = ' line that -m reads back; "
                         "-o receives the Newick with the fitted lengths")
    ap.add_argument("--place", type=str, default=None, metavar="QUERIES",
                    help="place the aligned query sequences of this FASTA file on the final tree "
                         "(needs --jplace)")
    ap.add_argument("--keep", type=int, default=5, metavar="K",
                    help="with --place: edges per query whose pendant length is refined")
    ap.add_argument("--jplace", type=str, default=None, metavar="FILE",
                    help="with --place: the jplace (version 3) file to write")
    ap.add_argument("--placed-trees", type=str, default=None, metavar="FILE", dest="placed_trees",
                    help="with --place: write one Newick per query, the tree with the query "
                         "joined at its best placement")
    ap.add_argument("--test-trees", type=str, default=None, metavar="FILE", dest="test_trees",
                    help="test the candidate trees of FILE (one Newick per line) and the run's "
                         "final tree (tree 0) against each other: RELL bootstrap proportions, KH, "
                         "SH, c-ELW and AU, one line per tree after the lnL line")
    ap.add_argument("--test-replicates", type=int, default=10000, metavar="R",
                    dest="test_replicates",
                    help="with --test-trees: RELL replicates per scale (default 10000; seed: "
                         "--seed)")
    ap.add_argument("--no-au", action="store_true", dest="no_au",
                    help="with --test-trees: no multiscale replicates; p-AU is printed as '-'")
    ap.add_argument("--consensus", type=str, default=None, metavar="FILE",
                    help="with --bootstrap: write the majority-rule consensus of the replicate "
                         "trees, labelled with the splits' shares in percent, to FILE")
    ap.add_argument("--consensus-threshold", type=float, default=0.5, metavar="P",
                    dest="consensus_threshold",
                    help="with --consensus: keep the splits in more than the share P of the "
                         "replicates (0.5 to 1; 1: in all of them; default 0.5)")
    ap.add_argument("--tree-metric", type=str, default=None, dest="tree_metric",
                    choices=["wrf", "kf", "path", "wpath"],
                    help="with --compare-trees: after the rf lines, one '<metric> i: ...' line per "
                         "tree with its weighted RF, branch-score, path or weighted path "
                         "distances to all of them (every tree needs branch lengths)")
    ap.add_argument("--compare-trees", type=str, default=None, metavar="FILE",
                    dest="compare_trees",
                    help="after the lnL line: Robinson-Foulds distances between the final tree "
                         "(tree 0) and the Newick trees of FILE, and the number of distinct "
                         "topologies among them")
    ap.add_argument("--scf", type=int, nargs="?", const=100, default=None, metavar="Q",
                    help="label the internal edges of the final tree with site concordance "
                         "factors over up to Q quartets per branch (default 100; seed: --seed)")
    ap.add_argument("--gcf", type=str, default=None, metavar="FILE",
                    help="label the internal edges of the final tree with gene concordance "
                         "factors in the Newick trees of FILE (one per line)")
    ap.add_argument("--cf-table", type=str, default=None, metavar="FILE", dest="cf_table",
                    help="with --scf or --gcf: write a TSV with one row per internal edge (id, "
                         "gCF, gDF1, gDF2, gDFP, gN, sCF, sDF1, sDF2, sN, length)")
    ap.add_argument("--lmap", type=int, nargs="?", const=LMAP_DEFAULT, default=None, metavar="Q",
                    help="likelihood mapping of -s (no -t): fit the three trees of Q quartets "
                         "(default min(C(n,4), 25 n); seed: --seed) and print the shares of the "
                         "seven regions of the triangle")
    ap.add_argument("--lmap-clusters", type=str, default=None, metavar="FILE",
                    dest="lmap_clusters",
                    help="with --lmap: four lines of taxon names; every quartet takes one taxon "
                         "of each line")
    ap.add_argument("--lmap-table", type=str, default=None, metavar="FILE", dest="lmap_table",
                    help="with --lmap: write a TSV with one row per quartet (taxa, three lnL, "
                         "three weights, regions)")
    ap.add_argument("--lmap-svg", type=str, default=None, metavar="FILE", dest="lmap_svg",
                    help="with --lmap: draw the two triangles to FILE")
    ap.add_argument("-o", "--output", type=str, default=None,
                    help="output file of --simulate / --distances (default: stdout) / --nj / "
                         "--nni")
    return ap.parse_args(argv)


def validate_args(args):
    """bin/phy.py:22-30."""
    if getattr(args, "lmap", None) is None:
        for k in ("lmap_clusters", "lmap_table", "lmap_svg"):
            if getattr(args, k, None) is not None:
                raise ValueError("--%s needs --lmap" % k.replace("_", "-"))
    else:  # a run of its own: it takes no tree and nothing that makes or works on one
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None \
                or args.tree is not None or getattr(args, "nj", None) is not None \
                or getattr(args, "parsimony", None) is not None:
            raise ValueError("--lmap excludes --distances, --simulate, -t, --nj and --parsimony")
        if args.lmap != LMAP_DEFAULT and args.lmap < 1:
            raise ValueError("--lmap needs at least one quartet")
        if args.alignment is None:
            raise ValueError("Alignment file not specified")
        if not os.path.exists(args.alignment):
            raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))
        cl = getattr(args, "lmap_clusters", None)
        if cl is not None and not os.path.exists(cl):
            raise FileNotFoundError("Cluster file {} does not exist".format(cl))
        return
    if getattr(args, "parsimony_spr", None) is not None:
        if getattr(args, "parsimony", None) is None:
            raise ValueError("--parsimony-spr needs --parsimony")
        if args.parsimony_spr < 0:
            raise ValueError("--parsimony-spr needs a number of rounds >= 0")
    if getattr(args, "parsimony_radius", None) is not None:
        if getattr(args, "parsimony_spr", None) is None:
            raise ValueError("--parsimony-radius needs --parsimony-spr")
        if args.parsimony_radius < 0:
            raise ValueError("--parsimony-radius needs a radius >= 0")
    if getattr(args, "ancestral", None) is not None or getattr(args, "site_rates", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--ancestral and --site-rates exclude --simulate and --distances")
    if getattr(args, "place", None) is not None or getattr(args, "jplace", None) is not None \
            or getattr(args, "placed_trees", None) is not None:
        if getattr(args, "place", None) is None or getattr(args, "jplace", None) is None:
            raise ValueError("--place and --jplace go together (--placed-trees needs both)")
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--place excludes --simulate and --distances")
        if getattr(args, "ascertainment", None):
            raise ValueError("--place with --ascertainment is not implemented")
        if getattr(args, "keep", 5) < 1:
            raise ValueError("--keep needs at least one edge")
        if not os.path.exists(args.place):
            raise FileNotFoundError("Query file {} does not exist".format(args.place))
    if getattr(args, "test_trees", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--test-trees excludes --simulate and --distances")
        if getattr(args, "ascertainment", None):
            raise ValueError("--test-trees with --ascertainment is not implemented")
        if getattr(args, "test_replicates", 10000) < 1:
            raise ValueError("--test-replicates needs at least one replicate")
        if not os.path.exists(args.test_trees):
            raise FileNotFoundError("Tree file {} does not exist".format(args.test_trees))
        if args.tree is None and getattr(args, "nj", None) is None and \
                getattr(args, "parsimony", None) is None:
            # no tree of the run's own: the candidates alone
            for name in ("optimise", "nni", "spr", "fit", "place", "support", "ancestral",
                         "site_rates", "parsimony_score", "scf", "gcf"):
                if getattr(args, name, None) not in (None, 0, False):
                    raise ValueError("--{} needs a tree (-t, --nj or --parsimony)".format(
                        name.replace("_", "-")))
            if args.alignment is None:
                raise ValueError("Alignment file not specified")
            if not os.path.exists(args.alignment):
                raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))
            return
    if getattr(args, "fit", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--fit excludes --simulate and --distances")
        if getattr(args, "ascertainment", None):
            raise ValueError("--fit with --ascertainment is not implemented")
    if getattr(args, "nni", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--nni excludes --simulate and --distances")
        if args.nni < 0:
            raise ValueError("--nni needs a non-negative number of rounds")
    if getattr(args, "spr", None) is not None or getattr(args, "spr_radius", None) is not None:
        if getattr(args, "spr", None) is None:
            raise ValueError("--spr-radius needs --spr")
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--spr excludes --simulate and --distances")
        if getattr(args, "ascertainment", None):
            raise ValueError("--spr with --ascertainment is not implemented")
        if args.spr < 0:
            raise ValueError("--spr needs a non-negative number of rounds")
        if getattr(args, "spr_radius", None) is not None and args.spr_radius < 1:
            raise ValueError("--spr-radius needs a radius of at least 1")
    if getattr(args, "support", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--support excludes --simulate and --distances")
        if args.support < 1:
            raise ValueError("--support needs at least one replicate")
    if getattr(args, "consensus", None) is not None:
        if getattr(args, "bootstrap", None) is None:
            raise ValueError("--consensus needs --bootstrap")
        if not 0.5 <= getattr(args, "consensus_threshold", 0.5) <= 1.0:
            raise ValueError("--consensus-threshold needs a share within [0.5, 1]")
    if getattr(args, "tree_metric", None) is not None \
            and getattr(args, "compare_trees", None) is None:
        raise ValueError("--tree-metric needs --compare-trees")
    if getattr(args, "compare_trees", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--compare-trees excludes --simulate and --distances")
        if not os.path.exists(args.compare_trees):
            raise FileNotFoundError("Tree file {} does not exist".format(args.compare_trees))
    if getattr(args, "cf_table", None) is not None and getattr(args, "scf", None) is None \
            and getattr(args, "gcf", None) is None:
        raise ValueError("--cf-table needs --scf or --gcf")
    if getattr(args, "scf", None) is not None or getattr(args, "gcf", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--scf and --gcf exclude --simulate and --distances")
        if getattr(args, "scf", None) is not None and args.scf < 1:
            raise ValueError("--scf needs at least one quartet per branch")
        if getattr(args, "gcf", None) is not None and not os.path.exists(args.gcf):
            raise FileNotFoundError("Tree file {} does not exist".format(args.gcf))
    if getattr(args, "bootstrap", None) is not None:
        if getattr(args, "nj", None) is None:
            raise ValueError("--bootstrap needs --nj")
        if args.bootstrap < 1:
            raise ValueError("--bootstrap needs at least one replicate")
    if getattr(args, "parsimony", None) is not None:
        if args.tree is not None or getattr(args, "nj", None) is not None:
            raise ValueError("--parsimony excludes -t and --nj")
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--parsimony excludes --distances and --simulate")
        if args.parsimony < 1:
            raise ValueError("--parsimony needs at least one addition order")
        if args.alignment is None:
            raise ValueError("Alignment file not specified")
        if not os.path.exists(args.alignment):
            raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))
        return
    if getattr(args, "parsimony_score", False):
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None:
            raise ValueError("--parsimony-score excludes --distances and --simulate")
    if getattr(args, "nj", None) is not None:
        if getattr(args, "distances", False) or getattr(args, "simulate", None) is not None \
                or args.tree is not None:
            raise ValueError("--nj excludes --distances, --simulate and -t")
        if args.alignment is None:
            raise ValueError("Alignment file not specified")
        if not os.path.exists(args.alignment):
            raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))
        return
    if getattr(args, "distances", False):
        if getattr(args, "simulate", None) is not None:
            raise ValueError("--distances and --simulate exclude each other")
        if args.alignment is None:
            raise ValueError("Alignment file not specified")
        if not os.path.exists(args.alignment):
            raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))
        return
    if args.tree is None:
        raise ValueError("Tree file not specified")
    if getattr(args, "simulate", None) is not None:
        if args.simulate <= 0:
            raise ValueError("--simulate needs a positive number of sites")
        if not os.path.exists(args.tree):
            raise FileNotFoundError("Tree file {} does not exist".format(args.tree))
        return
    if args.alignment is None:
        raise ValueError("Alignment file not specified")
    if not os.path.exists(args.tree):
        raise FileNotFoundError("Tree file {} does not exist".format(args.tree))
    if not os.path.exists(args.alignment):
        raise FileNotFoundError("Alignment file {} does not exist".format(args.alignment))


def run(args, out=None):
    out = sys.stdout if out is None else out
    nj = getattr(args, "nj", None)
    pars = getattr(args, "parsimony", None)
    pars_length = None
    given = nj is None and pars is None and args.tree is not None
    if given:
        with open(args.tree) as fh:
            tree = parse_newick(fh.read())
    aln = A.read_fasta(args.alignment)
    desc = parse_model_string(args.model)
    alphabet = A.PROTEIN if desc["subs_model"] in PROTEIN_MODELS else A.DNA
    tm = TreeModel(device=args.device)
    if given:
        tm.set_tree(tree)
    tm.set_alignment(aln, alphabet)
    tm.set_rate_model(build_rate_model(desc))
    tm.set_substitution_model(build_model(desc))
    if nj is None and pars is None and not given:  # --test-trees on its candidates alone
        for line in run_test_trees(args, tm, None):
            out.write(line + "\n")
        return None
    if nj is not None:  # --nj: the tree from the alignment's own distances
        if getattr(args, "bootstrap", None) is not None:
            want = getattr(args, "consensus", None) is not None
            res = tm.bootstrap_nj(args.bootstrap, seed=args.seed, method=nj,
                                  return_replicates=want)
            tree = res[0]
            if want:
                from . import treeset
                if res[2] != args.bootstrap:  # such a replicate's tree is unspecified
                    raise ValueError("--consensus: {} of the {} replicates have a distance that "
                                     "is not finite".format(args.bootstrap - res[2],
                                                            args.bootstrap))
                reps = res[3]
                names = sorted(tm.names, key=tm.names.get)
                res = treeset.compare(reps, names=names, rows=0, device=args.device, form="joins")
                cons = treeset.consensus(res, getattr(args, "consensus_threshold", 0.5))
                with open(args.consensus, "w") as fh:
                    fh.write(cons.as_newick() + "\n")
        else:
            tree = tm.set_nj_tree(method=nj)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
    if pars is not None:  # --parsimony: the shortest of R stepwise-addition trees
        tree, pars_length, _ = tm.set_parsimony_tree(
            n_rep=pars, seed=args.seed, spr_rounds=getattr(args, "parsimony_spr", None),
            spr_radius=getattr(args, "parsimony_radius", None))
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
    elif getattr(args, "parsimony_score", False):
        pars_length = tm.parsimony_length()
    if args.ascertainment:
        tm.set_ascertainment_bias_correction(weighted=args.ascertainment == "weighted")
    tm.initialise()
    if args.optimise:
        tm.optimise_branch_lengths(sweeps=args.optimise, method=args.optimiser)
    if getattr(args, "nni", None) is not None:
        tree, _, _ = tm.nni_search(max_rounds=args.nni, sweeps=max(args.optimise, 1),
                                   method=args.optimiser)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
    if getattr(args, "spr", None) is not None:
        tree, _, _ = tm.spr_search(radius=getattr(args, "spr_radius", None), max_rounds=args.spr,
                                   sweeps=max(args.optimise, 1), method=args.optimiser)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
    fitted = None
    if getattr(args, "fit", None) is not None:
        from . import modelfit
        from .tree import with_lengths
        names = [x for x in args.fit.split(",") if x] or \
            modelfit.free_parameters(tm.substitution_model, tm.rate_model)
        tm.optimise_model(params=names, branch_lengths=True)
        fitted = modelfit.model_string(tm.substitution_model, tm.rate_model)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(with_lengths(tm.tree, tm.traversal.brlens).as_newick() + "\n")
    if getattr(args, "place", None) is not None:
        from . import place as PL
        res = tm.place(A.read_fasta(args.place), keep=getattr(args, "keep", 5))
        placed_on = PL.current_tree(tm)
        PL.write_jplace(args.jplace, placed_on, res,
                        invocation="phy --place {} --keep {}".format(
                            os.path.basename(args.place), getattr(args, "keep", 5)))
        if getattr(args, "placed_trees", None):
            with open(args.placed_trees, "w") as fh:
                for name, rows in zip(res["names"], res["placements"]):
                    fh.write(PL.attach(placed_on, rows[0]["edge"], name,
                                       rows[0]["pendant"]).as_newick() + "\n")
    if getattr(args, "support", None) is not None:
        from .support import label_tree, support_label
        from .tree import with_lengths
        if not args.optimise and getattr(args, "nni", None) is None and \
                getattr(args, "spr", None) is None:
            tm.optimise_branch_lengths(sweeps=1, method=args.optimiser)
        quartets, _, sup = tm.branch_support(n_replicates=args.support, seed=args.seed)
        tree = label_tree(with_lengths(tm.tree, tm.traversal.brlens), quartets,
                          list(zip(sup["sh_alrt"], sup["abayes"])),
                          lambda v: support_label(*v))
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
        support_labels = {int(q[0]): support_label(a, b)
                          for q, a, b in zip(quartets, sup["sh_alrt"], sup["abayes"])}
    else:
        support_labels = None
    if getattr(args, "scf", None) is not None or getattr(args, "gcf", None) is not None:
        tree = run_concordance(args, tm, support_labels)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(tree.as_newick() + "\n")
    if getattr(args, "ancestral", None) is not None:
        seqs, newick = tm.ancestral_sequences(alphabet)
        with open(args.ancestral, "w") as fh:
            for name, seq in seqs.items():
                fh.write(">{}\n".format(name))
                for i in range(0, len(seq), 60):
                    fh.write(seq[i:i + 60] + "\n")
        with open(args.ancestral + ".nwk", "w") as fh:
            fh.write(newick + "\n")
    if getattr(args, "site_rates", None) is not None:
        cat, rate = tm.site_rates()
        with open(args.site_rates, "w") as fh:
            fh.write("site\tmean_rate\tmap_category\n")
            for i, (r, k) in enumerate(zip(rate, cat.argmax(axis=1))):
                fh.write("{}\t{:.10g}\t{}\n".format(i + 1, r, int(k) + 1))
    table = []
    if getattr(args, "test_trees", None) is not None:
        from .tree import with_lengths
        table = run_test_trees(args, tm, with_lengths(tm.tree, tm.traversal.brlens))
    lnl = tm.compute_likelihood_at_edge(*tm.traversal.root_edge).sum()
    if pars_length is not None:
        out.write("parsimony = {}\n".format(pars_length))
    if fitted is not None:
        out.write("model = {}\n".format(fitted))
    out.write("lnL = {}\n".format(lnl))
    for line in table:
        out.write(line + "\n")
    if getattr(args, "compare_trees", None) is not None:
        for line in run_compare_trees(args, tm):
            out.write(line + "\n")
    return lnl


def run_concordance(args, tm, support_labels):
    """--scf / --gcf / --cf-table: the final tree with its labels -- `support_labels` ({node
    index: SH-aLRT/aBayes} or None), then gCF, then sCF -- and the table."""
    from . import concordance
    from .tree import with_lengths
    trees = None
    if getattr(args, "gcf", None) is not None:
        with open(args.gcf) as fh:
            trees = [line.strip() for line in fh if line.strip()]
        if not trees:
            raise ValueError("--gcf: {} holds no tree".format(args.gcf))
    if getattr(args, "scf", None) is not None:
        res = tm.concordance_factors(trees=trees, n_quartets=args.scf, seed=args.seed)
    else:
        names = sorted(tm.names, key=tm.names.get)
        res = concordance.gene_concordance(tm.tree, trees, names=names, device=args.device,
                                           _prepared=True)
    current = with_lengths(tm.tree, tm.traversal.brlens)
    if getattr(args, "cf_table", None) is not None:
        cols = ("gCF", "gDF1", "gDF2", "gDFP", "gN", "sCF", "sDF1", "sDF2", "sN")
        with open(args.cf_table, "w") as fh:
            fh.write("\t".join(("id",) + cols + ("length",)) + "\n")
            for i, e in enumerate(res.internal):
                row = [str(int(e))]
                for c in cols:
                    v = getattr(res, c)
                    row.append("NA" if v is None else
                               str(int(v[i])) if c == "gN" else
                               concordance.format_value(float(v[i]), "%.10g"))
                row.append("{:.10g}".format(float(tm.traversal.brlens[res.pairs[int(e)]])))
                fh.write("\t".join(row) + "\n")
    return concordance.label_tree(current, res, prefix=support_labels)


def run_compare_trees(args, tm):
    """--compare-trees: the ``rf i:`` lines and the ``topologies =`` line of the run's final tree
    (tree 0) and the trees of the file."""
    from . import treeset
    with open(args.compare_trees) as fh:
        trees = [tm.tree] + [line.strip() for line in fh if line.strip()]
    names = sorted(tm.names, key=tm.names.get)
    res = treeset.compare(trees, names=names, device=args.device)
    lines = ["rf {}: {}".format(i, " ".join(str(int(d)) for d in row))
             for i, row in enumerate(res.rf)]
    metric = getattr(args, "tree_metric", None)
    if metric is not None:
        from .tree import with_lengths
        current = with_lengths(tm.tree, tm.traversal.brlens)
        d = treeset.distances([current] + trees[1:], metric, names=names, device=args.device)
        lines += ["{} {}: {}".format(metric, i, " ".join(repr(float(x)) for x in row))
                  for i, row in enumerate(d)]
    k = len(set(int(c) for c in treeset.topology_classes(res)))
    return lines + ["topologies = {} distinct of {}".format(k, len(trees))]


def run_test_trees(args, tm, first):
    """--test-trees: the table lines of ``topotest.topology_tests`` on `first` (the run's tree, or
    None) and the trees of the file."""
    from . import topotest
    with open(args.test_trees) as fh:
        trees = [line.strip() for line in fh if line.strip()]
    if first is not None:
        trees.insert(0, first)
    au = not getattr(args, "no_au", False)
    res = topotest.topology_tests(tm, trees, n_replicates=getattr(args, "test_replicates", 10000),
                                  scales=topotest.DEFAULT_SCALES if au else (), seed=args.seed,
                                  sweeps=max(args.optimise, 1))
    return topotest.format_table(res, au=au)


def run_simulate(args, out=None):
    """--simulate: FASTA of args.simulate columns down the tree under the model string."""
    from .simulation import simulate_alignment, states_to_sequences
    with open(args.tree) as fh:
        tree = parse_newick(fh.read())
    desc = parse_model_string(args.model)
    alphabet = A.PROTEIN if desc["subs_model"] in PROTEIN_MODELS else A.DNA
    names, states = simulate_alignment(tree, build_model(desc), build_rate_model(desc),
                                       args.simulate, seed=args.seed, device=args.device)
    seqs = states_to_sequences(states, alphabet)
    fh = open(args.output, "w") if args.output else (sys.stdout if out is None else out)
    try:
        for name, seq in zip(names, seqs):
            fh.write(">{}\n".format(name))
            for i in range(0, len(seq), 60):
                fh.write(seq[i:i + 60] + "\n")
    finally:
        if args.output:
            fh.close()
    return names, states


def run_distances(args, out=None):
    """--distances: the PHYLIP matrix of the alignment's pairwise ML distances."""
    from .distance import pairwise_distances, write_phylip
    aln = A.read_fasta(args.alignment)
    desc = parse_model_string(args.model)
    alphabet = A.PROTEIN if desc["subs_model"] in PROTEIN_MODELS else A.DNA
    names, D, V = pairwise_distances(aln, build_model(desc), build_rate_model(desc), alphabet,
                                     device=args.device)
    fh = open(args.output, "w") if args.output else (sys.stdout if out is None else out)
    try:
        write_phylip(names, D, fh)
    finally:
        if args.output:
            fh.close()
    return names, D, V


def read_clusters(path):
    """--lmap-clusters: four non-empty lines of taxon names, separated by blanks or commas."""
    with open(path) as fh:
        groups = [line.replace(",", " ").split() for line in fh if line.strip()]
    if len(groups) != 4:
        raise ValueError("{} holds {} lines of names, not four".format(path, len(groups)))
    return groups


def run_lmap(args, out=None):
    """--lmap: the ``lmap:`` lines of the alignment's likelihood map, and its table and SVG."""
    from . import lmap
    out = sys.stdout if out is None else out
    aln = A.read_fasta(args.alignment)
    desc = parse_model_string(args.model)
    alphabet = A.PROTEIN if desc["subs_model"] in PROTEIN_MODELS else A.DNA
    clusters = None
    if getattr(args, "lmap_clusters", None) is not None:
        clusters = read_clusters(args.lmap_clusters)
    res = lmap.likelihood_mapping(aln, build_model(desc), build_rate_model(desc),
                                  n_quartets=None if args.lmap == LMAP_DEFAULT else args.lmap,
                                  seed=args.seed, clusters=clusters,
                                  alphabet=alphabet, device=args.device)
    for line in lmap.report_lines(res):
        out.write(line + "\n")
    if getattr(args, "lmap_table", None) is not None:
        with open(args.lmap_table, "w") as fh:
            lmap.write_table(res, fh)
    if getattr(args, "lmap_svg", None) is not None:
        with open(args.lmap_svg, "w") as fh:
            lmap.write_svg(res, fh)
    return res


def main(argv=None):
    args = parse_cli(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as e:
        sys.stderr.write("ERROR: {}\n".format(e))
        return 1
    try:
        if getattr(args, "lmap", None) is not None:
            run_lmap(args)
        elif args.distances:
            run_distances(args)
        elif args.simulate is not None:
            run_simulate(args)
        else:
            run(args)
    except ValueError as e:
        sys.stderr.write("ERROR: {}\n".format(e))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
