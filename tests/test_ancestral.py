"""Host side of the ancestral reconstruction (phylo_utils_amd.ancestral): the CPU
restatement the device tests compare with (tests/ancestral_reference.py) against plain
enumeration, the new C symbols, the category limit and the Python refusals.  No device."""
import numpy as np
import pytest

import ancestral_reference as R

from phylo_utils_amd import TreeModel, ancestral, phy
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
from phylo_utils_amd.tree import Traversal, prepare_tree

FIVE = "((a:0.11,b:0.22):0.07,(c:0.13,d:0.31):0.09,e:0.17);"


def _five_taxa():
    """(traversal, tips {node: [40][4]}, eigen dict, pattern weights): 40 columns over the
    IUPAC codes, no column all gaps."""
    rng = np.random.default_rng(7)
    letters = np.array(list("ACGTACGTACGTRYMKWSBDHVN-"))
    cols = rng.choice(len(letters), size=(5, 40))
    cols[0] = rng.choice(4, size=40)  # one unambiguous row: no all-gap column
    tr = Traversal(prepare_tree(FIVE))
    tips = {tr.names[n]: A.seq_to_partials("".join(letters[cols[i]]), A.DNA)
            for i, n in enumerate("abcde")}
    assert any((v.sum(axis=1) > 1).any() for v in tips.values())
    e = R.eigen(SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(3, 0.6))
    return tr, tips, e, rng.integers(1, 5, size=40).astype(float)


def test_restatement_equals_enumeration(oracle_mod):
    """The yardstick itself: posteriors from two resident partials per node, walked as the
    library walks them, equal the sums over all 4^3 joint assignments of the three internal
    nodes (K = 4, C = 3) to 1e-12; every node's lnL is the tree's."""
    tr, tips, e, sw = _five_taxa()
    got = R.sweep(oracle_mod, tips, tr, e, site_weights=sw)
    ref = R.brute_force(oracle_mod, tips, tr, e)
    internal = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    assert sorted(got["nodes"].tolist()) == internal and len(internal) == 3
    for n, q in zip(got["nodes"], got["posteriors"]):
        err = np.abs(q - ref["posteriors"][int(n)]).max()
        assert err <= 1e-12, (n, err)
        assert np.abs(q.sum(axis=1) - 1).max() <= 1e-12
    assert np.abs(got["cat_post"] - ref["cat_post"]).max() <= 1e-12
    assert np.abs(got["cat_post"].sum(axis=1) - 1).max() <= 1e-12
    lnl, _ = oracle_mod.tree_lnl(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge,
                                 tr.root_length(), e["evecs"], e["evals"], e["ivecs"], e["freqs"],
                                 e["rates"], e["weights"], site_weights=sw, n_nodes=tr.n_nodes)
    for v in got["node_lnl"]:
        assert abs(v - lnl) <= 1e-12 * abs(lnl), (v, lnl)
    assert abs(np.dot(sw, ref["lnl"]) - lnl) <= 1e-12 * abs(lnl)


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_device_cases_on_the_restatement(oracle_mod, case):
    """The cases tests/test_gpu_ancestral.py runs, on the restatement alone: every internal node
    once, every node's lnL the tree's, posteriors that sum to 1, and at most 1 % of the (node,
    site) pairs with a MAP state too close to call (the cap of the device test's map_state
    check).  The caterpillar's deep nodes carry scalers that differ between the categories."""
    prob = R.problem(case)
    tr, e, ref = R.restate(oracle_mod, prob)
    internal = sorted(set(int(p) for p in tr.postorder_traversal[:, 0]))
    assert sorted(ref["nodes"].tolist()) == internal
    assert len(internal) == len(prob["names"]) - 2
    assert np.abs(ref["node_lnl"] - ref["lnl"]).max() <= 1e-10 * abs(ref["lnl"])
    assert np.abs(ref["posteriors"].sum(axis=2) - 1).max() <= 1e-12
    assert np.abs(ref["cat_post"].sum(axis=1) - 1).max() <= 1e-12
    assert (~R.decided(ref["posteriors"])).mean() <= 0.01
    if "caterpillar" in case:
        sig = ref["sigma"]
        assert (sig.max(axis=2) != sig.min(axis=2)).any()


def test_symbols_exported_and_bound():
    lib = N.lib()
    for name in ("pu_ancestral_max_cat", "pu_ancestral_edge", "pu_ancestral_sweep",
                 "pu_site_rates", "pu_ancestral_kernel_ms"):
        assert name in N.SIGNATURES
        assert getattr(lib, name).argtypes is not None
    for name in ("ancestral_states", "ancestral_sequences", "site_rates"):
        assert callable(getattr(TreeModel, name))
        assert callable(getattr(ancestral, name))


def test_ancestral_max_cat():
    for K in (2, 4, 20):
        assert N.lib().pu_ancestral_max_cat(K) >= 8
        assert ancestral.ancestral_max_cat(K) == N.lib().pu_ancestral_max_cat(K)
    assert N.lib().pu_ancestral_max_cat(7) < 0
    with pytest.raises(ValueError):
        ancestral.ancestral_max_cat(7)


def test_refuses_what_it_cannot_do():
    tm = TreeModel(keep_partials=False)
    for call in (tm.ancestral_states, tm.site_rates, lambda: tm.ancestral_sequences(A.DNA)):
        with pytest.raises(ValueError, match="keep_partials"):
            call()
    tm = TreeModel()
    tm.substitution_model = type("M", (), {"reversible": False})()
    for call in (tm.ancestral_states, tm.site_rates):
        with pytest.raises(ValueError, match="reversible"):
            call()
    tm = TreeModel()
    tm.substitution_model = type("M", (), {"reversible": True})()
    tm.set_alignment_codes([[0, 1], [1, 0], [0, 0]], [[1.0, 0.0], [0.0, 1.0]], "abc")
    with pytest.raises(ValueError, match="4 taxa"):
        tm.ancestral_states()
    tm.ascbias = True
    with pytest.raises(ValueError, match="ascertainment"):
        tm.site_rates()


def test_cli_options(tmp_path, capsys):
    t = tmp_path / "t.nwk"
    t.write_text(FIVE)
    fa = tmp_path / "a.fa"
    fa.write_text("".join(">%s\nACGT\n" % n for n in "abcde"))
    args = phy.parse_cli(["-t", str(t), "-s", str(fa)])
    assert args.ancestral is None and args.site_rates is None
    args = phy.parse_cli(["-t", str(t), "-s", str(fa), "--ancestral", "x.fa", "--site-rates",
                          "r.tsv"])
    assert (args.ancestral, args.site_rates) == ("x.fa", "r.tsv")
    phy.validate_args(args)
    assert phy.main(["-t", str(t), "--simulate", "10", "--ancestral", "x.fa"]) == 1
    assert "exclude" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--distances", "--site-rates", "r.tsv"]) == 1
    assert "exclude" in capsys.readouterr().err
