"""Bootstrap support of distance trees on the CPU: the ABI is exported and bound,
every refused argument is refused before a device is touched, the restatement
(tests/boot_reference.py) keeps the rule's own properties, the labelling survives Newick, and the
CLI's --bootstrap argument rules."""
import ctypes

import numpy as np
import pytest

from conftest import has_gpu

import boot_reference as BR
import nj_reference as NR
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import bootstrap, nj, phy
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
from phylo_utils_amd.tree import parse_newick

BOOT_SYMBOLS = ("pu_boot_weights", "pu_boot_weights_device", "pu_boot_pair_counts",
                "pu_boot_distances", "pu_boot_distances_device", "pu_split_support",
                "pu_split_support_device", "pu_bootstrap_nj")
FAKE = ctypes.c_void_p(0x1000)
i32 = lambda x: np.asarray(x, dtype=np.int32)


def test_symbols_exported_and_bound():
    lib = N.lib()
    for s in BOOT_SYMBOLS:
        assert s in N.SIGNATURES, s
        assert hasattr(lib, s), s


def test_module_imports():
    import phylo_utils_amd
    assert phylo_utils_amd.bootstrap is bootstrap
    for f in ("bootstrap_weights", "bootstrap_distances", "split_support", "bootstrap_nj"):
        assert callable(getattr(bootstrap, f))
    assert callable(phylo_utils_amd.TreeModel.bootstrap_nj)


# ------------------------------------------------------------------ the resampling rule
W_CASES = {"unit": 37, "repeats and zeros": [3, 0, 1, 1, 0, 0, 7, 2, 0, 5],
           "one pattern": [9], "leading and trailing zeros": [0, 0, 4, 1, 0]}


@pytest.mark.parametrize("name", sorted(W_CASES))
def test_restatement_weights_sum_to_n_and_skip_zero_patterns(name):
    w = W_CASES[name]
    total = w if np.ndim(w) == 0 else int(np.sum(w))
    W = BR.weights(w, 5, seed=11)
    assert W.dtype == np.uint32 and W.shape == (5, total if np.ndim(w) == 0 else len(w))
    assert np.array_equal(W.sum(axis=1), np.full(5, total))
    if np.ndim(w):
        assert np.all(W[:, np.asarray(w) == 0] == 0)  # a zero-weight pattern is never drawn
        if len(w) > 1:
            assert len({row.tobytes() for row in W}) > 1


def test_restatement_replicates_are_addressed_by_their_number():
    w = [2, 5, 0, 1, 8, 3]
    big = BR.weights(w, 7, seed=5)
    for r in (0, 3, 6):
        assert np.array_equal(BR.weights(w, 1, seed=5, first_rep=r)[0], big[r])
    assert np.array_equal(BR.weights(w, 3, seed=5, first_rep=2), big[2:5])
    assert not np.array_equal(BR.weights(w, 7, seed=6), big)


def test_restatement_stream_is_apart_from_the_simulator():
    import sim_reference as SR
    j = np.arange(64)
    assert not np.any(BR.uniform(3, j, 2) == SR.uniform(3, j, 2))  # counter word 3 = 1, not 0
    u = BR.uniform(3, j, 2)
    assert np.all((u >= 0) & (u < 1))


# ------------------------------------------------------------------ split support
# ((0,1),2,(3,4)) and its neighbour by one NNI across the edge above (0,1)
T5 = i32([[0, 1], [2, 5], [3, 6]])
T5_NNI = i32([[0, 2], [1, 5], [3, 6]])
T4 = i32([[0, 1], [2, 4]])
T4_OTHER = i32([[0, 2], [1, 4]])


def test_reference_splits_and_the_tip0_rule():
    assert BR.splits(T4, 4) == [frozenset([2, 3])]            # {0, 1} holds tip 0
    assert BR.splits(T5, 5) == [frozenset([2, 3, 4]), frozenset([3, 4])]
    # one split written from either side: cluster {3, 4} and cluster {0, 1, 2}
    a = i32([[3, 4], [0, 1], [2, 6]])   # clusters {3,4}, {0,1}, ...
    b = i32([[0, 1], [2, 5], [3, 6]])   # clusters {0,1}, {0,1,2}, ...
    assert BR.splits(a, 5)[0] == BR.splits(b, 5)[1] == frozenset([3, 4])
    assert set(BR.splits(a, 5)) == set(BR.splits(b, 5))
    sup, n_ok = BR.split_support(a, [b])
    assert sup.tolist() == [1.0, 1.0] and n_ok == 1


@pytest.mark.parametrize("n", [4, 5, 9])
def test_reference_support_of_identical_trees_is_one(n):
    rng = np.random.default_rng(n)
    joins, root = BR.random_joins(rng, n)
    sup, n_ok = BR.split_support(joins, np.stack([joins] * 3))
    assert sup.shape == (n - 3,) and np.all(sup == 1.0) and n_ok == 3
    # agreement with the tree helpers: the same bipartitions as the Tree of these joins
    names = ["t%d" % i for i in range(n)]
    tree = nj.joins_to_tree(names, joins, np.ones((n - 2, 2)), root, 1.0)
    want = {frozenset(names[i] for i in s) for s in BR.splits(joins, n)}
    assert want == NR.bipartitions(tree)


def test_reference_support_after_one_nni():
    sup, n_ok = BR.split_support(T5, np.stack([T5, T5_NNI, T5, T5_NNI]))
    assert sup.tolist() == [0.5, 1.0] and n_ok == 4        # exactly one split is lost
    sup, n_ok = BR.split_support(T5, np.stack([T5, T5_NNI, T5, T5_NNI]), ok=[1, 0, 1, 1])
    assert sup.tolist() == [2.0 / 3.0, 1.0] and n_ok == 3
    assert BR.split_support(T4, [T4_OTHER])[0].tolist() == [0.0]
    sup, n_ok = BR.split_support(T4, [T4], ok=[0])
    assert n_ok == 0 and np.isnan(sup[0])
    # n = 9: an NNI across the edge above the first cluster of two tips that is joined to a third
    rng = np.random.default_rng(9)
    joins, _ = BR.random_joins(rng, 9)
    m = next(k for k in range(6) if np.any(joins[k] >= 9))
    c = int(joins[m].max())                     # the cluster joined at m, made at c - 9
    other = int(joins[m].min())
    swapped = joins.copy()
    x = int(joins[c - 9][1])
    swapped[c - 9][1] = other
    swapped[m] = sorted((x, c))
    assert len(set(BR.splits(swapped, 9)) ^ set(BR.splits(joins, 9))) == 2
    sup, _ = BR.split_support(joins, [swapped])
    assert sorted(sup.tolist()) == [0.0] + [1.0] * 5


# ------------------------------------------------------------------ labels
def test_labels_survive_newick():
    n = 9
    names = ["taxon %d" % i if i == 3 else "t%d" % i for i in range(n)]
    res = NR.nj(NR.perturbed_additive(5, n), "bionj")
    tree = nj.joins_to_tree(names, res["joins"], res["lens"], res["root"], res["root_len"])
    support = np.array([1.0, 0.994, 0.995, 0.5, 0.0, 0.337])
    assert bootstrap.label_tree(tree, names, res["joins"], support) is tree
    want = ["100", "99", "100", "50", "0", "34"]
    assert [bootstrap.support_label(s) for s in support] == want
    back = parse_newick(tree.as_newick())
    assert back.as_newick() == tree.as_newick()
    for t in (tree, back):
        inner = [x for x in t.seed_node.postorder() if not x.is_leaf() and x is not t.seed_node]
        labelled = {frozenset(l.label for l in x.leaves()): x.label for x in inner
                    if x.label is not None}
        assert sorted(labelled.values()) == sorted(want)
        for m, s in enumerate(BR.splits(res["joins"], n)):
            tips = frozenset(names[i] for i in s)
            key = tips if tips in labelled else frozenset(names) - tips
            assert labelled[key] == want[m]
    assert NR.robinson_foulds(tree, back) == 0
    # a TreeModel takes the labelled tree as it is
    from phylo_utils_amd.tree import Traversal, prepare_tree
    tr = Traversal(prepare_tree(back))
    assert tr.n_nodes == 2 * n - 2 and set(tr.names) == set(names)


# ------------------------------------------------------------------ CLI
def test_cli_bootstrap_argument_rules(tmp_path, capsys):
    fa = tmp_path / "x.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n>c\nAGGA\n>d\nAGGT\n")
    nwk = tmp_path / "t.nwk"
    nwk.write_text("(a:0.1,b:0.1,(c:0.1,d:0.1):0.1);")
    args = phy.parse_cli(["-s", str(fa), "--nj", "nj", "--bootstrap", "20", "--seed", "4"])
    phy.validate_args(args)
    assert args.bootstrap == 20 and args.seed == 4
    assert phy.parse_cli(["-s", str(fa), "--nj", "nj"]).bootstrap is None
    assert phy.main(["-s", str(fa), "-t", str(nwk), "--bootstrap", "10"]) == 1
    assert "--bootstrap needs --nj" in capsys.readouterr().err
    assert phy.main(["-s", str(fa), "--distances", "--bootstrap", "10"]) == 1
    assert "--bootstrap needs --nj" in capsys.readouterr().err
    for bad in ("0", "-3"):
        assert phy.main(["-s", str(fa), "--nj", "bionj", "--bootstrap", bad]) == 1
        assert "--bootstrap needs at least one replicate" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        phy.parse_cli(["-s", str(fa), "--nj", "nj", "--bootstrap", "many"])
    capsys.readouterr()


# ------------------------------------------------------------------ refused arguments
def _weights_args(kw):
    a = dict(device=0, seed=1, first=0, R=3, S=5, w=np.array([1.0, 0, 2, 3, 1]),
             out=np.zeros((3, 5), dtype=np.uint32))
    a.update(kw)
    return a


def _weights_host(**kw):
    a = _weights_args(kw)
    return N.lib().pu_boot_weights(a["device"], a["seed"], a["first"], a["R"], a["S"],
                                   N.ptr(a["w"]), N.ptr(a["out"]))


def _weights_device(**kw):
    """The _device form with made-up device addresses: only for calls it must refuse, which it
    does before any address is read."""
    a = _weights_args(kw)
    return N.lib().pu_boot_weights_device(a["device"], None, a["seed"], a["first"], a["R"], a["S"],
                                          None if a["w"] is None else FAKE,
                                          None if a["out"] is None else FAKE, a.get("ldw", a["S"]))


BAD_WEIGHTS = {
    "null output": dict(out=None), "no replicate": dict(R=0), "negative replicates": dict(R=-2),
    "no sites": dict(S=0), "negative first replicate": dict(first=-1),
    "replicate numbers past 2^32": dict(first=2 ** 32 - 2),
}
BAD_WEIGHTS_HOST = {
    "negative weight": dict(w=np.array([1.0, -1, 2, 3, 1])),
    "non-integer weight": dict(w=np.array([1.0, 0.5, 2, 3, 1])),
    "nan weight": dict(w=np.array([1.0, np.nan, 2, 3, 1])),
    "inf weight": dict(w=np.array([1.0, np.inf, 2, 3, 1])),
    "N = 0": dict(w=np.zeros(5)),
    "N = 2^31": dict(w=np.array([2.0 ** 30, 2.0 ** 30, 0, 0, 0])),
}


@pytest.mark.parametrize("name", sorted(BAD_WEIGHTS))
def test_bad_weight_calls_are_refused_without_a_device(name):
    assert _weights_host(**BAD_WEIGHTS[name]) == N.PU_E_ARG, name
    assert "pu_boot_weights:" in N.last_error()
    assert _weights_device(**BAD_WEIGHTS[name]) == N.PU_E_ARG, name
    assert "pu_boot_weights_device" in N.last_error()


@pytest.mark.parametrize("name", sorted(BAD_WEIGHTS_HOST))
def test_bad_weights_are_refused_by_the_host_form(name):
    assert _weights_host(**BAD_WEIGHTS_HOST[name]) == N.PU_E_ARG, name
    assert "pu_boot_weights:" in N.last_error()


def test_weight_row_stride_and_unit_range_are_checked():
    assert _weights_device(ldw=4) == N.PU_E_ARG
    assert "row stride" in N.last_error()
    unit = dict(w=None, S=2 ** 31, out=np.zeros(1, dtype=np.uint32))  # unit weights: N = n_sites
    assert _weights_host(**unit) == N.PU_E_ARG and _weights_device(**unit) == N.PU_E_ARG


def _valid(n_taxa=4, S=10, R=3):
    """Keyword arguments of a valid pu_boot_distances / pu_bootstrap_nj call (DNA, GTR + G4)."""
    model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    table, _ = A.code_table(A.DNA)
    ev, el, iv = model.engine_eigen()
    rm = GammaRateModel(4, 0.5)
    rng = np.random.default_rng(1)
    n = n_taxa
    return dict(device=0, method=0, K=4, C=4, n_codes=len(table), table=N.f64(table), ev=ev, el=el,
                iv=iv, pi=N.f64(model.freqs), r=N.f64(rm.rates), q=N.f64(rm.weights),
                codes=rng.integers(0, len(table), (n, S)).astype(np.uint8), n_taxa=n, S=S,
                w=np.ones(S), W=np.ones((R, S), dtype=np.uint32), R=R, seed=3,
                n_pairs=n * (n - 1) // 2, pairs=None, lo=1e-5, hi=10.0, tol=1e-10, max_iter=50,
                out=np.zeros((R, 8, 5)), counts=np.zeros((R, 8, len(table), len(table))),
                joins=np.zeros((n - 2, 2), dtype=np.int32), lens=np.zeros((n - 2, 2)),
                root=np.zeros(2, dtype=np.int32), root_len=np.zeros(1), support=np.zeros(n),
                n_ok=np.zeros(1, dtype=np.int32), ld=S, ldw=S, ldd=n, D=None)


def _model(a):
    return (a["K"], a["C"], a["n_codes"], N.ptr(a["table"]), N.ptr(a["ev"]), N.ptr(a["el"]),
            N.ptr(a["iv"]), N.ptr(a["pi"]), N.ptr(a["r"]), N.ptr(a["q"]))


def _call_counts(a):
    return N.lib().pu_boot_pair_counts(a["device"], N.ptr(a["codes"]), a["n_taxa"], a["S"],
                                       a["n_codes"], N.ptr(a["W"]), a["R"], a["n_pairs"],
                                       N.ptr(a["pairs"]), N.ptr(a["counts"]))


def _call_dist(a):
    return N.lib().pu_boot_distances(a["device"], *_model(a), N.ptr(a["codes"]), a["n_taxa"],
                                     a["S"], N.ptr(a["W"]), a["R"], a["n_pairs"],
                                     N.ptr(a["pairs"]), a["lo"], a["hi"], a["tol"], a["max_iter"],
                                     N.ptr(a["out"]))


def _call_dist_device(a):
    fake = lambda k: None if a[k] is None else FAKE
    return N.lib().pu_boot_distances_device(
        a["device"], None, *_model(a), fake("codes"), a["ld"], a["n_taxa"], a["S"], fake("W"),
        a["ldw"], a["R"], a["n_pairs"], N.ptr(a["pairs"]), a["lo"], a["hi"], a["tol"],
        a["max_iter"], fake("out"), fake("D"), a["ldd"])


def _call_fused(a):
    return N.lib().pu_bootstrap_nj(
        a["device"], a["method"], *_model(a), N.ptr(a["codes"]), a["n_taxa"], a["S"],
        N.ptr(a["w"]), a["seed"], a["R"], a["lo"], a["hi"], a["tol"], a["max_iter"],
        N.ptr(a["joins"]), N.ptr(a["lens"]), N.ptr(a["root"]), N.ptr(a["root_len"]),
        N.ptr(a["support"]), N.ptr(a["n_ok"]), None, None)


BAD_SHAPE = {   # refused by every call that takes codes and W
    "null codes": dict(codes=None), "null W": dict(W=None), "no replicate": dict(R=0),
    "one taxon": dict(n_taxa=1, n_pairs=0), "no sites": dict(S=0),
    "no codes": dict(n_codes=0), "33 codes": dict(n_codes=33),
    "pair out of range": dict(pairs=i32([[0, 4]]), n_pairs=1),
    "i == j": dict(pairs=i32([[1, 1]]), n_pairs=1),
    "pair count without a list": dict(n_pairs=2),
}
BAD_MODEL = {
    "null table": dict(table=None), "null evecs": dict(ev=None), "null rates": dict(r=None),
    "K = 3": dict(K=3), "no category": dict(C=0), "too many categories": dict(C=65),
    "lo = 0": dict(lo=0.0), "lo > hi": dict(lo=2.0, hi=1.0), "tol = 0": dict(tol=0.0),
    "max_iter < 0": dict(max_iter=-1),
}


@pytest.mark.parametrize("name", sorted(BAD_SHAPE))
def test_bad_shapes_are_refused_without_a_device(name):
    a = dict(_valid(), **BAD_SHAPE[name])
    assert _call_counts(a) == N.PU_E_ARG, name
    assert "pu_boot_pair_counts" in N.last_error()
    assert _call_dist(a) == N.PU_E_ARG, name
    assert "pu_boot_distances" in N.last_error()
    assert _call_dist_device(a) == N.PU_E_ARG, name
    assert "pu_boot_distances_device" in N.last_error()


@pytest.mark.parametrize("name", sorted(BAD_MODEL))
def test_bad_models_are_refused_without_a_device(name):
    a = dict(_valid(), **BAD_MODEL[name])
    assert _call_dist(a) == N.PU_E_ARG, name
    assert _call_dist_device(a) == N.PU_E_ARG, name
    assert _call_fused(a) == N.PU_E_ARG, name
    assert "pu_bootstrap_nj" in N.last_error()


def test_null_outputs_bad_codes_and_bad_replicate_weights_are_refused():
    assert _call_counts(dict(_valid(), counts=None)) == N.PU_E_ARG
    assert _call_dist(dict(_valid(), out=None)) == N.PU_E_ARG
    assert _call_dist_device(dict(_valid(), out=None)) == N.PU_E_ARG
    a = _valid()
    a["codes"][2, 7] = a["n_codes"]
    for f in (_call_counts, _call_dist, _call_fused):
        assert f(a) == N.PU_E_ARG
        assert "taxon 2 site 7" in N.last_error()
    a = _valid()
    a["W"][1] = 0     # replicate 1 resamples nothing: N = 0
    for f in (_call_counts, _call_dist):
        assert f(a) == N.PU_E_ARG
        assert "replicate 1" in N.last_error()
    a = _valid()
    a["W"][2, :2] = 2 ** 30   # N = 2^31 + 8
    assert _call_counts(a) == N.PU_E_ARG


def test_device_form_strides_and_matrix_rules():
    assert _call_dist_device(dict(_valid(), ld=9)) == N.PU_E_ARG
    assert _call_dist_device(dict(_valid(), ldw=9)) == N.PU_E_ARG
    assert "row strides" in N.last_error()
    assert _call_dist_device(dict(_valid(), D=1, ldd=3)) == N.PU_E_ARG
    assert _call_dist_device(dict(_valid(), D=1, pairs=i32([[0, 1]]), n_pairs=1)) == N.PU_E_ARG
    assert "the matrices need all pairs" in N.last_error()


BAD_FUSED = {
    "null codes": dict(codes=None), "null joins": dict(joins=None), "null lens": dict(lens=None),
    "null root": dict(root=None), "null root length": dict(root_len=None),
    "null support": dict(support=None), "null n_ok": dict(n_ok=None),
    "two taxa": dict(n_taxa=2), "too many taxa": dict(n_taxa=8193),
    "method 2": dict(method=2), "no replicate": dict(R=0), "no sites": dict(S=0),
    "33 codes": dict(n_codes=33),
    "negative weight": dict(w=np.r_[-1.0, np.ones(9)]),
    "non-integer weight": dict(w=np.r_[0.25, np.ones(9)]),
    "nan weight": dict(w=np.r_[np.nan, np.ones(9)]),
    "N = 0": dict(w=np.zeros(10)), "N = 2^31": dict(w=np.r_[2.0 ** 31, np.zeros(9)]),
}


@pytest.mark.parametrize("name", sorted(BAD_FUSED))
def test_bad_fused_calls_are_refused_without_a_device(name):
    a = dict(_valid(), **BAD_FUSED[name])
    assert _call_fused(a) == N.PU_E_ARG, name
    assert "pu_bootstrap_nj" in N.last_error()


def _support_args(kw):
    a = dict(n=5, R=2, ref=T5, ref_root=i32([7, 4]), joins=np.stack([T5, T5_NNI]),
             roots=i32([[7, 4], [7, 4]]), ok=None, support=np.zeros(2),
             n_ok=np.zeros(1, dtype=np.int32))
    a.update(kw)
    return a


def _support_host(**kw):
    a = _support_args(kw)
    p = lambda k: N.ptr(a[k])
    return N.lib().pu_split_support(0, a["n"], a["R"], p("ref"), p("ref_root"), p("joins"),
                                    p("roots"), p("ok"), p("support"), p("n_ok"))


def _support_device(**kw):
    """The _device form with made-up device addresses: only for calls it must refuse."""
    a = _support_args(kw)
    f = lambda k: None if a[k] is None else FAKE
    return N.lib().pu_split_support_device(0, None, a["n"], a["R"], f("ref"), f("ref_root"),
                                           f("joins"), f("roots"), f("ok"), f("support"),
                                           f("n_ok"))


BAD_SUPPORT = {
    "null reference": dict(ref=None), "null reference root": dict(ref_root=None),
    "null joins": dict(joins=None), "null roots": dict(roots=None),
    "null support": dict(support=None), "null n_ok": dict(n_ok=None),
    "n = 2": dict(n=2), "n above the cap": dict(n=8193), "no replicate": dict(R=0),
}


@pytest.mark.parametrize("name", sorted(BAD_SUPPORT))
def test_bad_support_calls_are_refused_without_a_device(name):
    assert _support_host(**BAD_SUPPORT[name]) == N.PU_E_ARG, name
    assert "pu_split_support:" in N.last_error()
    assert _support_device(**BAD_SUPPORT[name]) == N.PU_E_ARG, name
    assert "pu_split_support_device" in N.last_error()


def test_joins_that_are_no_tree_are_refused_by_the_host_form():
    for bad in (i32([[0, 1], [0, 5], [3, 6]]),      # tip 0 joined twice
                i32([[0, 1], [2, 6], [3, 5]]),      # cluster 6 before it exists
                i32([[0, -1], [2, 5], [3, 6]])):
        assert _support_host(ref=bad) == N.PU_E_ARG
        assert "reference tree 0" in N.last_error()
        assert _support_host(joins=np.stack([T5, bad])) == N.PU_E_ARG
        assert "replicate tree 1" in N.last_error()


def test_python_argument_checks():
    with pytest.raises(ValueError):
        bootstrap.bootstrap_weights(10, 0)
    with pytest.raises(ValueError):
        bootstrap.split_support((T5, i32([7, 4])), (T4[None], i32([[5, 3]])))
    with pytest.raises(ValueError):
        bootstrap.split_support((T5, i32([7, 4])), (T5[None], i32([[7, 4]])), ok=[1, 1])
    with pytest.raises(ValueError):
        bootstrap.bootstrap_pair_counts(np.zeros((3, 4), dtype=np.uint8), 4,
                                        np.ones((2, 5), dtype=np.uint32))
    table, _ = A.code_table(A.DNA)
    codes = np.zeros((2, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        bootstrap.bootstrap_nj((codes, table), SM.GTR(), n_replicates=5)   # two taxa
    with pytest.raises(ValueError):
        bootstrap.bootstrap_nj((np.zeros((4, 4), dtype=np.uint8), table), SM.GTR(),
                               method="upgma")


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_valid_calls_fail_loudly_without_a_device():
    for f in (_call_counts, _call_dist, _call_fused):
        rc = f(_valid())
        assert rc != 0 and rc != N.PU_E_ARG
    assert _weights_host() not in (0, N.PU_E_ARG)
    assert _support_host() not in (0, N.PU_E_ARG)
    with pytest.raises(N.PhyloHipError):
        bootstrap.bootstrap_weights(10, 2)
    with pytest.raises(N.PhyloHipError):
        bootstrap.split_support((T5, i32([7, 4])), (T5[None], i32([[7, 4]])))
