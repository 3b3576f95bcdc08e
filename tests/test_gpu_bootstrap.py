"""Bootstrap support on the device (pu_bootstrap.hip) against the restatement of its
specification (tests/boot_reference.py) and against the calls it must compose: every comparison
is exact -- the weights and counts are integers, the distances reuse the pair calls' Newton
kernel on bitwise equal counts, the trees reuse pu_nj."""
import functools

import numpy as np
import pytest

import boot_reference as BR
import dist_reference as DR
import nj_reference as NR
from twostate import TwoState
from phylo_utils_amd import TreeModel
from phylo_utils_amd import alignment as A
from phylo_utils_amd import bootstrap, distance, nj, phy, simulation
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
from phylo_utils_amd.tree import parse_newick

pytestmark = pytest.mark.gpu

DNA_TABLE, _ = A.code_table(A.DNA)
AA_TABLE, _ = A.code_table(A.PROTEIN)
BIN_TABLE, _ = A.code_table(A.BINARY)

# 12 taxa, every internal branch 0.1 (the root edge 0.05 + 0.05)
NEWICK12 = ("((((t0:0.1,t1:0.1):0.1,(t2:0.1,t3:0.1):0.1):0.1,((t4:0.1,t5:0.1):0.1,t6:0.15):0.1):0.05,"
            "(((t7:0.1,t8:0.1):0.1,t9:0.15):0.1,(t10:0.1,t11:0.1):0.1):0.05);")
NEWICK9 = "(((a:0.1,b:0.2):0.1,(c:0.1,d:0.3):0.2):0.1,((e:0.2,f:0.1):0.1,(g:0.1,(h:0.2,i:0.1):0.1):0.2):0.1);"
NEWICK6 = "(((a:0.2,b:0.3):0.2,c:0.3):0.1,((d:0.2,e:0.4):0.2,f:0.3):0.1);"


def gtr():
    return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)


def state_codes(table):
    K = table.shape[1]
    return np.array([int(np.where((table == np.eye(K)[k]).all(1))[0][0]) for k in range(K)])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------- weights
def pattern_weights(rng, S):
    """Integer weights with repeats and zeros (never all zero)."""
    w = rng.integers(0, 4, S).astype(np.float64)
    w[rng.integers(0, S)] = 5.0
    return w


@pytest.mark.parametrize("S", [1, 37, 128, 129, 1000])
def test_weights_equal_the_restatement(S):
    rng = np.random.default_rng(S)
    for w in (S, pattern_weights(rng, S)):
        got = bootstrap.bootstrap_weights(w, 3, seed=S + 1)
        np.testing.assert_array_equal(got, BR.weights(w, 3, seed=S + 1))
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(bootstrap.bootstrap_weights(w, 3, seed=S + 1), got)


@pytest.mark.parametrize("R", [1, 3, 64, 65, 130])
def test_weights_of_many_replicates_and_a_later_start(R):
    w = pattern_weights(np.random.default_rng(R), 90)
    want = BR.weights(w, R, seed=2 ** 40 + 3, first_rep=17)
    got = bootstrap.bootstrap_weights(w, R, seed=2 ** 40 + 3, first_replicate=17)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.sum(axis=1), np.full(R, int(w.sum())))
    assert np.all(got[:, w == 0] == 0)
    # a row is addressed by its replicate number, whatever else the call asked for
    one = bootstrap.bootstrap_weights(w, 1, seed=2 ** 40 + 3, first_replicate=17 + R - 1)
    np.testing.assert_array_equal(one[0], got[R - 1])


# ---------------------------------------------------------------------------- pair counts
def check_counts(codes, n_codes, W, pairs=None):
    got = bootstrap.bootstrap_pair_counts(codes, n_codes, W, pairs)
    for r in range(len(W)):
        want = DR.counts(codes, n_codes, W[r].astype(np.float64), pairs)
        np.testing.assert_array_equal(got[r], want, err_msg="replicate %d" % r)
    return got


# the tile is 64 replicates (32 for 32 codes), a workgroup takes up to 4 pairs, sites come in
# chunks of 128 and in segments when the pairs and tiles alone do not fill the device
@pytest.mark.parametrize("n_codes", [3, 15, 21, 32])
@pytest.mark.parametrize("n_taxa", [2, 5, 17])
def test_pair_counts_are_exact(n_codes, n_taxa):
    rng = np.random.default_rng(100 * n_codes + n_taxa)
    S, R = (700, 70) if n_taxa < 17 else (300, 33)
    codes = rng.integers(0, n_codes, (n_taxa, S)).astype(np.uint8)
    W = BR.weights(pattern_weights(rng, S), R, seed=n_codes)
    check_counts(codes, n_codes, W)


def test_pair_counts_explicit_pairs_and_chunks(monkeypatch):
    rng = np.random.default_rng(8)
    n_codes = len(DNA_TABLE)
    codes = rng.integers(0, n_codes, (6, 515)).astype(np.uint8)
    W = BR.weights(515, 5, seed=1)
    pairs = [(3, 0), (0, 3), (5, 4), (0, 1), (3, 0), (2, 5), (1, 4)]  # a swap and a repeat
    got = check_counts(codes, n_codes, W, pairs)
    np.testing.assert_array_equal(got[:, 0], got[:, 1].transpose(0, 2, 1))
    np.testing.assert_array_equal(got[:, 0], got[:, 4])
    np.testing.assert_array_equal(
        got, np.stack([distance.pair_counts(codes, n_codes, W[r].astype(np.float64), pairs)
                       for r in range(5)]))
    whole = bootstrap.bootstrap_pair_counts(codes, n_codes, W)
    for chunk in ("1", "4", "7"):
        monkeypatch.setenv("PU_DIST_CHUNK", chunk)
        np.testing.assert_array_equal(bits(bootstrap.bootstrap_pair_counts(codes, n_codes, W)),
                                      bits(whole))
        np.testing.assert_array_equal(
            bits(bootstrap.bootstrap_pair_counts(codes, n_codes, W, pairs)), bits(got))
    # chunks of replicates (whole tiles by default; PU_BOOT_REP_CHUNK caps them), alone and
    # together with chunks of pairs
    for rep_chunk, pair_chunk in (("1", None), ("3", None), ("4", "4"), ("2", "1")):
        monkeypatch.setenv("PU_BOOT_REP_CHUNK", rep_chunk)
        if pair_chunk is None:
            monkeypatch.delenv("PU_DIST_CHUNK", raising=False)
        else:
            monkeypatch.setenv("PU_DIST_CHUNK", pair_chunk)
        np.testing.assert_array_equal(bits(bootstrap.bootstrap_pair_counts(codes, n_codes, W)),
                                      bits(whole))
        np.testing.assert_array_equal(
            bits(bootstrap.bootstrap_pair_counts(codes, n_codes, W, pairs)), bits(got))


def test_distances_do_not_depend_on_the_chunks(monkeypatch):
    codes, table, names, model, rm = simulated("dna")
    R = 70   # two tiles of replicates
    W = bootstrap.bootstrap_weights(codes.shape[1], R, seed=4)
    whole = bootstrap.evaluate_replicates(codes, table, W, model, rm)
    for rep_chunk, pair_chunk in (("64", None), ("5", "7"), ("1", "36")):
        monkeypatch.setenv("PU_BOOT_REP_CHUNK", rep_chunk)
        if pair_chunk is not None:
            monkeypatch.setenv("PU_DIST_CHUNK", pair_chunk)
        got = bootstrap.evaluate_replicates(codes, table, W, model, rm)
        np.testing.assert_array_equal(bits(got), bits(whole))


# ---------------------------------------------------------------------------- distances
@functools.lru_cache(maxsize=None)
def simulated(kind):
    """(codes, table, names, model, rate model) of an alignment simulated down a fixed tree."""
    if kind == "dna":
        newick, model, table, S = NEWICK9, gtr(), DNA_TABLE, 300
    elif kind == "protein":
        newick, model, table, S = NEWICK6, SM.LG(), AA_TABLE, 200
    elif kind == "binary":
        newick, model, table, S = NEWICK6, TwoState(), BIN_TABLE, 250
    else:
        newick, model, table, S = NEWICK12, gtr(), DNA_TABLE, 2000
    rm = GammaRateModel(4, 0.5)
    names, states = simulation.simulate_alignment(newick, model, rm, S, seed=2024)
    return state_codes(table)[states].astype(np.uint8), table, list(names), model, rm


@pytest.mark.parametrize("kind", ["dna", "protein", "binary"])
def test_replicate_distances_are_bitwise_the_weighted_pair_call(kind):
    codes, table, names, model, rm = simulated(kind)
    R = 5
    _, D, out5, W = bootstrap.bootstrap_distances((codes, table, names), model, rm,
                                                  n_replicates=R, seed=9, return_details=True)
    assert out5.shape == (R, len(codes) * (len(codes) - 1) // 2, 5)
    np.testing.assert_array_equal(W.sum(axis=1), np.full(R, codes.shape[1]))
    pats, pw, _ = A.compress_codes(codes, len(table), 0)  # what the replicates resampled
    for r in range(R):
        np.testing.assert_array_equal(W[r], BR.weights(pw, 1, seed=9, first_rep=r)[0])
        _, Dr, _, o = distance.pairwise_distances((pats, table, names), model, rm,
                                                  weights=W[r].astype(np.float64),
                                                  return_details=True)
        np.testing.assert_array_equal(bits(out5[r]), bits(o), err_msg="replicate %d" % r)
        np.testing.assert_array_equal(bits(D[r]), bits(Dr))
    assert np.all(np.isfinite(D))


# ---------------------------------------------------------------------------- trees
@pytest.mark.parametrize("method", ["nj", "bionj"])
def test_fused_call_equals_the_composition(method):
    codes, table, names, model, rm = simulated("dna")
    R = 7
    tree, support, n_ok, (rep_joins, rep_roots) = bootstrap.bootstrap_nj(
        (codes, table, names), model, rm, n_replicates=R, seed=31, method=method,
        return_replicates=True)
    # the separate calls
    _, D0, _ = distance.pairwise_distances((codes, table, names), model, rm)
    ref = nj.nj_joins(D0, method)
    _, D = bootstrap.bootstrap_distances((codes, table, names), model, rm, n_replicates=R,
                                         seed=31)
    reps = nj.nj_joins(D, method)
    np.testing.assert_array_equal(rep_joins, reps[0])
    np.testing.assert_array_equal(rep_roots, reps[2])
    ok = np.isfinite(D).all(axis=(1, 2))
    sup, nok = bootstrap.split_support(ref, reps, ok)
    np.testing.assert_array_equal(bits(support), bits(sup))
    assert n_ok == nok == R
    want = nj.joins_to_tree(names, ref[0], ref[1], ref[2], ref[3])
    bootstrap.label_tree(want, names, ref[0], sup)
    assert tree.as_newick() == want.as_newick()
    # the reference tree's lengths bit for bit (ref_lens_out, ref_root_len_out), not as printed
    lengths = lambda t: [np.nan if x.length is None else x.length for x in t.seed_node.postorder()]
    np.testing.assert_array_equal(bits(lengths(tree)), bits(lengths(want)))
    assert sorted(bits(lengths(tree)).tolist()) == sorted(
        bits(list(ref[1].ravel()) + [ref[3], 0.0, np.nan]).tolist())
    # and the restatement of the comparison
    sup_ref, nok_ref = BR.split_support(ref[0], reps[0], ok)
    np.testing.assert_array_equal(support, sup_ref)
    assert nok_ref == R
    assert np.all((support >= 0) & (support <= 1))


# ---------------------------------------------------------------------------- support
@pytest.mark.parametrize("n", [4, 5, 64, 65, 130])
@pytest.mark.parametrize("R", [1, 65])
def test_split_support_equals_the_restatement(n, R):
    rng = np.random.default_rng(1000 * n + R)
    ref = BR.random_joins(rng, n)
    trees = []
    for r in range(R):
        kind = rng.integers(0, 3)
        if kind == 0:
            trees.append(ref)                       # the reference itself
        elif kind == 1:                              # the reference with its first joins redone
            joins = ref[0].copy()
            k = int(rng.integers(0, n - 2))
            joins[k] = joins[k][::-1]
            trees.append((joins, ref[1]))
        else:
            trees.append(BR.random_joins(rng, n))
    joins = np.stack([t[0] for t in trees])
    roots = np.stack([t[1] for t in trees])
    for ok in (None, rng.integers(0, 2, R)):
        got, n_ok = bootstrap.split_support(ref, (joins, roots), ok)
        want, n_want = BR.split_support(ref[0], joins, ok)
        assert n_ok == n_want == (R if ok is None else int(np.count_nonzero(ok)))
        np.testing.assert_array_equal(got, want)   # NaN == NaN here: n_ok = 0
    if R > 1:
        same, _ = bootstrap.split_support(ref, (np.stack([ref[0]] * R), np.stack([ref[1]] * R)))
        assert np.all(same == 1.0)


# ---------------------------------------------------------------------------- end to end
def test_tree_model_bootstrap_recovers_a_well_supported_tree():
    """12 taxa x 2000 DNA sites simulated (seed 2024) down NEWICK12, GTR + G4(0.5), every internal
    branch 0.1; 100 replicates, bootstrap seed 7.  The numpy pipeline alone (sim_reference.walk,
    dist_reference counts and brentq optima, nj_reference.nj, boot_reference) gives RF = 0 and a
    smallest support of 1.0 on this shape."""
    codes, table, names, model, rm = simulated("end to end")
    tm = TreeModel()
    tm.set_alignment_codes(codes, table, names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tree, support, n_ok = tm.bootstrap_nj(100, seed=7)
    assert n_ok == 100 and support.shape == (9,)
    assert NR.robinson_foulds(tree, parse_newick(NEWICK12)) == 0
    assert support.min() >= 0.95, support
    back = parse_newick(tree.as_newick())
    labels = [x.label for x in back.seed_node.postorder()
              if not x.is_leaf() and x.label is not None]
    assert sorted(labels) == sorted(bootstrap.support_label(s) for s in support)
    tm.initialise()
    assert np.isfinite(tm.likelihood())


def test_cli_writes_support_labels(tmp_path, capsys):
    codes, table, names, _, _ = simulated("dna")
    inv = {int(c): "ACGT"[k] for k, c in enumerate(state_codes(table))}
    fa = tmp_path / "aln.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, "".join(inv[int(c)] for c in row))
                          for n, row in zip(names, codes)))
    out = tmp_path / "tree.nwk"
    rc = phy.main(["-s", str(fa), "-m", "GTR{1.0,2.0,1.0,1.0,2.0,1.0}+G4{0.5}", "--nj", "bionj",
                   "--bootstrap", "20", "--seed", "3", "-o", str(out)])
    assert rc == 0
    assert capsys.readouterr().out.startswith("lnL = ")
    tree = parse_newick(out.read_text())
    assert sorted(x.label for x in tree.leaf_nodes()) == sorted(names)
    labels = [x.label for x in tree.seed_node.postorder()
              if not x.is_leaf() and x.label is not None]
    assert len(labels) == len(names) - 3
    assert all(0 <= int(x) <= 100 for x in labels)
