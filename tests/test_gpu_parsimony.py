"""Fitch parsimony on the device (pu_parsimony.hip) against the numpy restatement
of the rule (tests/parsimony_reference.py): every result is an integer and every comparison is
exact equality -- tree lengths with their per-pattern and per-edge counts, insertion lengths,
stepwise-addition trees, chunking, the argument refusals and the way through TreeModel."""
import functools

import numpy as np
import pytest

import parsimony_reference as PR
from phylo_utils_amd import TreeModel, parsimony
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel

pytestmark = pytest.mark.gpu

TAXA = (3, 4, 5, 17, 65)
# 1; one wave less one, one wave, one more; a workgroup's tile of 256 and one more; three tiles,
# so that several tiles add to one sum
PATTERNS = (1, 63, 64, 65, 257, 600)
STATES = (2, 4, 20)


def names_of(n):
    return ["t%d" % i for i in range(n)]


@functools.lru_cache(maxsize=None)
def alignment(n, P, K):
    rng = np.random.default_rng(7 * n + 13 * P + K)
    codes, table = PR.random_alignment(rng, n, P, K)
    codes.setflags(write=False)
    return codes, table, PR.tip_sets(codes, table)


@functools.lru_cache(maxsize=None)
def weights(kind, n, P):
    """None; all ones; integers with a zero and one value of at least 2^32 / n_taxa, which
    wraps a 32-bit accumulator as soon as every taxon's edge counts it."""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(P, dtype=np.int64)
    w = np.random.default_rng(P + n).integers(0, 6, size=P).astype(np.int64)
    w[P // 2] = 2 ** 32 // n + 1
    w[0 if P // 2 else -1] = 0 if P > 1 else w[0]
    return w


@functools.lru_cache(maxsize=None)
def schedules(n):
    """Seven trees: the caterpillar, the balanced tree, random trees on random root edges, and
    the first random tree once more."""
    rng = np.random.default_rng(n)
    out = [PR.caterpillar_schedule(n), PR.balanced_schedule(n)]
    for _ in range(4):
        edges = PR.random_edges(rng, n)
        out.append(PR.edges_schedule(edges, n, int(rng.integers(len(edges))))[:2])
    out.append(out[2])
    return out


def expected(sched, S, w):
    edges = PR.schedule_edges(*sched)
    return PR.lengths(edges, S, w, len(edges) - 1), PR.pattern_changes(edges, S), \
        PR.edge_changes(edges, S, w)


def check_lengths(n, P, K, kind, trees):
    codes, table, S = alignment(n, P, K)
    w = weights(kind, n, P)
    got = parsimony.fitch_lengths((codes, table, names_of(n)), trees, weights=w, per_pattern=True,
                                  per_edge=True)
    for t, (L, pp, pe) in zip(trees, zip(*got)):
        eL, epp, epe = expected(t, S, w)
        assert int(L) == eL, (n, P, K, kind)
        assert np.array_equal(pp, epp), (n, P, K, kind)
        assert [int(x) for x in pe] == epe, (n, P, K, kind)
    return got


@pytest.mark.parametrize("K", STATES)
@pytest.mark.parametrize("n", TAXA)
def test_fitch_lengths(n, K):
    trees = schedules(n)
    for P in PATTERNS:
        for kind in ("none", "ones", "big"):
            got = check_lengths(n, P, K, kind, trees)
            assert got[0][2] == got[0][6] and np.array_equal(got[2][2], got[2][6])
    # batches of 1 and 2, and the plain call without the optional outputs
    codes, table, S = alignment(n, 65, K)
    aln = (codes, table, names_of(n))
    w = weights("big", n, 65)
    assert 2 * n * int(w.max()) >= 2 ** 32
    for T in (1, 2):
        check_lengths(n, 65, K, "big", trees[:T])
    one = parsimony.fitch_lengths(aln, trees[0], weights=w)
    assert isinstance(one, int) and one == expected(trees[0], S, w)[0]
    many = parsimony.fitch_lengths(aln, trees, weights=w)
    assert many.dtype == np.uint64 and [int(x) for x in many] == \
        [expected(t, S, w)[0] for t in trees]


def test_trees_by_name():
    """Tree objects and Newick strings, leaves mapped to rows by name."""
    n = 9
    codes, table, S = alignment(n, 65, 4)
    names = names_of(n)
    edges = PR.random_edges(np.random.default_rng(1), n)
    tree = parsimony.edges_to_tree(edges, names)
    aln = (codes, table, names)
    want = PR.lengths(edges, S)
    assert parsimony.fitch_lengths(aln, tree) == want
    assert parsimony.fitch_lengths(aln, tree.as_newick()) == want
    got = parsimony.fitch_lengths(aln, [tree, tree.as_newick()])
    assert [int(x) for x in got] == [want, want]
    # another row order: the same tree on permuted rows
    perm = np.random.default_rng(2).permutation(n)
    assert parsimony.fitch_lengths((codes[perm], table, [names[i] for i in perm]), tree) == want


@pytest.mark.parametrize("K", [4, 20])
@pytest.mark.parametrize("n", [5, 17])
def test_insertion_lengths(n, K):
    P = 300
    codes, table, S = alignment(n, P, K)
    aln = (codes, table, names_of(n))
    rng = np.random.default_rng(n + K)
    sched = schedules(n)[3]
    edges = PR.schedule_edges(*sched)
    for Q, kind in ((1, "none"), (3, "big"), (65, "ones"), (65, "big")):
        w = weights(kind, n, P)
        q = np.ascontiguousarray(rng.integers(len(table), size=(Q, P)), dtype=np.uint8)
        got = parsimony.insertion_lengths(aln, sched, q, weights=w)
        assert got.shape == (Q, 2 * n - 3) and got.dtype == np.uint64
        assert [[int(x) for x in row] for row in got] == \
            PR.insertion_lengths(edges, S, PR.tip_sets(q, table), w)
        # the tree actually built with query qi on edge e, scored on the device
        for qi, e in {(0, 0), (Q - 1, 2 * n - 4), (Q // 2, n - 1)}:
            grown = [(u + (u >= n), v + (v >= n)) for u, v in edges]  # row n is the query
            grown = PR.attach(grown, e, n, 2 * n - 1)
            ext = (np.vstack([codes, q[qi:qi + 1]]), table, names_of(n + 1))
            built = parsimony.fitch_lengths(ext, PR.edges_schedule(grown, n + 1)[:2], weights=w)
            assert built == int(got[qi, e])


@functools.lru_cache(maxsize=None)
def stepwise_reference(n, K, weighted):
    codes, table, w, orders = PR.stepwise_case(n, K)
    S = PR.tip_sets(codes, table)
    return [PR.stepwise(S, o, w if weighted else None) for o in orders]


def check_stepwise(got, ref):
    edges, steps, lengths = got
    assert len(edges) == len(ref)
    for r, want in enumerate(ref):
        assert np.array_equal(edges[r], want["edges"]), r
        assert [int(x) for x in steps[r]] == want["step_lengths"], r
        assert int(lengths[r]) == want["length"], r


@pytest.mark.parametrize("n,K", [(n, 4) for n in PR.STEP_TAXA] + [(17, 20), (5, 2)])
def test_stepwise_addition(n, K):
    codes, table, w, orders = PR.stepwise_case(n, K)
    assert np.array_equal(orders[0], np.arange(n)) and np.array_equal(orders[1], orders[0][::-1])
    aln = (codes, table, names_of(n))
    for weighted in (True, False):
        ref = stepwise_reference(n, K, weighted)
        ww = w if weighted else None
        for R in (1, 2, 9):
            batch = parsimony.stepwise_addition(aln, orders=orders[:R], weights=ww)
            assert batch[0].shape == (R, 2 * n - 3, 2) and batch[1].shape == (R, n - 2)
            check_stepwise(batch, ref[:R])
        for r in (1, 8):  # replicate r of the batch is the same order run alone
            alone = parsimony.stepwise_addition(aln, orders=orders[r], weights=ww)
            assert all(np.array_equal(a[0], b[r]) for a, b in zip(alone, batch))


def test_stepwise_random_orders():
    n = 17
    codes, table, w, _ = PR.stepwise_case(n, 4)
    S = PR.tip_sets(codes, table)
    got = parsimony.stepwise_addition((codes, table, names_of(n)), n_rep=3, seed=11, weights=w)
    check_stepwise(got, [PR.stepwise(S, o, w) for o in parsimony.random_orders(n, 3, 11)])


def all_outputs(n, K):
    P = 600
    codes, table, _ = alignment(n, P, K)
    aln = (codes, table, names_of(n))
    w = weights("big", n, P)
    trees = schedules(n)
    q = np.ascontiguousarray(np.random.default_rng(5).integers(len(table), size=(3, P)),
                             dtype=np.uint8)
    sc, st, sw, so = PR.stepwise_case(n, K)
    return list(parsimony.fitch_lengths(aln, trees, weights=w, per_pattern=True, per_edge=True)) \
        + [parsimony.fitch_lengths(aln, trees, weights=w),
           parsimony.insertion_lengths(aln, trees[3], q, weights=w)] \
        + list(parsimony.stepwise_addition((sc, st, names_of(n)), orders=so, weights=sw)) \
        + list(parsimony.stepwise_addition(aln, orders=so[:3]))


@pytest.mark.parametrize("n,K", [(17, 4), (17, 20), (5, 2)])
def test_chunking_changes_nothing(n, K, monkeypatch):
    """PU_PARS_CHUNK (trees or replicates per chunk) and PU_PARS_WS (a lower workspace cap, which
    cuts this shape into pattern chunks too) are read at each call."""
    monkeypatch.delenv("PU_PARS_CHUNK", raising=False)
    monkeypatch.delenv("PU_PARS_WS", raising=False)
    plain = all_outputs(n, K)
    again = all_outputs(n, K)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    for chunk, ws in (("1", None), ("2", None), (None, "4096"), ("2", "20000")):
        if chunk:
            monkeypatch.setenv("PU_PARS_CHUNK", chunk)
        else:
            monkeypatch.delenv("PU_PARS_CHUNK", raising=False)
        if ws:
            monkeypatch.setenv("PU_PARS_WS", ws)
        else:
            monkeypatch.delenv("PU_PARS_WS", raising=False)
        got = all_outputs(n, K)
        assert len(got) == len(plain)
        assert all(np.array_equal(a, b) for a, b in zip(plain, got)), (chunk, ws)


def test_refusals_leave_the_device_usable():
    """Every refusal is an argument check on the host (PU_E_ARG); a valid call afterwards is
    still exact."""
    n, P, K = 5, 65, 4
    codes, table, S = alignment(n, P, K)
    names = names_of(n)
    aln = (codes, table, names)
    good = schedules(n)[2]
    ops, root = good
    orders = PR.stepwise_case(n, K)[3][:2]

    def bad_ops(i, j, v):
        o = ops.copy()
        o[i, j] = v
        return o, root

    bad_codes = codes.copy()
    bad_codes[2, 7] = len(table)
    zero_row = table.copy()
    zero_row[K + 1] = 0.0
    neg = np.ones(P, dtype=np.int64)
    neg[3] = -1
    dup = orders.copy()
    dup[1, 0] = dup[1, 1]
    out_of_range = orders.copy()
    out_of_range[0, 2] = n
    calls = [
        # n_taxa < 3
        lambda: parsimony.fitch_lengths((codes[:2], table, names[:2]),
                                        (np.zeros((0, 3), np.int32), [0, 1])),
        lambda: parsimony.stepwise_addition((codes[:2], table, names[:2]), orders=[[0, 1]]),
        # n_pat < 1
        lambda: parsimony.fitch_lengths((codes[:, :0], table, names), good),
        # a code >= n_codes
        lambda: parsimony.fitch_lengths((bad_codes, table, names), good),
        lambda: parsimony.insertion_lengths(aln, good, bad_codes[2:3]),
        # an all-zero table row
        lambda: parsimony.fitch_lengths((codes, zero_row, names), good),
        # K > 32
        lambda: parsimony.fitch_lengths((np.zeros_like(codes), np.ones((1, 33)), names), good),
        # an order that is not a permutation
        lambda: parsimony.stepwise_addition(aln, orders=dup),
        lambda: parsimony.stepwise_addition(aln, orders=out_of_range),
        # op lists that are no post-order of a binary tree over the alignment's rows
        lambda: parsimony.fitch_lengths(aln, bad_ops(0, 1, int(ops[0, 2]))),  # a child twice
        lambda: parsimony.fitch_lengths(aln, bad_ops(0, 0, 1)),               # a tip as parent
        lambda: parsimony.fitch_lengths(aln, bad_ops(0, 0, 2 * n - 2)),       # parent past range
        lambda: parsimony.fitch_lengths(aln, bad_ops(0, 1, -1)),
        lambda: parsimony.fitch_lengths(aln, (ops[::-1], root)),              # children first
        lambda: parsimony.fitch_lengths(aln, (ops, [int(root[0]), int(root[0])])),
        lambda: parsimony.fitch_lengths(aln, (ops, [int(root[0]), int(ops[0, 1])])),
        lambda: parsimony.insertion_lengths(aln, bad_ops(0, 0, 1), codes[:1]),
        # a negative weight
        lambda: parsimony.fitch_lengths(aln, good, weights=neg),
        lambda: parsimony.stepwise_addition(aln, orders=orders, weights=neg),
    ]
    want = expected(good, S, None)[0]
    for i, call in enumerate(calls):
        with pytest.raises(N.PhyloHipError) as err:
            call()
        assert "(-1)" in str(err.value), (i, str(err.value))
        assert parsimony.fitch_lengths(aln, good) == want, i


def test_profile_hook():
    n = 17
    codes, table, _ = alignment(n, 600, 4)
    parsimony.profile(True)
    try:
        parsimony.fitch_lengths((codes, table, names_of(n)), schedules(n))
        assert parsimony.kernel_ms() > 0.0
    finally:
        parsimony.profile(False)
    with pytest.raises(N.PhyloHipError):
        parsimony.kernel_ms()


# ---- TreeModel ---------------------------------------------------------------------------

NEWICK = "((a:0.1,b:0.2):0.05,((c:0.1,d:0.3):0.1,(e:0.2,f:0.1):0.2):0.1,(g:0.3,(h:0.1,i:0.2):0.1):0.2);"


@functools.lru_cache(maxsize=None)
def records():
    """Nine DNA sequences of 400 columns with signal, repeated columns, and a few percent of
    gaps and ambiguity characters."""
    rng = np.random.default_rng(3)
    n, S = 9, 400
    base = rng.integers(4, size=S)
    rows = np.where(rng.random((n, S)) < 0.3, rng.integers(4, size=(n, S)), base[None])
    rows[:4] = np.where(rng.random((4, S)) < 0.5, (base[None] + 1) % 4, rows[:4])
    chars = np.array(list("ACGT"))[rows]
    amb = rng.random((n, S)) < 0.04
    chars[amb] = rng.choice(list("-NRYK"), size=int(amb.sum()))
    return tuple((name, "".join(row)) for name, row in zip("abcdefghi", chars))


def model(subst=None):
    tm = TreeModel()
    tm.set_alignment(list(records()), A.DNA)
    tm.set_substitution_model(subst or SM.GTR())
    tm.set_rate_model(GammaRateModel(4, 0.5))
    return tm


def test_treemodel_parsimony_length():
    tm = model()
    tm.set_tree(NEWICK)
    codes, table, names = tm._coded_alignment()
    assert codes.shape[1] < 400  # compressed patterns with weights
    edges = PR.schedule_edges(*parsimony.tree_schedule(NEWICK, names)[:2])
    S = PR.tip_sets(codes, table)
    want = PR.lengths(edges, S, np.asarray(tm.siteweights))
    tm.initialise()
    lnl, dirty, site = tm.likelihood(), tm._dirty, tm.sitewise_patterns()
    got, pp = tm.parsimony_length(per_pattern=True)
    assert got == tm.parsimony_length() == want and isinstance(got, int)
    assert np.array_equal(pp, PR.pattern_changes(edges, S))
    # the uncompressed alignment with unit weights
    raw, raw_table, raw_names = A.char_codes(list(records()), A.DNA)
    assert raw.shape[1] == 400
    raw_edges = PR.schedule_edges(*parsimony.tree_schedule(NEWICK, sorted(raw_names,
                                                                          key=raw_names.get))[:2])
    assert PR.lengths(raw_edges, PR.tip_sets(raw, raw_table)) == want
    # the likelihood state is as it was
    assert tm._dirty == dirty and tm.likelihood() == lnl
    assert np.array_equal(tm.sitewise_patterns(), site)


def test_treemodel_set_parsimony_tree():
    tm = model()
    codes, table, names = tm._coded_alignment()
    n = len(names)
    w = np.asarray(tm.siteweights).astype(np.int64)
    S = PR.tip_sets(codes, table)
    runs = [PR.stepwise(S, o, w) for o in parsimony.random_orders(n, 5, 3)]
    ref_lengths = [r["length"] for r in runs]
    best = ref_lengths.index(min(ref_lengths))  # ties: the lowest replicate
    tree, length, all_lengths = tm.set_parsimony_tree(n_rep=5, seed=3)
    assert length == ref_lengths[best] and [int(x) for x in all_lengths] == ref_lengths
    edges = runs[best]["edges"]
    changes = PR.edge_changes(edges, S, w)
    want_lens = sorted(max(c / float(w.sum()), 1e-8) for c in changes)
    assert sorted(tm.traversal.brlens.values()) == want_lens
    # the same tree, edge by edge: the restatement's edge list with its own lengths
    ref_tree = parsimony.edges_to_tree(edges, names,
                                       [max(c / float(w.sum()), 1e-8) for c in changes])
    sched = parsimony.tree_schedule(ref_tree, names)
    assert np.array_equal(parsimony.tree_schedule(tree, names)[0], sched[0])
    from phylo_utils_amd.tree import Traversal, prepare_tree
    assert dict(Traversal(prepare_tree(ref_tree)).brlens) == dict(tm.traversal.brlens)
    assert tm.parsimony_length() == length
    tm.initialise()
    before = tm.likelihood()
    tm.optimise_branch_lengths()
    after = tm.likelihood()
    print("lnL %.6f -> %.6f" % (before, after))
    assert np.isfinite(before) and after > before


def test_treemodel_parsimony_tree_under_unrest():
    tm = model(SM.Unrest())
    with pytest.raises(ValueError):
        tm.set_nj_tree()
    tree, length, _ = tm.set_parsimony_tree(n_rep=2, seed=1)
    assert length == tm.parsimony_length() > 0
    tm.initialise()
    assert np.isfinite(tm.likelihood())
