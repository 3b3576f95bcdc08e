"""Concordance factors on the device (pu_scf.hip, phylo_utils_amd/concordance.py)
against the plain-Python restatement of the rule (tests/concordance_reference.py): counts, nq and
picks are compared exactly, the finished factors to rtol = 4 Q 2^-53 (one division and a mean over
at most Q terms)."""
import functools

import numpy as np
import pytest

import concordance_reference as CR
import parsimony_reference as PR
import treeset_cases as C
from phylo_utils_amd import _native as N
from phylo_utils_amd import concordance, treeset

pytestmark = pytest.mark.gpu

PATTERN_TILE = 2048   # k_scf_counts, rows from memory: 256 lanes x 8 patterns
LDS_BYTES, LDS_COUNTERS = 160 * 1024, 512 * 24  # a workgroup's LDS; its 512 quartets' counters


def lds_tile(n):
    """The LDS feed's tile: 256 lanes x 8, 4 or 2 patterns, the widest whose n rows fit beside the
    counters (pu_scf.hip: acc_bytes(kQbLds) + n_taxa * 256 * PPL <= kLdsCap); None: no tile fits."""
    for ppl in (8, 4, 2):
        if LDS_COUNTERS + n * 256 * ppl <= LDS_BYTES:
            return 256 * ppl
    return None


LDS_TAXA = (8, 74, 75, 100, 148, 149, 200)  # both sides of the two thresholds between the tiles
QUARTET_BLOCK = 64    # quartets of a workgroup, rows from memory (512 with the rows in LDS)
FEEDS = ("global", "lds")


def tree_edges(kind, n, seed):
    """A caterpillar or a balanced tree over n tips with its tips, internal nodes and edges
    renumbered at random."""
    rng = np.random.default_rng(seed)
    ops, root = PR.caterpillar_schedule(n) if kind == "caterpillar" else PR.balanced_schedule(n)
    edges = np.array(PR.schedule_edges(ops, root), dtype=np.int64)
    name = np.concatenate([rng.permutation(n), n + rng.permutation(n - 2)])
    edges = name[edges]
    flip = rng.random(len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    return np.ascontiguousarray(edges[rng.permutation(len(edges))], dtype=np.int32)


def alignment(n, P, K, seed):
    """(codes, table): K states, a gap code (every state) and an ambiguity code (two states, for
    K = 2 every state); columns drift from a shared base so that all three resolutions occur;
    where there is room every row holds a gap and an ambiguity code."""
    rng = np.random.default_rng(seed)
    table = np.zeros((K + 2, K))
    table[:K] = np.eye(K)
    table[K] = 1.0
    table[K + 1, [0, K - 1]] = 1.0
    states = min(K, 3) if P < 8 else K   # few columns: few states, so that the resolutions occur
    base = rng.integers(states, size=P)
    codes = np.where(rng.random((n, P)) < 0.5, rng.integers(states, size=(n, P)), base[None])
    codes = np.where(rng.random((n, P)) < 0.04, rng.integers(K, K + 2, size=(n, P)), codes)
    if P >= 16:
        for r in range(n):
            c = rng.choice(P, size=2, replace=False)
            codes[r, c[0]], codes[r, c[1]] = K, K + 1
    return np.ascontiguousarray(codes, dtype=np.uint8), table


def weights_of(kind, P, seed):
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "small":
        return rng.integers(0, 5, size=P).astype(np.int64)
    if kind == "one":
        w = np.zeros(P, dtype=np.int64)
        w[int(rng.integers(P))] = 3
        return w
    return (2 ** 40 - rng.integers(0, 1000, size=P)).astype(np.int64)  # "big"


@functools.lru_cache(maxsize=None)
def case(kind, n, P, K, wkind, Q, seed=0):
    edges = tree_edges(kind, n, 100 * n + seed)
    codes, table = alignment(n, P, K, 7 * n + P + K + seed)
    w = weights_of(wkind, P, P + seed)
    ref = CR.site(codes, table, w, edges, Q, seed)
    for v in ref.values():
        v.setflags(write=False)
    return edges, codes, table, w, ref


def run(edges, codes, table, w, Q, seed=0):
    names = ["t%d" % i for i in range(len(codes))]
    return concordance.site_concordance((codes, table, names), edges, n_quartets=Q, seed=seed,
                                        weights=w)


def check(r, ref, Q):
    # the reference itself: no resolution is vacuous
    assert all(ref["counts"][..., i].any() for i in range(3))
    assert np.array_equal(r.nq, ref["nq"])
    assert np.array_equal(r.taxa, ref["taxa"])
    assert r.counts.dtype == np.uint64 and np.array_equal(r.counts, ref["counts"])
    rtol = 4 * Q * 2.0 ** -53
    for i, e in enumerate(r.internal):
        want = CR.finish(ref["counts"][e], ref["nq"][e])
        got = (r.sCF[i], r.sDF1[i], r.sDF2[i], r.sN[i], r.sQ[i])
        assert got[4] == want[4]
        np.testing.assert_allclose(got[:4], want[:4], rtol=rtol, atol=0.0, equal_nan=True)


# the last entry seeds the case: two were chosen so that one quartet, or one pattern, still shows
# all three resolutions
SHAPES = [("caterpillar", 4, 65, 4, "small", 100, 3),   # one branch, one quartet
          ("balanced", 5, 63, 2, "none", 100, 0),
          ("balanced", 8, 64, 20, "big", 100, 0),
          ("caterpillar", 8, 1, 2, "none", 100, 7),      # one pattern, K = 2
          ("caterpillar", 65, 65, 4, "one", QUARTET_BLOCK + 1, 0),
          ("balanced", 65, PATTERN_TILE - 1, 4, "small", 1, 0),
          ("balanced", 65, PATTERN_TILE, 20, "none", 3, 0),
          ("caterpillar", 65, PATTERN_TILE + 1, 2, "big", 3, 0),
          ("balanced", 200, 65, 20, "small", 100, 0),
          ("caterpillar", 200, 64, 4, "none", 9, 0)]


@pytest.mark.parametrize("feed", FEEDS)
@pytest.mark.parametrize("kind,n,P,K,wkind,Q,seed", SHAPES)
def test_counts_picks_and_factors_equal_the_restatement(kind, n, P, K, wkind, Q, seed, feed,
                                                        monkeypatch):
    """Both feeds of k_scf_counts, the trees' two shapes, pattern counts round the wave and the
    tile, the three alphabets, the four kinds of weights, Q below, at and across the quartet
    block."""
    edges, codes, table, w, ref = case(kind, n, P, K, wkind, Q, seed)
    monkeypatch.setenv("PU_SCF_FEED", feed)
    check(run(edges, codes, table, w, Q, seed), ref, Q)


def test_the_lds_taxa_reach_every_tile_width():
    assert [lds_tile(n) for n in LDS_TAXA] == [2048, 2048, 1024, 1024, 1024, 512, 512]
    assert lds_tile(296) == 512 and lds_tile(297) is None
    assert lds_tile(65) == 2048  # the shapes above run the widest tile, and 200 the narrowest


@pytest.mark.parametrize("feed", FEEDS)
@pytest.mark.parametrize("n", LDS_TAXA)
def test_the_tiles_of_the_lds_feed(n, feed, monkeypatch):
    """The LDS feed's tile narrows with n (2048 patterns up to 74 taxa, 1024 up to 148, 512 up to
    296), so all three builds of the kernel run here: one pattern less than the tile, the tile,
    one more; and several tiles walked by one workgroup."""
    tile = lds_tile(n)
    monkeypatch.setenv("PU_SCF_FEED", feed)
    for P in (tile - 1, tile, tile + 1, 3 * tile + 5):
        edges, codes, table, w, ref = case("balanced", n, P, 4, "small", 2, seed=1)
        check(run(edges, codes, table, w, 2, seed=1), ref, 2)


def test_past_the_last_lds_tile_the_rows_come_from_memory(monkeypatch):
    n = 297
    assert lds_tile(n) is None
    monkeypatch.setenv("PU_SCF_FEED", "lds")
    edges, codes, table, w, ref = case("caterpillar", n, 513, 4, "small", 2, seed=1)
    check(run(edges, codes, table, w, 2, seed=1), ref, 2)


def test_exhaustive_and_sampled_branches_in_one_call_two_seeds():
    """n = 8 and Q = 6: the branches next to the cherries have m = 5, the middle ones 8 or 9.  Two seeds
    give the same exhaustive branches and other picks."""
    edges, codes, table, w, ref = case("caterpillar", 8, 130, 4, "small", 6, seed=0)
    ref2 = CR.site(codes, table, w, edges, 6, 5)  # the same tree and alignment, another seed
    m = {e: int(np.prod([len(c) for c in four])) for e, four in CR.clades(edges).items()}
    small = [e for e in m if m[e] <= 6]
    large = [e for e in m if m[e] > 6]
    assert small and large
    a, b = run(edges, codes, table, w, 6, seed=0), run(edges, codes, table, w, 6, seed=5)
    check(a, ref, 6)
    check(b, ref2, 6)
    assert np.array_equal(a.taxa[small], b.taxa[small])
    assert np.array_equal(a.counts[small], b.counts[small])
    assert all(not np.array_equal(a.taxa[e], b.taxa[e]) for e in large)
    assert list(a.nq[small]) == [m[e] for e in small] and (a.nq[large] == 6).all()


@pytest.mark.parametrize("feed", FEEDS)
def test_chunks_change_nothing(feed, monkeypatch):
    """One branch per chunk, and a workspace so small that the patterns are cut too."""
    edges, codes, table, w, ref = case("balanced", 65, 2 * PATTERN_TILE + 77, 4, "small", 5)
    monkeypatch.setenv("PU_SCF_FEED", feed)
    check(run(edges, codes, table, w, 5), ref, 5)
    monkeypatch.setenv("PU_SCF_CHUNK", "1")
    check(run(edges, codes, table, w, 5), ref, 5)
    monkeypatch.setenv("PU_SCF_WS", str(2 * 65 * PATTERN_TILE))  # one tile of patterns per chunk
    check(run(edges, codes, table, w, 5), ref, 5)
    monkeypatch.delenv("PU_SCF_CHUNK")
    check(run(edges, codes, table, w, 5), ref, 5)


def test_rows_of_gaps_leave_a_branch_without_a_decisive_site():
    edges, codes, table, w, _ = case("caterpillar", 8, 70, 4, "small", 100)
    codes = codes.copy()
    # the two tips of a cherry are all gaps: no quartet of the cherry's branch is decisive
    cl = CR.clades(edges)
    e = next(e for e, four in cl.items() if sorted(len(c) for c in four)[:2] == [1, 1]
             and len(four[0]) == 1 and len(four[1]) == 1)
    codes[cl[e][0][0]] = 4
    ref = CR.site(codes, table, w, edges, 100, 0)
    assert not ref["counts"][e].any() and CR.finish(ref["counts"][e], ref["nq"][e])[4] == 0
    r = run(edges, codes, table, w, 100)
    check(r, ref, 100)
    i = list(r.internal).index(e)
    assert r.sQ[i] == 0 and r.sN[i] == 0.0 and np.isnan([r.sCF[i], r.sDF1[i], r.sDF2[i]]).all()
    assert (r.sQ > 0).any()


def test_refusals_and_a_refused_tree():
    edges, codes, table, w, _ = case("balanced", 5, 63, 2, "none", 100)
    names = ["t%d" % i for i in range(5)]
    bad = edges.copy()
    bad[0] = bad[1]
    with pytest.raises(N.PhyloHipError, match="binary tree"):
        concordance.site_concordance((codes, table, names), bad)
    with pytest.raises(N.PhyloHipError, match="n_quartets"):
        concordance.site_concordance((codes, table, names), edges, n_quartets=0)
    with pytest.raises(N.PhyloHipError, match="negative"):
        concordance.site_concordance((codes, table, names), edges, weights=-np.ones(63, dtype=np.int64))
    with pytest.raises(N.PhyloHipError, match="n_taxa"):
        concordance.site_concordance((codes[:3], table, names[:3]), np.array([[0, 3], [1, 3], [2, 3]]))


def test_profile_times():
    edges, codes, table, w, _ = case("balanced", 65, PATTERN_TILE, 20, "none", 3)
    concordance.profile(True)
    try:
        run(edges, codes, table, w, 3)
        ms = concordance.kernel_ms()
    finally:
        concordance.profile(False)
    assert len(ms) == 3 and all(np.isfinite(x) and x >= 0.0 for x in ms) and ms[2] > 0.0
    with pytest.raises(N.PhyloHipError):
        concordance.kernel_ms()


def form_arg(case_, form):
    return case_["edges"] if form == "edges" else case_[form]


def form_list(case_, form):
    return list(case_["edges"]) if form == "edges" else list(zip(*case_[form]))


@pytest.mark.parametrize("n", [5, 65, 200])
def test_gene_concordance_in_the_three_forms(n):
    """Tree sets of tests/treeset_cases.py; the reference is tree 0 and, so that gDF1 and gDF2
    occur, a tree that none of the set equals."""
    T = 17
    cs = C.case(n, T)
    far = C.random_moves(np.random.default_rng(n), cs["edges"][0], 3)
    seen = np.zeros(4)
    for ref_edges in (cs["edges"][0], far):
        want = None
        for form in ("edges", "ops", "joins"):
            w = CR.gene(ref_edges, form, form_list(cs, form))
            want = w if want is None else want
            assert w == want  # the reference itself sees one tree set in three encodings
            r = concordance.gene_concordance(ref_edges, form_arg(cs, form), form=form)
            assert list(r.internal) == sorted(want) and r.sCF is None
            got = np.stack([r.gCF, r.gDF1, r.gDF2, r.gDFP], axis=1)
            assert np.array_equal(got, np.array([want[e][:4] for e in r.internal]))
            assert (r.gN == T).all()
            np.testing.assert_allclose(got.sum(axis=1), 100.0, rtol=0, atol=1e-12)
            seen += (got > 0).any(axis=0)
        # gCF is 100 x treeset.support's frequency of the same reference
        sup, _ = treeset.support(ref_edges[None], cs["edges"])
        assert np.array_equal(r.gCF, 100.0 * sup[r.internal])
    assert seen[0] > 0 and seen[3] > 0 and (n == 5 or (seen[1] > 0 or seen[2] > 0))


def test_gene_concordance_of_nni_neighbours():
    edges = tree_edges("balanced", 12, 3)
    cl = CR.clades(edges)
    e = sorted(cl)[2]
    x, y = (int(v) for v in edges[e])
    gx = [g for g in range(len(edges)) if g != e and x in edges[g]]
    gy = [g for g in range(len(edges)) if g != e and y in edges[g]]
    for which, field in ((0, "gDF1"), (1, "gDF2")):
        near = edges.copy()
        gb, gc = gx[1], gy[which]
        near[gb] = np.where(near[gb] == x, y, near[gb])
        near[gc] = np.where(near[gc] == y, x, near[gc])
        r = concordance.gene_concordance(edges, np.stack([near, near]))
        i = list(r.internal).index(e)
        assert getattr(r, field)[i] == 100.0 and r.gCF[i] == 0.0 and r.gDFP[i] == 0.0
        assert (np.delete(r.gCF, i) == 100.0).all()


def test_tree_model_concordance_factors_equal_the_module_call():
    from phylo_utils_amd import TreeModel
    from phylo_utils_amd import alignment as A
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem
    m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    tree, names, st = make_problem(12, 300, m, GammaRateModel(4, 0.7).rates, seed=2)
    seqs = ["".join("ACGT"[x] for x in row) for row in st]
    seqs[0] = "N-R" + seqs[0][3:]
    tm = TreeModel(device=0)
    tm.set_tree(tree)
    tm.set_alignment(list(zip(names, seqs)), A.DNA)
    others = [tree.as_newick(), "((t0,t3),(t1,(t2,t4)),((t5,t6),((t7,t8),(t9,(t10,t11)))));"]
    assert set(names) == set("t%d" % i for i in range(12))
    got = tm.concordance_factors(trees=others, n_quartets=7, seed=3)
    aln = tm._coded_alignment()
    want = concordance.site_concordance(aln, tm.tree, n_quartets=7, seed=3,
                                        weights=tm.siteweights, _prepared=True)
    assert np.array_equal(got.edges, want.edges) and np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.taxa, want.taxa) and want.counts.any()
    for f in ("sCF", "sDF1", "sDF2", "sN", "sQ"):
        assert np.array_equal(getattr(got, f), getattr(want, f), equal_nan=True)
    # against the restatement too, on the model's own patterns and weights
    ref = CR.site(aln[0], aln[1], np.asarray(tm.siteweights, dtype=np.int64), got.edges, 7, 3)
    assert np.array_equal(got.counts, ref["counts"]) and np.array_equal(got.taxa, ref["taxa"])
    gene = concordance.gene_concordance(tm.tree, others, names=aln[2], _prepared=True)
    for f in ("gCF", "gDF1", "gDF2", "gDFP", "gN"):
        assert np.array_equal(getattr(got, f), getattr(gene, f))
    assert (got.gCF >= 50.0).all() and (got.gCF == 100.0).any() and (got.gN == 2).all()
    # site factors alone, and labels on the model's tree
    alone = tm.concordance_factors(n_quartets=7, seed=3)
    assert alone.gCF is None and np.array_equal(alone.counts, got.counts)
    labelled = concordance.label_tree(None, got)
    labs = [x.label for x in labelled.seed_node.postorder()
            if x.children and x is not labelled.seed_node and x.label is not None]
    assert len(labs) == 12 - 3 and all(len(s.split("/")) == 2 for s in labs)
