"""The restatement of DESIGN 4.29 (tests/concordance_reference.py) against things that do not
share its code -- a hand-counted alignment, the rule's own invariances, hand-made NNI neighbours
-- the host side of phylo_utils_amd/concordance.py, and every refusal pu_scf_counts makes before
it touches a device."""
import numpy as np
import pytest

import concordance_reference as CR
import parsimony_reference as PR
from phylo_utils_amd import _native as N
from phylo_utils_amd import concordance

DNA_TABLE = np.vstack([np.eye(4), np.ones((1, 4)), [[1.0, 0.0, 1.0, 0.0]]])  # A C G T - R
CODE = {c: i for i, c in enumerate("ACGT-R")}
FOUR = np.array([[0, 4], [1, 4], [2, 5], [3, 5], [4, 5]], dtype=np.int32)  # ((0,1),(2,3))


def coded(columns):
    return np.ascontiguousarray(np.array([[CODE[c] for c in col] for col in columns],
                                         dtype=np.uint8).T)


def test_hand_counted_four_taxon_alignment():
    """AACC supports ab|cd, ACAC ac|bd, ACCA ad|bc; AAAA and AACG are decisive and support
    nothing; A-CC and ARCC are not decisive."""
    codes = coded(["AACC", "ACAC", "ACCA", "AAAA", "AACG", "A-CC", "ARCC"])
    w = np.array([1, 2, 3, 5, 7, 11, 13], dtype=np.int64)
    r = CR.site(codes, DNA_TABLE, w, FOUR, 100, 0)
    assert list(r["nq"]) == [0, 0, 0, 0, 1]
    assert list(r["taxa"][4, 0]) == [0, 1, 2, 3] and (r["taxa"][4, 1:] == -1).all()
    assert [int(v) for v in r["counts"][4, 0]] == [1, 2, 3]
    assert not r["counts"][:4].any() and not r["counts"][4, 1:].any()
    sCF, sDF1, sDF2, sN, sQ = CR.finish(r["counts"][4], r["nq"][4])
    assert sCF == 100.0 * (1 / 6) and abs(sCF - 100 / 6) < 1e-13
    assert (sDF1, sDF2, sN, sQ) == (100.0 * (2 / 6), 100.0 * (3 / 6), 6.0, 1)
    assert concordance.finish(r["counts"][4], r["nq"][4]) == (sCF, sDF1, sDF2, sN, sQ)
    # unit weights count the columns
    assert [int(v) for v in CR.site(codes, DNA_TABLE, None, FOUR, 1, 0)["counts"][4, 0]] == [1, 1, 1]


def random_case(seed, n, P, K=4):
    rng = np.random.default_rng(seed)
    edges = np.array(PR.random_edges(rng, n), dtype=np.int32)
    codes, table = PR.random_alignment(rng, n, P, K)
    return rng, edges, codes, table


def test_exhaustive_branches_list_every_quartet_once_in_mixed_radix_order():
    _, edges, _, _ = random_case(1, 9, 5)
    cl = CR.clades(edges)
    nq, taxa = CR.quartets(edges, 10 ** 6, 3)
    assert len(cl) == 9 - 3
    for e, (A, B, C, D) in cl.items():
        assert sorted(A + B + C + D) == list(range(9))  # the four clades split the tips
        want = [(a, b, c, d) for a in A for b in B for c in C for d in D]
        assert nq[e] == len(want)
        assert [tuple(row) for row in taxa[e, :nq[e]]] == want
        assert (taxa[e, nq[e]:] == -1).all()
    pend = [e for e in range(len(edges)) if e not in cl]
    assert not nq[pend].any() and (taxa[pend] == -1).all()


def test_sampled_picks_lie_in_their_clades_and_do_not_depend_on_q():
    _, edges, _, _ = random_case(2, 40, 5)
    cl = CR.clades(edges)
    Q = 30
    nq, taxa = CR.quartets(edges, Q, 7)
    more_nq, more = CR.quartets(edges, 3 * Q, 7)
    other = CR.quartets(edges, Q, 8)[1]
    sampled = 0
    for e, four in cl.items():
        m = np.prod([len(c) for c in four])
        for k in range(4):
            assert set(taxa[e, :nq[e], k]) <= set(four[k])
        if m > 3 * Q:  # both above m: the first Q quartets stay
            sampled += 1
            assert nq[e] == Q and more_nq[e] == 3 * Q
            assert np.array_equal(more[e, :Q], taxa[e])
            assert not np.array_equal(other[e], taxa[e])
        elif m <= Q:   # both exhaustive: the seed changes nothing
            assert np.array_equal(other[e], taxa[e]) and np.array_equal(more[e, :m], taxa[e, :m])
    assert sampled > 10
    # the draw is the rule's: counter word 3 = 2, c2 = 4 e + k
    e = next(e for e, four in cl.items() if np.prod([len(c) for c in four]) > Q)
    u = float(CR.philox_u(7, 5, 4 * e + 2).ravel()[0])
    size = len(cl[e][2])
    assert taxa[e, 5, 2] == cl[e][2][min(int(np.floor(u * size)), size - 1)]
    import sim_reference as SR
    assert u != float(SR.uniform(7, 5, 4 * e + 2)[0])  # the simulator's stream is another


def test_weights_are_repeated_columns_and_pattern_order_is_free():
    rng, edges, codes, table = random_case(3, 12, 40)
    w = rng.integers(0, 4, size=40).astype(np.int64)
    base = CR.site(codes, table, w, edges, 20, 1)
    assert all(base["counts"][..., i].any() for i in range(3))
    cols = np.repeat(np.arange(40), w)
    expanded = CR.site(codes[:, cols], table, None, edges, 20, 1)
    assert np.array_equal(expanded["counts"], base["counts"])
    perm = rng.permutation(40)
    shuffled = CR.site(codes[:, perm], table, w[perm], edges, 20, 1)
    assert np.array_equal(shuffled["counts"], base["counts"])
    assert np.array_equal(shuffled["taxa"], base["taxa"])


def nni(edges, e, which):
    """The NNI neighbour of `edges` at internal edge e = (x, y): clade B (x's second other edge)
    changes places with C (which = 0) or D (which = 1)."""
    edges = np.array(edges, dtype=np.int32)
    x, y = (int(v) for v in edges[e])
    gx = [g for g in range(len(edges)) if g != e and x in edges[g]]
    gy = [g for g in range(len(edges)) if g != e and y in edges[g]]
    gb, gc = gx[1], gy[which]
    edges[gb] = np.where(edges[gb] == x, y, edges[gb])
    edges[gc] = np.where(edges[gc] == y, x, edges[gc])
    return edges


def test_gene_factors_sum_to_100_and_follow_nni_neighbours():
    rng, edges, _, _ = random_case(4, 11, 3)
    trees = [edges] * 3 + [np.array(PR.random_edges(rng, 11), dtype=np.int32) for _ in range(4)]
    g = CR.gene(edges, "edges", trees)
    assert sorted(g) == sorted(CR.clades(edges))
    for e, (gCF, gDF1, gDF2, gDFP, gN) in g.items():
        assert gCF + gDF1 + gDF2 + gDFP == pytest.approx(100.0, abs=1e-12) and gN == 7
        assert gCF >= 100.0 * (3 / 7)
    for e in g:
        for which in (0, 1):
            near = CR.gene(edges, "edges", [nni(edges, e, which)] * 2)
            want = (0.0, 100.0, 0.0) if which == 0 else (0.0, 0.0, 100.0)
            assert near[e][:3] == want and near[e][3] == 0.0
            for f in near:  # every other branch is still there
                if f != e:
                    assert near[f][0] == 100.0


def test_branch_clades_of_the_library_are_the_references():
    for n, seed in ((4, 0), (9, 1), (70, 2)):
        _, edges, _, _ = random_case(seed, n, 2)
        lib, ref = concordance.branch_clades(edges), CR.clades(edges)
        assert sorted(lib) == sorted(ref)
        for e in ref:
            assert list(lib[e]) == [CR.bitset(c) for c in ref[e]]
    with pytest.raises(ValueError):
        concordance.branch_clades(np.array([[0, 4], [1, 4], [2, 4], [3, 5], [4, 5]]))


def call(n, P, n_codes, K, codes, table, w, edges, Q, counts=True, nq=True):
    E = max(2 * n - 3, 1)
    c = np.zeros((E, max(Q, 1), 3), dtype=np.uint64) if counts else None
    q = np.zeros(E, dtype=np.int32) if nq else None
    rc = N.lib().pu_scf_counts(0, n, P, n_codes, K, N.ptr(codes), N.ptr(table), N.ptr(w),
                               N.ptr(edges), Q, 0, N.ptr(c), N.ptr(q), None)
    return rc, N.last_error()


def test_refusals_before_any_device():
    _, edges, codes, table = random_case(5, 6, 9)
    n, P = codes.shape
    nc, K = table.shape
    bad = N.PU_E_ARG
    ok = (n, P, nc, K, codes, table, None, edges, 10)

    def with_(**kw):
        names = ("n", "P", "n_codes", "K", "codes", "table", "w", "edges", "Q")
        a = dict(zip(names, ok))
        a.update(kw)
        return call(*[a[k] for k in names], **{k: kw[k] for k in ("counts", "nq") if k in kw})

    # the alignment, as pu_fitch_lengths refuses it
    assert with_(codes=None)[0] == bad and with_(table=None)[0] == bad
    assert with_(P=0)[0] == bad and with_(K=0)[0] == bad and with_(K=33)[0] == bad
    assert with_(n_codes=0)[0] == bad and with_(n_codes=33)[0] == bad
    high = codes.copy()
    high[2, 3] = nc
    rc, msg = with_(codes=high)
    assert rc == bad and "code" in msg
    empty = table.copy()
    empty[1] = 0.0
    assert with_(table=empty)[0] == bad and "allows no state" in N.last_error()
    assert with_(w=np.array([1] * 8 + [-1], dtype=np.int64))[0] == bad
    assert with_(w=np.array([2 ** 62] * 9, dtype=np.int64))[0] == bad
    # its own
    assert with_(n=3)[0] == bad and "n_taxa" in N.last_error()
    assert with_(n=4001)[0] == bad
    assert with_(edges=None)[0] == bad and with_(counts=False)[0] == bad
    assert with_(nq=False)[0] == bad
    assert with_(Q=0)[0] == bad and "n_quartets" in N.last_error()
    assert with_(Q=-3)[0] == bad
    rc, msg = with_(Q=2 ** 31 - 1, counts=False)   # refused for its size: no buffer is looked at
    assert rc == bad and "workspace" in msg
    twice = edges.copy()
    twice[3] = twice[4]                               # a tip on two edges
    assert with_(edges=twice)[0] == bad and "binary tree" in N.last_error()
    out = edges.copy()
    out[0, 0] = 2 * n - 2                             # a node out of range
    assert with_(edges=out)[0] == bad
    loop = np.array([[0, 6], [1, 6], [2, 7], [3, 7], [6, 7], [8, 9], [8, 9], [4, 8], [5, 9]],
                    dtype=np.int32)                   # full degrees, two components
    assert with_(edges=loop)[0] == bad and "connected" in N.last_error()


def test_python_layer_refusals():
    _, edges, codes, table = random_case(6, 6, 9)
    names = ["t%d" % i for i in range(6)]
    with pytest.raises(ValueError):
        concordance.site_concordance((codes, table, names), edges[:-2])
    with pytest.raises(ValueError):
        concordance.site_concordance((codes, table, names), edges, weights=np.full(9, 0.5))
    with pytest.raises(ValueError):
        concordance.site_concordance((codes, table, names), np.zeros((3, 3)))
    r = concordance.ConcordanceResult(edges, names)
    assert list(r.internal) == sorted(CR.clades(edges)) and r.sCF is None and r.gCF is None
    with pytest.raises(ValueError):
        concordance.labels(r)
