"""The restatement of DESIGN 4.30 (tests/lmap_reference.py) against the oracle -- its four-taxon
likelihood against ``oracle.tree_lnl`` on the explicit tree, its derivatives against
``oracle.edge_derivs`` on the two partials of every edge -- its quartet draws against an
independent formulation on the Python Philox, the host finish of phylo_utils_amd/lmap.py, the
writers, and every refusal the C calls make before they touch a device."""
import io
import itertools
import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import concordance_reference as CR
import lmap_reference as LR
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import lmap
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import (GammaRateModel, InvariantGammaModel, InvariantSitesModel,
                                         UniformRateModel)
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES

DNA_TABLE, _ = A.code_table(A.DNA)
AA_TABLE, _ = A.code_table(A.PROTEIN)
BIN_TABLE, _ = A.code_table(A.BINARY)


def case(K, rate, seed, S=40, n_taxa=5, real_weights=False):
    """(model, rate model, table, codes with gap and ambiguity codes, weights)."""
    rng = np.random.default_rng(seed)
    if K == 2:
        sub, table = LR.TwoState(0.3), BIN_TABLE
    elif K == 4:
        sub, table = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), DNA_TABLE
    else:
        sub, table = SM.LG(), AA_TABLE
    rm = {"1": UniformRateModel(), "4": GammaRateModel(4, 0.7), "I": InvariantSitesModel(0.2),
          "I4": InvariantGammaModel(0.2, 4, 0.7)}[rate]
    base = rng.integers(0, len(table), S)
    codes = np.stack([np.where(rng.random(S) < 0.6, base, rng.integers(0, len(table), S))
                      for _ in range(n_taxa)]).astype(np.uint8)
    w = rng.random(S) + 0.25 if real_weights else rng.integers(1, 9, S).astype(np.float64)
    w[S // 3] = 0.0
    return sub, rm, table, codes, w


def rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


@pytest.mark.parametrize("K", [2, 4, 20])
@pytest.mark.parametrize("rate", ["1", "4", "I", "I4"])
def test_restatement_equals_the_oracle(oracle_mod, K, rate):
    """lnL against oracle.tree_lnl on ((p, q), (r, s)); lnL' and lnL'' in each of the five
    lengths against oracle.edge_derivs on that edge's two partials: 1e-10 on max(1, |y|), the
    bound tests/test_gpu_nni.py holds k_quartet's evaluation to."""
    sub, rm, table, codes, w = case(K, rate, 100 * K + len(rate), real_weights=(rate == "4"))
    assert (table[codes].sum(axis=2) > 1).any()  # gaps or ambiguity codes are in play
    m = LR.Model(sub, rm.rates, rm.weights)
    rng = np.random.default_rng(K)
    for tau in range(3):
        x = LR.tip_vectors(codes, table, (3, 0, 4, 1), tau)
        lens = list(rng.uniform(0.01, 0.6, 5))
        lnl = LR.evaluate(m, x, w, lens)[0]
        assert rel(lnl, LR.four_taxon_oracle(m, x, w, lens)) <= 1e-10
        for h in range(5):
            got = LR.evaluate(m, x, w, lens, h)
            want = LR.edge_derivs_oracle(m, x, w, lens, h)
            assert got[0] == lnl
            for g, r in zip(got, want):
                assert rel(g, r) <= 1e-10, (tau, h, got, want)


def test_topologies_permute_the_tips():
    sub, rm, table, codes, w = case(4, "4", 3)
    m = LR.Model(sub, rm.rates, rm.weights)
    lens = [0.1, 0.2, 0.3, 0.15, 0.05]
    a = LR.evaluate(m, LR.tip_vectors(codes, table, (0, 1, 2, 3), 1), w, lens)[0]
    b = LR.evaluate(m, LR.tip_vectors(codes, table, (0, 2, 1, 3), 0), w, lens)[0]
    c = LR.evaluate(m, LR.tip_vectors(codes, table, (0, 1, 3, 2), 2), w, lens)[0]
    assert a == b == c


def test_impossible_pattern_gives_minus_infinity():
    """+I alone at a variable pattern: L_s = 0 exactly only without the rounding of E E^-1, so
    the -inf is forced with a zero tip vector."""
    sub, rm, table, codes, w = case(4, "1", 5)
    table = np.vstack([table, np.zeros((1, 4))])
    codes[2, 7] = len(table) - 1
    m = LR.Model(sub, rm.rates, rm.weights)
    x = LR.tip_vectors(codes, table, (0, 1, 2, 3), 0)
    assert LR.evaluate(m, x, w, [0.1] * 5, 2)[0] == -np.inf
    row, der = LR.optimise(m, x, w, with_derivs=True)
    assert row[0] == -np.inf and row[6] == 0 and row[7] == 1 and np.isnan(der).all()
    w[7] = 0.0  # a weight of zero does not see it
    assert np.isfinite(LR.evaluate(m, x, w, [0.1] * 5, 2)[0])


def test_optimiser_schedule(oracle_mod):
    sub, rm, table, codes, w = case(4, "4", 8, S=200)
    m = LR.Model(sub, rm.rates, rm.weights)
    x = LR.tip_vectors(codes, table, (0, 1, 2, 3), 0)
    start = LR.evaluate(m, x, w, [0.1] * 5)[0]
    row0, _ = LR.optimise(m, x, w, max_rounds=0)
    assert row0[0] == start and list(row0[1:]) == [0.1] * 5 + [0, 1]
    rows = [LR.optimise(m, x, w, max_rounds=r, min_gain=-1.0)[0] for r in (1, 2, 3)]
    assert [r[6] for r in rows] == [1, 2, 3]
    assert start < rows[0][0] <= rows[1][0] <= rows[2][0]
    assert rows[0][7] < rows[1][7] < rows[2][7]
    early, der = LR.optimise(m, x, w, max_rounds=50, min_gain=1e-6, with_derivs=True)
    assert early[6] < 50 and early[0] >= rows[2][0] - 1e-6
    for h in range(5):  # stationary, or on a bound with the sign that keeps it there
        t, d1, d2 = early[1 + h], der[h, 0], der[h, 1]
        assert (d2 < 0 and abs(d1 / d2) < 1e-3) or (t == 1e-8 and d1 <= 0) or (t == 100.0 and d1 >= 0)
    clamped, _ = LR.optimise(m, x, w, t0=[1e-12, 0.1, 0.1, 0.1, 500.0], max_rounds=0)
    assert clamped[1] == 1e-8 and clamped[5] == 100.0


# ---- quartets -----------------------------------------------------------------------------------

def philox_u3(seed, g, c2):
    """u of counter (g, c2, word 3 = 3) on the Philox tests/concordance_reference.py uses."""
    x = CR.SR.philox4x32_10((np.uint64(g & 0xFFFFFFFF), np.uint64(g >> 32), np.uint64(c2),
                             np.uint64(3)), (seed & 0xFFFFFFFF, seed >> 32))
    return float((int(x[1][0]) >> 5 << 26 | int(x[0][0]) >> 6) * 2.0 ** -53)


def test_all_quartets_in_lexicographic_order():
    q = LR.draw_quartets(7, 35, 9)
    assert len(q) == 35 and [tuple(r) for r in q] == list(itertools.combinations(range(7), 4))
    assert np.array_equal(q, LR.draw_quartets(7, 1000, 1))  # nothing is drawn
    assert len(LR.draw_quartets(7, 34, 9)) == 34


def test_drawn_quartets():
    """Against drawing without replacement from the list of the taxa left, on the Python
    Philox; four distinct taxa in draw order; quartet g does not depend on Q."""
    n, Q, seed = 23, 60, 0x1234567890ABCDEF
    q = LR.draw_quartets(n, Q, seed)
    assert q.shape == (Q, 4)
    for g in range(Q):
        left = list(range(n))
        want = [left.pop(min(int(math.floor(philox_u3(seed, g, k) * (n - k))), n - k - 1))
                for k in range(4)]
        assert list(q[g]) == want and len(set(want)) == 4
    assert any(list(r) != sorted(r) for r in q)  # the draw order, not sorted
    assert np.array_equal(LR.draw_quartets(n, 3 * Q, seed)[:Q], q)
    assert not np.array_equal(LR.draw_quartets(n, Q, seed + 1), q)


def test_cluster_quartets():
    cluster = np.array([0, 1, -1, 2, 3, 0, 3, 2, 1, 0, -1, 3])
    members = [list(np.flatnonzero(cluster == k)) for k in range(4)]
    allq = LR.draw_quartets(12, 3 * 2 * 2 * 3, 5, cluster)
    assert [tuple(r) for r in allq] == list(itertools.product(*members))
    assert tuple(allq[1]) == (0, 1, 3, 6)  # d runs fastest
    seed, Q = 77, 20
    q = LR.draw_quartets(12, Q, seed, cluster)
    for g in range(Q):
        want = [members[k][min(int(math.floor(philox_u3(seed, g, 4 + k) * len(members[k]))),
                               len(members[k]) - 1)] for k in range(4)]
        assert list(q[g]) == want
    assert np.array_equal(LR.draw_quartets(12, 35, seed, cluster)[:Q], q)


# ---- finish -------------------------------------------------------------------------------------

def test_weights_and_regions_at_attractors_and_ties():
    for k, a in enumerate(LR.ATTRACTORS):
        assert lmap.regions([a])[0][0] == k == LR.region7(a)
    # ties: the first index wins
    assert lmap.regions([[.75, .25, 0]])[0][0] == 0       # corner 0 / edge 3
    assert lmap.regions([[.25, .75, 0]])[0][0] == 1       # corner 1 / edge 3
    assert list(lmap.regions([[.5, .5, 0], [1 / 3., 1 / 3., 1 / 3.], [.4, .4, .2]])[1]) == [0, 0, 0]
    assert lmap.regions([[0.2, 0.4, 0.4]])[1][0] == 1
    lnl = np.array([[-100.0, -100.0, -100.0], [-50.0, -60.0, -70.0], [-10.0, -np.inf, -12.0],
                    [-1e5, -1e5 - 1.0, -1e5 - 800.0]])
    p, ok = lmap.posterior_weights(lnl)
    assert list(ok) == [True, True, False, True] and np.isnan(p[2]).all()
    np.testing.assert_allclose(p[0], [1 / 3.] * 3, rtol=1e-15)
    for q in (1, 3):
        np.testing.assert_allclose(p[q], LR.weights(list(lnl[q])), rtol=1e-15)
        assert abs(p[q].sum() - 1) < 1e-15
    assert p[3, 2] == 0.0  # e^-800 underflows: no NaN
    seven, three = lmap.regions(p)
    assert list(seven) == [6, 0, -1, 3] and list(three) == [0, 0, -1, 0]
    s = lmap.summarise(seven, three)
    assert (s["n_quartets"], s["counted"], s["left_out"]) == (4, 3, 1)
    assert list(s["counts7"]) == [1, 0, 0, 1, 0, 0, 1] and list(s["counts3"]) == [3, 0, 0]
    assert (s["resolved"], s["partly"], s["unresolved"]) == (1, 1, 1)
    np.testing.assert_allclose(s["pct7"][[0, 3, 6]], [100 / 3.] * 3)
    empty = lmap.summarise([-1], [-1])
    assert empty["counted"] == 0 and np.isnan(empty["pct7"]).all()


def test_regions_equal_a_brute_force_search_on_a_grid():
    n = 60
    pts = np.array([[i / n, j / n, (n - i - j) / n] for i in range(n + 1) for j in range(n + 1 - i)])
    seven, three = lmap.regions(pts)
    for p, s, t in zip(pts, seven, three):
        assert s == LR.region7(p) and t == LR.region3(p)
    assert set(seven) == set(range(7)) and set(three) == set(range(3))


def fake_result():
    rng = np.random.default_rng(1)
    Q = 12
    out = np.zeros((Q, 3, 8))
    out[:, :, 0] = -1000.0 - rng.random((Q, 3)) * np.array([0.1, 3.0, 10.0])
    out[5, 1, 0] = -np.inf
    quartets = LR.draw_quartets(9, Q, 3)
    return lmap.LikelihoodMap(quartets, out, ["n%d" % i for i in range(9)])


def test_result_coordinates():
    r = fake_result()
    ok = r.ok
    assert ok.sum() == 11 and r.region7[5] == -1
    np.testing.assert_allclose(r.x[ok], r.weights[ok, 1] + r.weights[ok, 2] / 2)
    np.testing.assert_allclose(r.y[ok], math.sqrt(3) / 2 * r.weights[ok, 2])


def test_table_round_trips_and_svg_parses():
    r = fake_result()
    buf = io.StringIO()
    lmap.write_table(r, buf)
    buf.seek(0)
    taxa, lnl, w, r7, r3 = lmap.read_table(buf)
    assert taxa == [[r.names[t] for t in row] for row in r.quartets]
    assert np.array_equal(lnl, r.lnl)  # repr round-trips a double, -inf too
    assert np.array_equal(w, r.weights, equal_nan=True)
    assert np.array_equal(r7, r.region7) and np.array_equal(r3, r.region3)
    buf = io.StringIO()
    lmap.write_svg(r, buf)
    root = ET.fromstring(buf.getvalue())
    ns = "{http://www.w3.org/2000/svg}"
    assert root.tag == ns + "svg"
    assert len(root.findall(".//%scircle[@class='quartet']" % ns)) == int(r.ok.sum())
    assert len(root.findall(".//%sg[@class='triangle']" % ns)) == 2
    lines = lmap.report_lines(r)
    assert lines[0] == "lmap: quartets = 12 (left out: 1)" and len(lines) == 9
    assert lines[1].startswith("lmap: region 1 = ") and lines[8].startswith("lmap: resolved ")


def test_draw_quartets_sizes_its_buffer_to_what_comes_back(monkeypatch):
    """A huge n_quartets on few taxa must not allocate n_quartets rows."""
    seen = {}

    class Lib(object):
        def pu_lmap_quartets(self, device, n, cl, Q, seed, out, n_out):
            seen["Q"] = Q
            return 0

    made = []
    zeros = np.zeros
    monkeypatch.setattr(lmap.N, "lib", lambda: Lib())
    monkeypatch.setattr(lmap.np, "zeros", lambda shape, **kw: made.append(shape) or zeros(shape, **kw))
    lmap.draw_quartets(10, 10 ** 12)
    lmap.draw_quartets(6, 10 ** 12, clusters=[0, 1, 2, 3, 3, -1])
    lmap.draw_quartets(100, 50)
    assert made == [(210, 4), (2, 4), (50, 4)] and seen["Q"] == 50


def test_default_number_of_quartets():
    assert lmap.default_quartets(5) == 5 and lmap.default_quartets(50) == 1250
    assert lmap.default_quartets(8) == 70


# ---- refusals: through the loaded library, no device --------------------------------------------

def scores_call(device_form=False, **kw):
    sub, rm, table, codes, w = case(4, "4", 1)
    ev, el, iv = sub.engine_eigen()
    a = dict(K=4, C=4, n_codes=len(table), table=table, ev=ev, el=el, iv=iv,
             pi=N.f64(sub.freqs), rates=N.f64(rm.rates), cw=N.f64(rm.weights), codes=codes,
             n_taxa=5, S=codes.shape[1], w=w, Q=2,
             quartets=np.array([[0, 1, 2, 3], [4, 2, 1, 0]], dtype=np.int32), t0=None, tol=1e-8,
             max_iter=50, max_rounds=5, min_gain=1e-6, out=np.zeros((2, 3, 8)), ld=None)
    a.update(kw)
    L = N.lib()
    if device_form:  # refused before the addresses are looked at
        rc = L.pu_lmap_scores_device(
            0, None, a["K"], a["C"], a["n_codes"], N.ptr(a["table"]), N.ptr(a["ev"]),
            N.ptr(a["el"]), N.ptr(a["iv"]), N.ptr(a["pi"]), N.ptr(a["rates"]), N.ptr(a["cw"]),
            N.ptr(a["codes"]), a["S"] if a["ld"] is None else a["ld"], a["n_taxa"], a["S"], None,
            a["Q"], N.ptr(a["quartets"]), N.ptr(a["t0"]), a["tol"], a["max_iter"],
            a["max_rounds"], a["min_gain"], N.ptr(a["out"]), None)
    else:
        rc = L.pu_lmap_scores(
            0, a["K"], a["C"], a["n_codes"], N.ptr(a["table"]), N.ptr(a["ev"]), N.ptr(a["el"]),
            N.ptr(a["iv"]), N.ptr(a["pi"]), N.ptr(a["rates"]), N.ptr(a["cw"]), N.ptr(a["codes"]),
            a["n_taxa"], a["S"], N.ptr(a["w"]), a["Q"], N.ptr(a["quartets"]), N.ptr(a["t0"]),
            a["tol"], a["max_iter"], a["max_rounds"], a["min_gain"], N.ptr(a["out"]), None)
    return rc, N.last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_score_refusals_before_any_device(device_form):
    bad = N.PU_E_ARG

    def refused(word=None, **kw):
        rc, msg = scores_call(device_form, **kw)
        assert rc == bad, (kw.keys(), rc, msg)
        assert word is None or word in msg, msg

    # the pair calls' shape and model refusals
    refused("null", codes=None)
    refused("null", table=None)
    refused("null output", out=None)
    refused("n_sites", S=0)
    refused("n_codes", n_codes=0)
    refused("n_codes", n_codes=33)
    refused("K = 3", K=3)
    refused("n_cat", C=0)
    refused("n_cat", C=65)
    # its own
    refused("n_taxa", n_taxa=3)
    refused("n_quartets", Q=0)
    refused("null quartets", quartets=None)
    refused("quartet 1", quartets=np.array([[0, 1, 2, 3], [0, 1, 2, 5]], dtype=np.int32))
    refused("quartet 0", quartets=np.array([[0, -1, 2, 3], [0, 1, 2, 4]], dtype=np.int32))
    refused("quartet 1", quartets=np.array([[0, 1, 2, 3], [2, 1, 2, 4]], dtype=np.int32))
    refused("tol", tol=0.0)
    refused("tol", tol=float("nan"))
    refused("max_iter", max_iter=-1)
    refused("max_rounds", max_rounds=-1)
    refused("min_gain", min_gain=float("nan"))
    refused("t0[4]", t0=np.array([0.1, 0.1, 0.1, 0.1, 1e-9]))
    refused("t0[0]", t0=np.array([100.5, 0.1, 0.1, 0.1, 0.1]))
    refused("t0[2]", t0=np.array([0.1, 0.1, np.nan, 0.1, 0.1]))
    refused("fewer rate categories", K=20, C=8, n_codes=len(AA_TABLE), table=AA_TABLE,
            rates=np.ones(8), cw=np.full(8, 0.125), codes=np.zeros((5, 40), dtype=np.uint8))
    # the tables of one workgroup against the LDS of a CU
    big = np.ones((32, 20))
    refused("LDS", K=20, C=16, n_codes=32, table=big, codes=np.zeros((5, 40), dtype=np.uint8))
    if device_form:
        refused("stride", ld=39)
    else:
        high = case(4, "4", 1)[3]
        high[3, 5] = len(DNA_TABLE)
        refused("code", codes=high)
        refused("weight", w=np.array([1.0] * 39 + [-1.0]))
        refused("weight", w=np.array([np.nan] + [1.0] * 39))
        refused("weight", w=np.array([np.inf] + [1.0] * 39))


def test_non_reversible_models_are_refused():
    sub, rm, table, codes, w = case(4, "1", 2)

    class NonRev(object):
        reversible = False
        name = "nonrev"

    with pytest.raises(ValueError, match="reversible"):
        lmap.quartet_likelihoods((codes, table), [[0, 1, 2, 3]], NonRev())


def test_quartet_and_bin_refusals_before_any_device():
    bad = N.PU_E_ARG
    L = N.lib()
    out = np.zeros((10, 4), dtype=np.int32)
    import ctypes
    n = ctypes.c_int64()

    def quartets(n_taxa=6, cluster=None, Q=10, out=out, n_out=n):
        rc = L.pu_lmap_quartets(0, n_taxa, N.ptr(cluster), Q, 0, N.ptr(out),
                                ctypes.byref(n_out) if n_out is not None else None)
        return rc, N.last_error()

    assert quartets(n_taxa=3)[0] == bad and "n_taxa" in N.last_error()
    assert quartets(Q=0)[0] == bad and "n_quartets" in N.last_error()
    assert quartets(out=None)[0] == bad and quartets(n_out=None)[0] == bad
    rc, msg = quartets(cluster=np.array([0, 1, 2, 2, 0, 1], dtype=np.int32))
    assert rc == bad and "cluster 3 is empty" in msg
    rc, msg = quartets(cluster=np.array([0, 1, 2, 3, 4, 1], dtype=np.int32))
    assert rc == bad and "outside -1..3" in msg
    assert quartets(cluster=np.array([0, 1, 2, 3, -2, 1], dtype=np.int32))[0] == bad
    with pytest.raises(ValueError):
        lmap.draw_quartets(6, 10, clusters=[0, 1, 2])
    with pytest.raises(ValueError, match="two clusters"):
        lmap.draw_quartets(6, 10, clusters=[[0], [0], [1], [2]])
    with pytest.raises(ValueError, match="no taxon"):
        lmap.draw_quartets(4, 10, clusters=[["a"], ["b"], ["c"], ["x"]], names=list("abcd"))

    codes = np.random.default_rng(3).integers(0, 5, (5, 30)).astype(np.uint8)
    q = np.array([[0, 1, 2, 3]], dtype=np.int32)

    def bins(codes=codes, n_codes=5, w=None, Q=1, quartets=q, n_used=5, used=None, give_out=True):
        res = np.zeros((1, 8 ** 4), dtype=np.uint64) if give_out else None
        rc = L.pu_lmap_bins(0, N.ptr(codes), codes.shape[0] if codes is not None else 5, 30,
                            n_codes, N.ptr(w), Q, N.ptr(quartets), n_used, N.ptr(used), N.ptr(res))
        return rc, N.last_error()

    assert bins(codes=None)[0] == bad and bins(give_out=False)[0] == bad
    assert bins(Q=0)[0] == bad
    assert bins(quartets=np.array([[0, 1, 1, 3]], dtype=np.int32))[0] == bad
    rc, msg = bins(n_codes=9)
    assert rc == bad and "n_used^4" in msg
    rc, msg = bins(w=np.full(30, 1.5))
    assert rc == bad and "integer" in msg
    assert bins(w=np.array([1.0] * 29 + [-1.0]))[0] == bad
    assert bins(w=np.array([1.0] * 29 + [2.0 ** 53]))[0] == bad
    rc, msg = bins(n_used=2, used=np.array([3, 1], dtype=np.uint8))
    assert rc == bad and "ascending" in msg
    rc, msg = bins(n_used=4, used=np.array([0, 1, 2, 3], dtype=np.uint8))
    assert rc == bad and "not in `used`" in msg
    assert bins(n_codes=4)[0] == bad  # a code >= n_codes
