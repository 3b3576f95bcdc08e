"""Pairwise ML distances on the device (pu_distance.hip) against the numpy
restatement of their specification (tests/dist_reference.py): exact pair counts, lnL / lnL' /
lnL'' at fixed lengths, the optimum against brentq and the JC69 closed form, the defined results
at the bounds, invariance to everything the specification leaves out, the device pipeline
simulate -> compress -> distances, the TreeModel facade and the CLI."""
import ctypes
import functools

import numpy as np
import pytest

import dist_reference as DR
from phylo_utils_amd import TreeModel, _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import distance, phy, simulation
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES

pytestmark = pytest.mark.gpu

DNA_TABLE, _ = A.code_table(A.DNA)
AA_TABLE, _ = A.code_table(A.PROTEIN)
BIN_TABLE, _ = A.code_table(A.BINARY)
GAP = int(np.where(DNA_TABLE.all(axis=1))[0][0])


class TwoState(object):
    """A reversible two-state model (the project has no class for one): Q normalised to one
    expected change per unit time, eigen-system through the symmetrised matrix."""
    reversible = True
    name = "TwoState"

    def __init__(self, pi0=0.3):
        pi = np.array([pi0, 1.0 - pi0])
        self.freqs = pi
        q = np.array([[-pi[1], pi[1]], [pi[0], -pi[0]]]) / (2.0 * pi[0] * pi[1])
        s = np.sqrt(pi)
        lam, u = np.linalg.eigh(s[:, None] * q / s[None, :])
        self._eig = (np.ascontiguousarray(u / s[:, None]), np.ascontiguousarray(lam),
                     np.ascontiguousarray(u.T * s[None, :]))

    def engine_eigen(self):
        return self._eig


def gtr():
    return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)


def state_codes(table):
    """code of every state's one-hot vector"""
    K = table.shape[1]
    return np.array([int(np.where((table == np.eye(K)[k]).all(1))[0][0]) for k in range(K)])


def dna_codes(rng, n_taxa, S):
    """Random DNA codes with ambiguity and gaps, an all-gap column and an all-gap taxon."""
    codes = rng.integers(0, len(DNA_TABLE), (n_taxa, S)).astype(np.uint8)
    codes[:, S // 2] = GAP
    if n_taxa > 2:
        codes[1] = GAP
    return codes


# ---------------------------------------------------------------------------- counts
# k_pair_counts gives a workgroup 19 consecutive DNA pairs (10 protein, 64 binary): 7 taxa are 21
# pairs, two more than one group; 21 taxa put 20 pairs in the first row of the triangle (one
# more than a group along a row) and groups that span several rows.  Sites: chunks of 128,
# segments of at least 256 (257: two segments, 1000: four)
@pytest.mark.parametrize("n_taxa", [2, 3, 5, 7, 21])
def test_counts_are_exact(n_taxa):
    rng = np.random.default_rng(n_taxa)
    for S in (1, 63, 64, 65, 127, 128, 129, 257, 1000):
        codes = dna_codes(rng, n_taxa, S)
        w = rng.integers(1, 50, S).astype(np.float64)
        for weights in (None, w):
            got = distance.pair_counts(codes, len(DNA_TABLE), weights)
            np.testing.assert_array_equal(got, DR.counts(codes, len(DNA_TABLE), weights),
                                          err_msg="S=%d" % S)


def test_counts_protein_binary_and_wide_tables():
    rng = np.random.default_rng(5)
    for n_codes, n_taxa, S in ((len(AA_TABLE), 6, 257), (len(BIN_TABLE), 13, 300), (32, 4, 513),
                               (1, 3, 70)):
        codes = rng.integers(0, n_codes, (n_taxa, S)).astype(np.uint8)
        w = rng.integers(1, 9, S).astype(np.float64)
        np.testing.assert_array_equal(distance.pair_counts(codes, n_codes, w),
                                      DR.counts(codes, n_codes, w))


def test_counts_explicit_pairs_and_real_weights():
    rng = np.random.default_rng(6)
    codes = dna_codes(rng, 6, 500)
    pairs = [(3, 0), (0, 3), (5, 4), (0, 1), (3, 0), (2, 5)] * 5  # (j, i) order, repeats, 30 pairs
    w = rng.integers(1, 9, 500).astype(np.float64)
    got = distance.pair_counts(codes, len(DNA_TABLE), w, pairs)
    np.testing.assert_array_equal(got, DR.counts(codes, len(DNA_TABLE), w, pairs))
    np.testing.assert_array_equal(got[0], got[1].T)
    np.testing.assert_array_equal(got[0], got[4])
    wr = rng.random(500) + 0.1  # not integers: the order of the adds shows, to rounding
    got = distance.pair_counts(codes, len(DNA_TABLE), wr, pairs)
    np.testing.assert_allclose(got, DR.counts(codes, len(DNA_TABLE), wr, pairs), rtol=1e-13,
                               atol=0)


# ---------------------------------------------------------------------------- evaluation
def eval_case(K, C, rng):
    if K == 2:
        model, table, n_taxa = TwoState(0.3), BIN_TABLE, 4
    elif K == 4:
        model, table, n_taxa = gtr(), DNA_TABLE, 4
    else:
        model, table, n_taxa = SM.LG(), AA_TABLE, 3
    rm = UniformRateModel() if C == 1 else GammaRateModel(C, 0.7)
    S = 300
    base = rng.integers(0, len(table), S)
    codes = np.stack([np.where(rng.random(S) < 0.6, base, rng.integers(0, len(table), S))
                      for _ in range(n_taxa)]).astype(np.uint8)
    return model, rm, table, codes, rng.integers(1, 20, S).astype(np.float64)


@pytest.mark.parametrize("K", [2, 4, 20])
@pytest.mark.parametrize("C", [1, 4, 5])
def test_evaluation_at_fixed_lengths(K, C):
    """max_iter = 0: lnL, lnL', lnL'' at t against the restatement, to the tolerance
    tests/test_gpu_edges.py holds pu_lnl_branch_derivs to per item (rtol 1e-11, atol 1e-12),
    the atol scaled by the total weight the sums run over."""
    model, rm, table, codes, w = eval_case(K, C, np.random.default_rng(10 * K + C))
    pm = DR.PairModel(table, model, rm.rates, rm.weights)
    Nc = DR.counts(codes, len(table), w)
    for t in (1e-5, 0.1, 3.0, 10.0):
        got = distance.evaluate_pairs((codes, table), model, t, rm, weights=w)
        ref = np.array([pm.derivs(n, t) for n in Nc])
        print("K=%d C=%d t=%g max rel err %.3g" % (K, C, t, np.max(np.abs(got - ref) /
                                                                   np.maximum(np.abs(ref), 1))))
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12 * w.sum())


def test_evaluation_per_pair_lengths_and_details():
    model, rm, table, codes, w = eval_case(4, 4, np.random.default_rng(3))
    pm = DR.PairModel(table, model, rm.rates, rm.weights)
    Nc = DR.counts(codes, len(table), w)
    t = np.array([1e-5, 0.02, 0.5, 1.0, 4.0, 10.0])
    out5 = distance.evaluate_codes(codes, table, model, rm, w, None, t, max_iter=0)
    np.testing.assert_array_equal(out5[:, 0], t)
    np.testing.assert_array_equal(out5[:, 4], 1.0)
    ref = np.array([pm.derivs(n, x) for n, x in zip(Nc, t)])
    np.testing.assert_allclose(out5[:, 1:4], ref, rtol=1e-11, atol=1e-12 * w.sum())


def test_nonpositive_f_gives_nan():
    """A custom table can make F <= 0 where a count is positive: lnL = -inf, t = NaN."""
    table = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0.0, 0, 0, 0]])
    codes = np.array([[0, 1, 2, 0], [0, 1, 1, 1]], dtype=np.uint8)
    for max_iter in (0, 20):
        out5 = distance.evaluate_codes(codes, table, gtr(), None, None, None,
                                       0.1 if max_iter == 0 else None, max_iter=max_iter)
        assert np.isnan(out5[0, 0]) and np.isneginf(out5[0, 1])
        assert np.isnan(out5[0, 2]) and np.isnan(out5[0, 3])


# ---------------------------------------------------------------------------- optimum
TRUE = (0.02, 0.3, 1.5)
SIM = {"gtr": (gtr, lambda: GammaRateModel(4, 0.5), DNA_TABLE),
       "jc": (SM.JC69, UniformRateModel, DNA_TABLE),
       "lg": (SM.LG, lambda: GammaRateModel(4, 0.8), AA_TABLE)}


@functools.lru_cache(maxsize=None)
def simulated_pair(kind, i):
    """2000 sites of the project's simulator down a two-taxon tree at true distance TRUE[i]
    (seeds 11 + i: checked on the CPU, through tests/sim_reference.py, to give the restatement an
    interior root for every model here)."""
    mk_model, mk_rm, table = SIM[kind]
    model, rm = mk_model(), mk_rm()
    T = TRUE[i]
    names, states = simulation.simulate_alignment("(a:%r,b:%r);" % (T, T), model, rm, 2000,
                                                  seed=11 + i)
    assert states.shape == (2, 2000)
    return model, rm, table, state_codes(table)[states].astype(np.uint8), states


@pytest.mark.parametrize("kind", sorted(SIM))
@pytest.mark.parametrize("i", range(3))
def test_optimum_against_brentq(kind, i):
    model, rm, table, codes, _ = simulated_pair(kind, i)
    pm = DR.PairModel(table, model, rm.rates, rm.weights)
    t_ref, l_ref, d1_ref, d2_ref, where = pm.optimum(DR.counts(codes, len(table))[0])
    assert where == "interior"
    names, D, V, out5 = distance.pairwise_distances((codes, table), model, rm, tol=1e-10,
                                                    return_details=True)
    t, lnl, d1, d2, evals = out5[0]
    print("%s true %g: t_dev %.17g t_ref %.17g diff %.3g evals %d" % (kind, TRUE[i], t, t_ref,
                                                                    t - t_ref, evals))
    assert abs(t - t_ref) <= 1e-9 * max(t_ref, 1e-3)
    assert abs(d1) <= 1e-4 * abs(d2)
    assert D[0, 1] == D[1, 0] == t and D[0, 0] == D[1, 1] == 0.0
    np.testing.assert_allclose(V[0, 1], -1.0 / d2_ref, rtol=1e-7)
    assert 3 < evals < 2 + 50
    assert abs(lnl - l_ref) <= 1e-11 * abs(l_ref)


@pytest.mark.parametrize("i", range(3))
def test_optimum_jc69_closed_form(i):
    model, rm, table, codes, states = simulated_pair("jc", i)
    t_ref, v_ref, p = DR.jc69_distance(states[0], states[1])
    names, D, V = distance.pairwise_distances((codes, table), model, rm)
    assert abs(D[0, 1] - t_ref) <= 1e-9 * max(t_ref, 1e-3)
    np.testing.assert_allclose(V[0, 1], v_ref, rtol=1e-7)


def test_defined_results_at_the_bounds():
    rng = np.random.default_rng(8)
    s2c = state_codes(DNA_TABLE)
    a = rng.integers(0, 4, 600)
    rows = np.stack([s2c[a], s2c[a], s2c[rng.integers(0, 4, 600)], s2c[rng.integers(0, 4, 600)],
                     np.full(600, GAP)]).astype(np.uint8)
    pairs = [(0, 1), (2, 3), (0, 4), (4, 2)]
    lo, hi = 1e-5, 10.0
    out5 = distance.evaluate_codes(rows, DNA_TABLE, gtr(), GammaRateModel(4, 0.5), None, pairs,
                                   None, lo, hi)
    # identical sequences: lo after one evaluation
    assert out5[0, 0] == lo and out5[0, 2] < 0 and out5[0, 4] == 1
    # two independent random sequences: hi after two
    assert out5[1, 0] == hi and out5[1, 2] >= 0 and out5[1, 4] == 2
    # an all-gap taxon: lo, zero derivatives
    for r in out5[2:]:
        assert r[0] == lo and r[2] == 0.0 and r[3] == 0.0 and np.isfinite(r[1])
    names, D, V = distance.pairwise_distances((rows, DNA_TABLE), gtr(), GammaRateModel(4, 0.5))
    assert np.isposinf(V[0, 4]) and V[4, 4] == 0.0
    # zero total weight
    z = distance.evaluate_codes(rows, DNA_TABLE, gtr(), None, np.zeros(600), [(0, 2)])
    assert z[0, 0] == lo and np.all(z[0, 1:4] == 0.0)


def test_max_iter_one_reports_its_evaluations():
    model, rm, table, codes, _ = simulated_pair("gtr", 1)
    out5 = distance.evaluate_codes(codes, table, model, rm, None, None, 1.0, max_iter=1)
    t, lnl, d1, d2, evals = out5[0]
    # lo, hi and the start: 2 + max_iter evaluations, the last evaluated point, not a root
    assert evals == 3 and t == 1.0
    assert abs(d1) > 1e-4 * abs(d2)
    pm = DR.PairModel(table, model, rm.rates, rm.weights)
    ref = pm.derivs(DR.counts(codes, len(table))[0], 1.0)
    np.testing.assert_allclose([lnl, d1, d2], ref, rtol=1e-11, atol=2e-9)
    full = distance.evaluate_codes(codes, table, model, rm, None, None, 1.0, max_iter=50)
    assert 3 < full[0, 4] < 52 and full[0, 0] < 1.0


# ---------------------------------------------------------------------------- invariances
@functools.lru_cache(maxsize=None)
def twelve():
    rng = np.random.default_rng(12)
    s2c = state_codes(DNA_TABLE)
    base = rng.integers(0, 4, 700)
    rows = [base]
    for k in range(11):
        prev = rows[-1]
        rows.append(np.where(rng.random(700) < 0.08 + 0.02 * k, rng.integers(0, 4, 700), prev))
    codes = s2c[np.stack(rows)].astype(np.uint8)
    codes[3, :40] = GAP
    return codes


def test_bitwise_repeatable_and_chunk_independent(monkeypatch):
    codes = twelve()
    model, rm = gtr(), GammaRateModel(4, 0.5)
    run = lambda: distance.pairwise_distances((codes, DNA_TABLE), model, rm, return_details=True)
    base = run()
    assert np.all(np.isfinite(base[3]))
    np.testing.assert_array_equal(run()[3], base[3])
    cnt = distance.pair_counts(codes, len(DNA_TABLE))
    for chunk in ("1", "7"):
        monkeypatch.setenv("PU_DIST_CHUNK", chunk)
        np.testing.assert_array_equal(run()[3], base[3])
        np.testing.assert_array_equal(distance.pair_counts(codes, len(DNA_TABLE)), cnt)
    monkeypatch.delenv("PU_DIST_CHUNK")
    # compressed and uncompressed input: the same integer counts
    raw = distance.pairwise_distances((codes, DNA_TABLE), model, rm, compress=False)
    np.testing.assert_allclose(raw[1], base[1], rtol=1e-12, atol=0)
    D = base[1]
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0)


def test_device_form_equals_host_form_with_a_padded_stride():
    import torch
    codes = twelve()
    nt, S = codes.shape
    ld = S + 37
    model, rm = gtr(), GammaRateModel(4, 0.5)
    w = np.random.default_rng(2).integers(1, 6, S).astype(np.float64)
    pairs = [(1, 0), (5, 11), (11, 5), (2, 7)]
    host = distance.evaluate_codes(codes, DNA_TABLE, model, rm, w, pairs)
    host_all = distance.evaluate_codes(codes, DNA_TABLE, model, rm, w)
    dev = torch.device("cuda", 0)
    padded = np.full((nt, ld), 255, dtype=np.uint8)
    padded[:, :S] = codes
    d_codes = torch.from_numpy(padded).to(dev)
    d_w = torch.from_numpy(w).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for pr, ref in ((pairs, host), (None, host_all)):
        d_out = torch.full((len(ref), 5), -1.0, dtype=torch.float64, device=dev)
        distance.distances_device(stream, d_codes.data_ptr(), ld, nt, S, DNA_TABLE, model, rm,
                                  d_w.data_ptr(), pr, d_out5=d_out.data_ptr())
        torch.cuda.synchronize(dev)
        np.testing.assert_array_equal(d_out.cpu().numpy(), ref)
    assert np.all(d_codes.cpu().numpy()[:, S:] == 255)


def test_back_to_back_calls_on_two_streams():
    """Two device calls with pair lists of different lengths on two streams and nothing between
    them: the second waits for the first before it reuses the per-device buffers.  257 sites are
    two count segments, so the slabs and the merge kernel are in play."""
    import torch
    codes = dna_codes(np.random.default_rng(257), 6, 257)
    nt, S = codes.shape
    model, rm = gtr(), GammaRateModel(4, 0.5)
    lists = ([(0, 5), (4, 2), (3, 0)], None)
    refs = [distance.evaluate_codes(codes, DNA_TABLE, model, rm, None, pr) for pr in lists]
    assert [len(r) for r in refs] == [3, 15]
    dev = torch.device("cuda", 0)
    d_codes = torch.from_numpy(codes).to(dev)
    outs = [torch.full((len(r), 5), -1.0, dtype=torch.float64, device=dev) for r in refs]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize(dev)  # the inputs are in place; from here on nothing waits
    for st, pr, d_out in zip(streams, lists, outs):
        distance.distances_device(st.cuda_stream, d_codes.data_ptr(), S, nt, S, DNA_TABLE, model,
                                  rm, None, pr, d_out5=d_out.data_ptr())
    for st in streams:
        st.synchronize()
    for d_out, ref in zip(outs, refs):
        np.testing.assert_array_equal(d_out.cpu().numpy(), ref)


# ---------------------------------------------------------------------------- pipeline
NEWICK9 = ("(((a:0.05,b:0.05):0.1,c:0.2):0.1,((d:0.15,e:0.2):0.1,f:0.25):0.1,"
           "((g:0.04,h:0.06):0.15,i:0.3):0.1);")


def test_simulate_compress_distances_on_one_stream():
    """pu_simulate_device -> pu_compress_patterns_device -> pu_pair_distances_device: the
    alignment never leaves the device."""
    import torch
    model, rm = gtr(), GammaRateModel(4, 0.5)
    tm = TreeModel(keep_partials=False)
    tm.set_tree(NEWICK9)
    names = list(tm.traversal.names)
    tm.set_alignment_codes(np.zeros((9, 1), dtype=np.uint8), np.ones((1, 4)), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.initialise()
    S = 4096
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    N.check(N.lib().pu_ctx_set_stream(tm._ctx, stream), tm._ctx)
    try:
        d_t = torch.zeros((9, S), dtype=torch.uint8, device=dev)
        N.check(N.lib().pu_simulate_device(tm._ctx, 21, 0, S, ctypes.c_void_p(d_t.data_ptr()), S,
                                           None, None, 0), tm._ctx)
        d_u = torch.zeros((9, S), dtype=torch.uint8, device=dev)
        d_c = torch.empty(S, dtype=torch.int64, device=dev)
        d_i = torch.empty(S, dtype=torch.int64, device=dev)
        U = ctypes.c_int64()
        N.check(N.lib().pu_compress_patterns_device(
            0, stream, ctypes.c_void_p(d_t.data_ptr()), 9, S, 4, ctypes.c_void_p(d_u.data_ptr()),
            S, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_void_p(d_i.data_ptr()), ctypes.byref(U)))
        U = U.value
        assert 1 < U < S
        d_w = d_c[:U].to(torch.float64)
        d_out = torch.empty((36, 5), dtype=torch.float64, device=dev)
        # simulated rows are states: code k is state k
        distance.distances_device(stream.value, d_u.data_ptr(), S, 9, U, np.eye(4), model, rm,
                                  d_w.data_ptr(), d_out5=d_out.data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        N.check(N.lib().pu_ctx_set_stream(tm._ctx, N.PU_OWN_STREAM), tm._ctx)
    out5 = d_out.cpu().numpy()
    D, V = distance.matrices(out5, None, 9)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0) and np.all(D[~np.eye(9, dtype=bool)] > 0)
    # the same distances from the host copy of the simulated rows
    host = distance.pairwise_distances((d_t.cpu().numpy(), np.eye(4)), model, rm)
    np.testing.assert_allclose(D, host[1], rtol=1e-12, atol=0)
    # rows are tip slots: the cherries (a, b) and (g, h) are each other's nearest neighbours
    slot = {n: k for k, n in enumerate(tm._slot_names)}
    Dn = D + np.diag(np.full(9, np.inf))
    for x, y in (("a", "b"), ("g", "h")):
        assert Dn[slot[x]].argmin() == slot[y] and Dn[slot[y]].argmin() == slot[x]


# ---------------------------------------------------------------------------- facade, CLI
def _alignment(seed=4):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, 300)
    seqs = []
    for k in range(5):
        s = np.where(rng.random(300) < 0.1 * (k + 1), rng.integers(0, 4, 300), base)
        seqs.append("".join("ACGT"[x] for x in s))
    seqs[2] = "N-R" + seqs[2][3:]
    return [("s%d" % k, s) for k, s in enumerate(seqs)]


def test_tree_model_facade():
    recs = _alignment()
    model, rm = SM.HKY85(2.0, [0.3, 0.2, 0.25, 0.25]), GammaRateModel(4, 0.7)
    tm = TreeModel()
    tm.set_alignment(recs, A.DNA)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    names, D, V = tm.pairwise_distances()
    n2, D2, V2 = distance.pairwise_distances(recs, model, rm, A.DNA)
    assert names == n2 == [n for n, _ in recs]
    np.testing.assert_array_equal(D, D2)
    np.testing.assert_array_equal(V, V2)
    assert tm._ctx is None  # no tree, no context


def test_cli_distances_end_to_end(tmp_path, capsys):
    recs = _alignment()
    fa = tmp_path / "aln.fasta"
    fa.write_text("".join(">%s\n%s\n" % r for r in recs))
    spec = "HKY{2.0}+F{0.3,0.2,0.25,0.25}+G4{0.7}"
    assert phy.main(["-s", str(fa), "-m", spec, "--distances"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0] == "5" and len(lines) == 6
    names, D, V = distance.pairwise_distances(recs, SM.HKY85(2.0, [0.3, 0.2, 0.25, 0.25]),
                                              GammaRateModel(4, 0.7), A.DNA)
    for k, line in enumerate(lines[1:]):
        f = line.split()
        assert f[0] == names[k]
        assert f[1:] == ["%.10g" % x for x in D[k]]
    out = tmp_path / "d.phy"
    assert phy.main(["-s", str(fa), "-m", spec, "--distances", "-o", str(out)]) == 0
    assert out.read_text().strip().split("\n") == lines
