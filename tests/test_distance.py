"""Pairwise ML distances (the reference's phylo_utils/likelihood.py:226-236) on the
CPU: the ABI is exported and bound, every refused argument is refused before a device is
touched, the numpy restatement (tests/dist_reference.py) agrees with the JC69 closed form and
with the oracle's lnl_branch_derivs, and the CLI's --distances validation and PHYLIP writer."""
import ctypes
import io

import numpy as np
import pytest

from conftest import has_gpu

import dist_reference as DR
from phylo_utils_amd import _native as N
from phylo_utils_amd import alignment as A
from phylo_utils_amd import phy
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel, UniformRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES

PAIR_SYMBOLS = ("pu_pair_counts", "pu_pair_distances", "pu_pair_distances_device")


def test_symbols_exported_and_bound():
    lib = N.lib()
    for s in PAIR_SYMBOLS:
        assert s in N.SIGNATURES, s
        assert hasattr(lib, s), s


def test_module_imports():
    import phylo_utils_amd
    from phylo_utils_amd import distance
    assert phylo_utils_amd.distance is distance
    for f in ("pair_counts", "pairwise_distances", "evaluate_pairs", "write_phylip"):
        assert callable(getattr(distance, f))
    from phylo_utils_amd import TreeModel
    assert callable(TreeModel.pairwise_distances)


# ------------------------------------------------------------------ refused arguments
def _valid(K=4, C=4, n_taxa=3, S=10):
    """Keyword arguments of a valid pu_pair_distances call (DNA, GTR + G4)."""
    model = {2: None, 4: SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), 20: SM.LG()}[K]
    table, _ = A.code_table(A.DNA if K == 4 else A.PROTEIN)
    ev, el, iv = model.engine_eigen()
    rm = GammaRateModel(C, 0.5)
    rng = np.random.default_rng(1)
    return dict(device=0, K=K, C=C, n_codes=len(table), table=N.f64(table), ev=ev, el=el, iv=iv,
                pi=N.f64(model.freqs), r=N.f64(rm.rates), q=N.f64(rm.weights),
                codes=rng.integers(0, len(table), (n_taxa, S)).astype(np.uint8), n_taxa=n_taxa,
                S=S, w=np.ones(S), n_pairs=n_taxa * (n_taxa - 1) // 2, pairs=None, t0=None,
                lo=1e-5, hi=10.0, tol=1e-10, max_iter=50, out=np.zeros((8, 5)))


def _call(a):
    return N.lib().pu_pair_distances(
        a["device"], a["K"], a["C"], a["n_codes"], N.ptr(a["table"]), N.ptr(a["ev"]),
        N.ptr(a["el"]), N.ptr(a["iv"]), N.ptr(a["pi"]), N.ptr(a["r"]), N.ptr(a["q"]),
        N.ptr(a["codes"]), a["n_taxa"], a["S"], N.ptr(a["w"]), a["n_pairs"], N.ptr(a["pairs"]),
        N.ptr(a["t0"]), a["lo"], a["hi"], a["tol"], a["max_iter"], N.ptr(a["out"]))


def _call_device(a, ld=None):
    """The _device form with made-up device addresses: refused before any is read."""
    fake = ctypes.c_void_p(0x1000)
    return N.lib().pu_pair_distances_device(
        a["device"], None, a["K"], a["C"], a["n_codes"], N.ptr(a["table"]), N.ptr(a["ev"]),
        N.ptr(a["el"]), N.ptr(a["iv"]), N.ptr(a["pi"]), N.ptr(a["r"]), N.ptr(a["q"]),
        fake if a["codes"] is not None else None, a["S"] if ld is None else ld, a["n_taxa"],
        a["S"], None, a["n_pairs"], N.ptr(a["pairs"]), N.ptr(a["t0"]), a["lo"], a["hi"],
        a["tol"], a["max_iter"], fake if a["out"] is not None else None)


def _call_counts(a):
    return N.lib().pu_pair_counts(a["device"], N.ptr(a["codes"]), a["n_taxa"], a["S"],
                                  a["n_codes"], N.ptr(a["w"]), a["n_pairs"], N.ptr(a["pairs"]),
                                  N.ptr(a["out"]))


i32 = lambda x: np.asarray(x, dtype=np.int32)
BAD = {
    "null table": dict(table=None), "null evecs": dict(ev=None), "null evals": dict(el=None),
    "null ivecs": dict(iv=None), "null freqs": dict(pi=None), "null rates": dict(r=None),
    "null cat weights": dict(q=None), "null codes": dict(codes=None), "null out": dict(out=None),
    "one taxon": dict(n_taxa=1, n_pairs=0), "no sites": dict(S=0), "negative sites": dict(S=-3),
    "no codes": dict(n_codes=0), "33 codes": dict(n_codes=33),
    "K = 3": dict(K=3), "K = 5": dict(K=5), "no category": dict(C=0),
    "too many categories": dict(C=65),
    "lo = 0": dict(lo=0.0), "lo = hi": dict(lo=1.0, hi=1.0), "lo > hi": dict(lo=2.0, hi=1.0),
    "lo nan": dict(lo=float("nan")), "tol = 0": dict(tol=0.0), "tol < 0": dict(tol=-1e-3),
    "max_iter < 0": dict(max_iter=-1),
    "pair out of range": dict(pairs=i32([[0, 3]]), n_pairs=1),
    "negative pair": dict(pairs=i32([[-1, 1]]), n_pairs=1),
    "i == j": dict(pairs=i32([[1, 1]]), n_pairs=1),
    "pair count without a list": dict(n_pairs=2),
    "no pairs": dict(pairs=i32([[0, 1]]), n_pairs=0),
    "t0 below lo": dict(t0=np.array([1e-6, 0.1, 0.1])),
    "t0 above hi": dict(t0=np.array([0.1, 0.1, 11.0])),
    "t0 nan": dict(t0=np.array([0.1, np.nan, 0.1])),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_arguments_are_refused_without_a_device(name):
    a = dict(_valid(), **BAD[name])
    assert _call(a) == N.PU_E_ARG, name
    assert "pu_pair_distances" in N.last_error()
    assert _call_device(a) == N.PU_E_ARG, name
    if not set(BAD[name]) & {"table", "ev", "el", "iv", "pi", "r", "q", "K", "C", "lo", "hi",
                             "tol", "max_iter", "t0"}:
        assert _call_counts(a) == N.PU_E_ARG, name


def test_row_stride_and_codes_are_checked():
    a = _valid()
    assert _call_device(a, ld=a["S"] - 1) == N.PU_E_ARG
    assert "row stride" in N.last_error()
    a["codes"][2, 7] = a["n_codes"]  # a code outside the table: the host forms look
    assert _call(a) == N.PU_E_ARG
    assert "taxon 2 site 7" in N.last_error()
    assert _call_counts(a) == N.PU_E_ARG


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_valid_call_fails_loudly_without_a_device():
    from phylo_utils_amd import distance
    a = _valid()
    rc = _call(a)
    assert rc != 0 and rc != N.PU_E_ARG
    assert _call_counts(a) not in (0, N.PU_E_ARG)
    with pytest.raises(N.PhyloHipError):
        distance.pair_counts(a["codes"], a["n_codes"])
    with pytest.raises(N.PhyloHipError):
        distance.pairwise_distances(a["codes"], SM.GTR(CFG2_GTR_RATES, CFG2_FREQS),
                                    GammaRateModel(4, 0.5), table=a["table"], compress=False)


def test_non_reversible_models_are_refused():
    from phylo_utils_amd import distance
    table, _ = A.code_table(A.DNA)
    codes = np.zeros((3, 5), dtype=np.uint8)
    for m in (SM.Strsym(), SM.Unrest()):
        with pytest.raises(ValueError, match="reversible"):
            distance.pairwise_distances(codes, m, table=table, compress=False)


# ------------------------------------------------------------------ the restatement itself
def _dna_codes(states):
    table, _ = A.code_table(A.DNA)
    s2c = np.array([int(np.where((table == np.eye(4)[k]).all(1))[0][0]) for k in range(4)])
    return s2c[states].astype(np.uint8), table


@pytest.mark.parametrize("p_target", [0.01, 0.2, 0.6])
def test_restatement_matches_the_jc69_closed_form(p_target):
    rng = np.random.default_rng(int(1000 * p_target))
    S = 3000
    a = rng.integers(0, 4, S)
    b = np.where(rng.random(S) < p_target, (a + rng.integers(1, 4, S)) % 4, a)
    codes, table = _dna_codes(np.stack([a, b]))
    t_ref, v_ref, p = DR.jc69_distance(a, b)
    assert 0 < p < 0.75
    pm = DR.PairModel(table, SM.JC69())
    t, lnl, d1, d2, kind = pm.optimum(DR.counts(codes, len(table))[0])
    assert kind == "interior"
    assert abs(t - t_ref) <= 1e-10 * t_ref
    assert abs(-1.0 / d2 - v_ref) <= 1e-10 * v_ref


def test_restatement_matches_the_oracle_branch_derivatives(oracle_mod):
    """lnL, lnL', lnL'' of a Gamma(4) GTR pair with ambiguity codes and gaps against
    oracle.lnl_branch_derivs summed over the sites (the category mixture of P, dP, d2P as its
    probs): lnL to 1e-12 relative, derivatives to 1e-10 of max(1, |value|), the tolerances
    tests/test_edges.py and tests/test_gpu_edges.py hold these quantities to.  Lengths from 0.05
    up: the oracle builds P(t) as a plain eigen-sum, so each entry carries an absolute error of
    about 1e-16, which a mismatch's F = O(q t) turns into a relative error of 1e-16 / (q t) per
    site -- 1e-11 at t = 1e-5, past the 1e-12 this test asks of the sum, and the oracle's error,
    not the restatement's (which takes F from F(0) through expm1)."""
    orc = oracle_mod
    m = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)
    rm = GammaRateModel(4, 0.5)
    table, _ = A.code_table(A.DNA)
    rng = np.random.default_rng(7)
    S = 400
    a = rng.integers(0, len(table), S)
    b = np.where(rng.random(S) < 0.6, a, rng.integers(0, len(table), S))
    codes = np.stack([a, b]).astype(np.uint8)
    w = rng.integers(1, 9, S).astype(np.float64)
    Nc = DR.counts(codes, len(table), w)[0]
    pm = DR.PairModel(table, m, rm.rates, rm.weights)
    ev, el, iv = m.engine_eigen()
    q = np.asarray(rm.weights)[:, None, None]
    for t in (0.05, 0.1, 3.0, 10.0):
        probs = np.stack([(q * orc.pmatrix_deriv(ev, el, iv, t, rm.rates, k)).sum(axis=0)
                          for k in range(3)])
        d = orc.lnl_branch_derivs(probs, m.freqs, table[b], table[a], 0.0, 0.0)
        ref = (w[:, None] * d).sum(axis=0)
        got = pm.derivs(Nc, t)
        assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0]), (t, got, ref)
        for k in (1, 2):
            assert abs(got[k] - ref[k]) <= 1e-10 * max(1.0, abs(ref[k])), (t, k, got, ref)


def test_restatement_bound_rules():
    table, _ = A.code_table(A.DNA)
    pm = DR.PairModel(table, SM.JC69())
    a = np.arange(400) % 4
    same, _ = _dna_codes(np.stack([a, a]))
    t, lnl, d1, d2, kind = pm.optimum(DR.counts(same, len(table))[0])
    assert kind == "lo" and t == 1e-5 and d1 < 0
    far, _ = _dna_codes(np.stack([a, (a + 1 + np.arange(400) // 4 % 3) % 4]))
    assert pm.optimum(DR.counts(far, len(table))[0])[4] == "hi"
    gap = int(np.where(table.all(axis=1))[0][0])
    gaps = np.stack([same[0], np.full(400, gap)]).astype(np.uint8)
    t, lnl, d1, d2, kind = pm.optimum(DR.counts(gaps, len(table))[0])
    assert kind == "lo" and d1 == 0.0 and d2 == 0.0


# ------------------------------------------------------------------ CLI and writer
def test_cli_distances_argument_validation(tmp_path, capsys):
    assert phy.main(["--distances"]) == 1
    assert "Alignment file not specified" in capsys.readouterr().err
    assert phy.main(["--distances", "-s", str(tmp_path / "missing.fa")]) == 1
    assert "does not exist" in capsys.readouterr().err
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    args = phy.parse_cli(["--distances", "-s", str(fa)])
    phy.validate_args(args)  # no -t needed
    assert args.distances and args.tree is None
    assert phy.main(["--distances", "-s", str(fa), "--simulate", "5"]) == 1
    assert "exclude" in capsys.readouterr().err
    # without --distances the tree is still required
    assert phy.main(["-s", str(fa)]) == 1
    assert "Tree file not specified" in capsys.readouterr().err


def test_phylip_writer():
    from phylo_utils_amd.distance import write_phylip
    D = np.array([[0.0, 0.1234567890123, 2.5], [0.1234567890123, 0.0, 1e-5], [2.5, 1e-5, 0.0]])
    fh = io.StringIO()
    write_phylip(["a", "taxon_b", "c"], D, fh)
    assert fh.getvalue() == ("3\n"
                             "a 0 0.123456789 2.5\n"
                             "taxon_b 0.123456789 0 1e-05\n"
                             "c 2.5 1e-05 0\n")
    with pytest.raises(ValueError):
        write_phylip(["a", "b"], D, io.StringIO())


def test_matrices_from_out5():
    from phylo_utils_amd.distance import matrices
    out5 = np.array([[0.1, -5.0, 0.0, -4.0, 6], [10.0, -7.0, 0.2, 0.0, 2],
                     [1e-5, -1.0, -3.0, 2.0, 1]])
    D, V = matrices(out5, None, 3)
    assert np.array_equal(D, D.T) and np.array_equal(V, V.T)
    assert np.all(np.diag(D) == 0) and np.all(np.diag(V) == 0)
    assert D[0, 1] == 0.1 and D[0, 2] == 10.0 and D[1, 2] == 1e-5
    assert V[0, 1] == 0.25 and np.isposinf(V[0, 2]) and np.isposinf(V[1, 2])
