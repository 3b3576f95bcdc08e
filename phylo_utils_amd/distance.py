"""Pairwise maximum-likelihood distances and their variances on the GPU -- the counterpart of
the reference's ``phylo_utils/likelihood.py:226-236`` ``optimise(model, partials_a, partials_b,
min_brlen=1e-5, max_brlen=10)``, which returns ``(t, -1 / lnL''(t))`` for two sequences
(``brent_optimise`` / ``scipy_optimise`` beside it; the module needs the missing ``likcalc`` and
cannot run upstream).

Here every pair of an alignment is done in one call, with no tree and no context: the alignment is
read once into per-pair code count matrices (``k_pair_counts``), and a wave per pair then runs a
safeguarded Newton iteration on ``lnL'(t) = 0`` over those counts (``k_pair_newton``); DESIGN 4.11
gives the exact rule.  Only reversible models have the real eigen-system this needs.

There is no host fallback: every function here runs the HIP kernels of ``pu_distance.hip``.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .alignment import char_codes, compress_codes
from .rate_models import UniformRateModel


def _codes(codes):
    codes = np.asarray(codes)
    if codes.ndim != 2:
        raise ValueError("codes must be [n_taxa][n_sites]")
    if codes.dtype.kind not in "iu":
        raise TypeError("codes must be an integer array")
    if codes.size and (codes.min() < 0 or codes.max() > 255):
        raise ValueError("codes out of the uint8 range")
    return np.ascontiguousarray(codes, dtype=np.uint8)


def _pairs(pairs, n_taxa):
    """(int32 [n][2] or None, n)"""
    if pairs is None:
        return None, n_taxa * (n_taxa - 1) // 2
    pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
    return pairs, len(pairs)


def all_pairs(n_taxa):
    """The default pair list: every i < j, row-major."""
    i, j = np.triu_indices(n_taxa, 1)
    return np.stack([i, j], axis=1).astype(np.int32)


def _weights(weights, n_sites):
    if weights is None:
        return None
    weights = N.f64(weights).reshape(-1)
    if len(weights) != n_sites:
        raise ValueError("weights and codes differ in length")
    return weights


def pair_counts(codes, n_codes, weights=None, pairs=None, device=0):
    """Weighted code pair count matrices (pu_pair_counts): out[p][u][v] = the sum of weights[s]
    over the sites s where pairs[p]'s first taxon shows code u and its second code v.  `pairs`
    [n][2] (any order, repeats allowed) or None: every i < j, row-major."""
    codes = _codes(codes)
    nt, S = codes.shape
    weights = _weights(weights, S)
    pairs, n = _pairs(pairs, nt)
    out = np.empty((max(n, 0), int(n_codes), int(n_codes)))
    N.check(N.lib().pu_pair_counts(int(device), N.ptr(codes), nt, S, int(n_codes), N.ptr(weights),
                                   n, N.ptr(pairs), N.ptr(out)), None, "pu_pair_counts")
    return out


def _model_args(substitution_model, rate_model):
    if not getattr(substitution_model, "reversible", True):
        raise ValueError("pairwise distances need a reversible model: %s has no real "
                         "eigen-system" % (substitution_model.name,))
    rate_model = UniformRateModel() if rate_model is None else rate_model
    ev, el, iv = substitution_model.engine_eigen()
    return (ev, el, iv, N.f64(substitution_model.freqs), N.f64(rate_model.rates),
            N.f64(rate_model.weights))


def evaluate_codes(codes, table, substitution_model, rate_model=None, weights=None, pairs=None,
                   t0=None, lo=1e-5, hi=10.0, tol=1e-10, max_iter=50, device=0):
    """pu_pair_distances on coded rows: out5 [n_pairs][5] = (t, lnL, lnL', lnL'', evaluations)."""
    codes = _codes(codes)
    table = N.f64(table)
    nt, S = codes.shape
    weights = _weights(weights, S)
    pairs, n = _pairs(pairs, nt)
    m = _model_args(substitution_model, rate_model)
    if table.ndim != 2 or table.shape[1] != len(m[3]):
        raise ValueError("code table %r does not match the model's %d states"
                         % (table.shape, len(m[3])))
    if t0 is not None:
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
    out = np.empty((max(n, 0), 5))
    N.check(N.lib().pu_pair_distances(
        int(device), table.shape[1], len(m[4]), len(table), N.ptr(table), N.ptr(m[0]),
        N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]), N.ptr(codes), nt, S,
        N.ptr(weights), n, N.ptr(pairs), N.ptr(t0), float(lo), float(hi), float(tol),
        int(max_iter), N.ptr(out)), None, "pu_pair_distances")
    return out


def distances_device(stream, d_codes, ld, n_taxa, n_sites, table, substitution_model,
                     rate_model=None, d_weights=None, pairs=None, t0=None, lo=1e-5, hi=10.0,
                     tol=1e-10, max_iter=50, d_out5=None, device=0):
    """pu_pair_distances_device: `d_codes`, `d_weights` and `d_out5` are device addresses
    (integers), `stream` a hipStream_t handle; asynchronous on that stream."""
    table = N.f64(table)
    pairs, n = _pairs(pairs, n_taxa)
    m = _model_args(substitution_model, rate_model)
    if t0 is not None:
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
    import ctypes
    vp = lambda x: None if x is None else ctypes.c_void_p(int(x))
    N.check(N.lib().pu_pair_distances_device(
        int(device), vp(stream), table.shape[1], len(m[4]), len(table), N.ptr(table),
        N.ptr(m[0]), N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]),
        vp(d_codes), int(ld), int(n_taxa), int(n_sites), vp(d_weights), n, N.ptr(pairs),
        N.ptr(t0), float(lo), float(hi), float(tol), int(max_iter), vp(d_out5)), None,
        "pu_pair_distances_device")
    return n


def _coded(alignment_or_codes, alphabet, table):
    """(codes, table, names) of an alignment ([(name, seq)], dict, records) or of a
    (codes, table[, names]) tuple."""
    if isinstance(alignment_or_codes, tuple) and len(alignment_or_codes) in (2, 3) \
            and isinstance(alignment_or_codes[0], np.ndarray):
        codes, table = alignment_or_codes[0], alignment_or_codes[1]
        names = (list(alignment_or_codes[2]) if len(alignment_or_codes) == 3
                 else ["t%d" % i for i in range(len(codes))])
        return _codes(codes), N.f64(table), names
    if isinstance(alignment_or_codes, np.ndarray):
        if table is None:
            raise ValueError("a code array needs its code table (table=...)")
        return (_codes(alignment_or_codes), N.f64(table),
                ["t%d" % i for i in range(len(alignment_or_codes))])
    if alphabet is None:
        raise ValueError("an alignment of sequences needs its alphabet")
    codes, table, names = char_codes(alignment_or_codes, alphabet)
    return codes, table, sorted(names, key=names.get)


def matrices(out5, pairs, n_taxa):
    """(D, V) [n][n] from out5 rows: D symmetric with a zero diagonal, V = -1 / lnL'' where
    lnL'' < 0, else +inf, with a zero diagonal."""
    pairs = all_pairs(n_taxa) if pairs is None else np.asarray(pairs).reshape(-1, 2)
    D = np.zeros((n_taxa, n_taxa))
    V = np.zeros((n_taxa, n_taxa))
    d2 = out5[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(d2 < 0, -1.0 / d2, np.inf)
    D[pairs[:, 0], pairs[:, 1]] = D[pairs[:, 1], pairs[:, 0]] = out5[:, 0]
    V[pairs[:, 0], pairs[:, 1]] = V[pairs[:, 1], pairs[:, 0]] = var
    return D, V


def pairwise_distances(alignment_or_codes, substitution_model, rate_model=None, alphabet=None,
                       lo=1e-5, hi=10.0, tol=1e-10, max_iter=50, pairs=None,
                       return_details=False, device=0, table=None, weights=None, compress=True):
    """ML distances of all pairs (likelihood.py:226-236 per pair; `lo`, `hi` default to its
    min_brlen, max_brlen): returns (names, D [n][n], V [n][n]) -- D symmetric with a zero
    diagonal, V = -1 / lnL'' where lnL'' < 0, else +inf -- and with `return_details` also the
    out5 rows (t, lnL, lnL', lnL'', evaluations), one per pair (`pairs`, or every i < j
    row-major).  A pair that used 2 + max_iter evaluations did not converge.
    `alignment_or_codes`: [(name, seq)] / dict / records with `alphabet`, or a uint8 code array
    with `table`, or a (codes, table[, names]) tuple.  Site patterns are compressed first
    (``compress_codes``), so the weights are integer counts; `weights` (per site) skips that."""
    codes, table, names = _coded(alignment_or_codes, alphabet, table)
    if weights is None and compress:
        codes, weights, _ = compress_codes(codes, len(table), device)
    out5 = evaluate_codes(codes, table, substitution_model, rate_model, weights, pairs, None, lo,
                          hi, tol, max_iter, device)
    D, V = matrices(out5, pairs, len(codes))
    return (names, D, V, out5) if return_details else (names, D, V)


def evaluate_pairs(alignment_or_codes, substitution_model, t, rate_model=None, alphabet=None,
                   pairs=None, device=0, table=None, weights=None):
    """(lnL, lnL', lnL'') [n_pairs][3] of every pair at length(s) `t` (a scalar or one per pair):
    pu_pair_distances with max_iter = 0."""
    codes, table, _ = _coded(alignment_or_codes, alphabet, table)
    t = np.asarray(t, dtype=np.float64)
    lo, hi = min(1e-5, float(t.min())), max(10.0, float(t.max()))
    if lo == hi or not lo > 0:
        raise ValueError("lengths must be positive")
    out5 = evaluate_codes(codes, table, substitution_model, rate_model, weights, pairs, t, lo, hi,
                          1e-10, 0, device)
    return out5[:, 1:4].copy()


def write_phylip(names, D, fh):
    """A square PHYLIP distance matrix: the taxon count, then one row per taxon -- its name and
    its distances, %.10g."""
    D = np.asarray(D)
    if D.shape != (len(names), len(names)):
        raise ValueError("matrix %r for %d names" % (D.shape, len(names)))
    fh.write("%d\n" % len(names))
    for name, row in zip(names, D):
        fh.write("%s %s\n" % (name, " ".join("%.10g" % x for x in row)))
