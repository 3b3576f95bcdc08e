"""Nonparametric bootstrap (Felsenstein 1985) of neighbour-joining and BIONJ trees on the GPU
(DESIGN 4.14).

The reference has no tree builder and so no bootstrap; this is the measure of trust that goes with
``nj.neighbour_joining``: site patterns are resampled by a counter-based rule (Philox4x32-10, the
simulator's generator on a stream of its own), the pair count matrices of *all* replicates are
taken in one pass over the alignment, every replicate x pair goes through the pair calls' Newton
kernel, the matrices through ``pu_nj`` as one batch, and each split of the reference tree gets
the share of the replicate trees that hold it.  Everything up to the distances is integer
arithmetic, so replicate ``r`` of ``bootstrap_distances`` is bitwise what
``distance.pairwise_distances(..., weights=W[r])`` gives.

There is no host fallback: every function here runs the HIP kernels of ``pu_bootstrap.hip``.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from . import distance as _dist
from . import nj as _nj
from .alignment import compress_codes


def _rep_count(n_replicates):
    n_replicates = int(n_replicates)
    if n_replicates < 1:
        raise ValueError("n_replicates must be at least 1, not %d" % n_replicates)
    return n_replicates


def bootstrap_weights(weights_or_n_sites, n_replicates, seed=0, first_replicate=0, device=0):
    """pu_boot_weights: the resampled weights uint32 [n_replicates][S] of replicates
    first_replicate .. first_replicate + n_replicates - 1.  `weights_or_n_sites`: the pattern
    weights (non-negative integers) or a site count for unit weights.  Every row sums to the sum
    of the weights and depends on (seed, its replicate number, the weights) alone."""
    R = _rep_count(n_replicates)
    if np.ndim(weights_or_n_sites) == 0:
        w, S = None, int(weights_or_n_sites)
    else:
        w = N.f64(weights_or_n_sites).reshape(-1)
        S = len(w)
    out = np.empty((R, max(S, 0)), dtype=np.uint32)
    N.check(N.lib().pu_boot_weights(int(device), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    int(first_replicate), R, S, N.ptr(w), N.ptr(out)), None,
            "pu_boot_weights")
    return out


def _W(W, n_sites):
    W = np.ascontiguousarray(W, dtype=np.uint32)
    if W.ndim != 2 or W.shape[1] != n_sites:
        raise ValueError("W must be [n_replicates][%d], not %r" % (n_sites, W.shape))
    return W


def bootstrap_pair_counts(codes, n_codes, W, pairs=None, device=0):
    """pu_boot_pair_counts: [R][n_pairs][n_codes][n_codes], replicate r's the counts
    ``distance.pair_counts(codes, n_codes, W[r], pairs)``, from one pass over `codes`."""
    codes = _dist._codes(codes)
    nt, S = codes.shape
    W = _W(W, S)
    pairs, n = _dist._pairs(pairs, nt)
    out = np.empty((len(W), max(n, 0), int(n_codes), int(n_codes)))
    N.check(N.lib().pu_boot_pair_counts(int(device), N.ptr(codes), nt, S, int(n_codes), N.ptr(W),
                                        len(W), n, N.ptr(pairs), N.ptr(out)), None,
            "pu_boot_pair_counts")
    return out


def evaluate_replicates(codes, table, W, substitution_model, rate_model=None, pairs=None, lo=1e-5,
                        hi=10.0, tol=1e-10, max_iter=50, device=0):
    """pu_boot_distances on coded rows: out5 [R][n_pairs][5], replicate r's rows bitwise those of
    ``distance.evaluate_codes(codes, table, ..., weights=W[r])``."""
    codes = _dist._codes(codes)
    table = N.f64(table)
    nt, S = codes.shape
    W = _W(W, S)
    pairs, n = _dist._pairs(pairs, nt)
    m = _dist._model_args(substitution_model, rate_model)
    if table.ndim != 2 or table.shape[1] != len(m[3]):
        raise ValueError("code table %r does not match the model's %d states"
                         % (table.shape, len(m[3])))
    out = np.empty((len(W), max(n, 0), 5))
    N.check(N.lib().pu_boot_distances(
        int(device), table.shape[1], len(m[4]), len(table), N.ptr(table), N.ptr(m[0]),
        N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]), N.ptr(codes), nt, S,
        N.ptr(W), len(W), n, N.ptr(pairs), float(lo), float(hi), float(tol), int(max_iter),
        N.ptr(out)), None, "pu_boot_distances")
    return out


def _patterns(alignment_or_codes, alphabet, table, weights, compress, device, min_taxa=2):
    """(codes, table, names, weights): the coded alignment as site patterns with integer
    weights."""
    codes, table, names = _dist._coded(alignment_or_codes, alphabet, table)
    if len(codes) < min_taxa:
        raise ValueError("%d taxa, where at least %d are needed" % (len(codes), min_taxa))
    if weights is None and compress:
        codes, weights, _ = compress_codes(codes, len(table), device)
        weights = N.f64(weights)
    elif weights is not None:
        weights = _dist._weights(weights, codes.shape[1])
    return codes, table, names, weights


def bootstrap_distances(alignment_or_codes, substitution_model, rate_model=None, alphabet=None,
                        n_replicates=100, seed=0, first_replicate=0, lo=1e-5, hi=10.0, tol=1e-10,
                        max_iter=50, return_details=False, device=0, table=None, weights=None,
                        compress=True):
    """The ML distance matrices of bootstrap replicates: (names, D [R][n][n]), and with
    `return_details` also the out5 rows [R][n_pairs][5] and the resampled weights W [R][S].
    Inputs as ``distance.pairwise_distances``; the site patterns are compressed first unless
    `weights` (per pattern, integers) are given."""
    codes, table, names, weights = _patterns(alignment_or_codes, alphabet, table, weights,
                                             compress, device)
    W = bootstrap_weights(codes.shape[1] if weights is None else weights, n_replicates, seed,
                          first_replicate, device)
    out5 = evaluate_replicates(codes, table, W, substitution_model, rate_model, None, lo, hi, tol,
                               max_iter, device)
    D = np.stack([_dist.matrices(o, None, len(codes))[0] for o in out5])
    return (names, D, out5, W) if return_details else (names, D)


def _join_arrays(x):
    """(joins [n-2][2], root [2]) of a (joins, root) pair or of an ``nj.nj_joins`` tuple (joins,
    lens, root, root_len[, q])."""
    if len(x) == 2:
        joins, root = x
    else:
        joins, root = x[0], x[2]
    return (np.ascontiguousarray(joins, dtype=np.int32),
            np.ascontiguousarray(root, dtype=np.int32))


def split_support(ref, replicates, ok=None, device=0):
    """pu_split_support on join arrays: `ref` is (joins [n-2][2], root [2]) of the reference tree
    (or the tuple ``nj.nj_joins`` returns), `replicates` the same with a leading batch axis.
    Returns (support [n-3] -- of the split of cluster n + m, the share of the ok replicates that
    hold it --, n_ok)."""
    rj, rr = _join_arrays(ref)
    joins, roots = _join_arrays(replicates)
    if rj.ndim != 2 or rj.shape[1] != 2 or rr.shape != (2,):
        raise ValueError("the reference needs joins [n-2][2] and root [2]")
    n = len(rj) + 2
    if joins.ndim != 3 or joins.shape[1:] != rj.shape or roots.shape != (len(joins), 2):
        raise ValueError("the replicates need joins [R][%d][2] and roots [R][2], not %r and %r"
                         % (n - 2, joins.shape, roots.shape))
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok) != 0, dtype=np.int32)
        if ok.shape != (len(joins),):
            raise ValueError("ok must be [R]")
    support = np.empty(max(n - 3, 0))
    n_ok = np.zeros(1, dtype=np.int32)
    N.check(N.lib().pu_split_support(int(device), n, len(joins), N.ptr(rj), N.ptr(rr),
                                     N.ptr(joins), N.ptr(roots), N.ptr(ok), N.ptr(support),
                                     N.ptr(n_ok)), None, "pu_split_support")
    return support, int(n_ok[0])


def support_label(s):
    """The node label of a support value: its percentage, rounded."""
    return "%d" % round(100 * float(s))


def label_tree(tree, names, joins, support):
    """Label the internal nodes of ``nj.joins_to_tree``'s `tree` that carry a reference split --
    cluster n + m for m = 0..n-4 -- with ``support_label(support[m])``.  Returns the tree."""
    names = [str(x) for x in names]
    n = len(names)
    joins = np.asarray(joins).reshape(-1, 2)
    leaf = {x.label: x for x in tree.leaf_nodes()}
    node = [leaf[x] for x in names]
    for a, _ in joins:
        node.append(node[int(a)].parent)
    for m in range(max(n - 3, 0)):
        node[n + m].label = support_label(support[m])
    return tree


def bootstrap_nj(alignment_or_codes, model, rate_model=None, alphabet=None, n_replicates=100,
                 seed=0, method="nj", min_length=None, return_replicates=False, device=0,
                 table=None, weights=None, compress=True, lo=1e-5, hi=10.0, tol=1e-10,
                 max_iter=50):
    """The NJ (or BIONJ) tree of the alignment's pairwise ML distances with bootstrap support
    (pu_bootstrap_nj: distances, resampling, the replicates' distances and trees and the split
    comparison on one stream, only the results coming back).  Returns (tree, support, n_ok):
    `tree` is ``nj.joins_to_tree``'s, every internal node that carries a reference split
    labelled with its support in percent; `support` [n-3] belongs to clusters n + m in join
    order; `n_ok` is the number of replicates whose distances were all finite, the only ones
    counted.  With `return_replicates` also (joins [R][n-2][2], roots [R][2]) of the replicate
    trees."""
    R = _rep_count(n_replicates)
    mth = _nj._method(method)
    codes, table, names, weights = _patterns(alignment_or_codes, alphabet, table, weights,
                                             compress, device, min_taxa=3)
    n, S = codes.shape
    m = _dist._model_args(model, rate_model)
    if table.ndim != 2 or table.shape[1] != len(m[3]):
        raise ValueError("code table %r does not match the model's %d states"
                         % (table.shape, len(m[3])))
    joins = np.empty((n - 2, 2), dtype=np.int32)
    lens = np.empty((n - 2, 2))
    root = np.empty(2, dtype=np.int32)
    root_len = np.empty(1)
    support = np.empty(n - 3)
    n_ok = np.zeros(1, dtype=np.int32)
    rep_joins = np.empty((R, n - 2, 2), dtype=np.int32) if return_replicates else None
    rep_roots = np.empty((R, 2), dtype=np.int32) if return_replicates else None
    N.check(N.lib().pu_bootstrap_nj(
        int(device), mth, table.shape[1], len(m[4]), len(table), N.ptr(table), N.ptr(m[0]),
        N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]), N.ptr(codes), n, S,
        N.ptr(weights), int(seed) & 0xFFFFFFFFFFFFFFFF, R, float(lo), float(hi), float(tol),
        int(max_iter), N.ptr(joins), N.ptr(lens), N.ptr(root), N.ptr(root_len), N.ptr(support),
        N.ptr(n_ok), N.ptr(rep_joins), N.ptr(rep_roots)), None, "pu_bootstrap_nj")
    tree = _nj.joins_to_tree(names, joins, lens, root, root_len[0], min_length)
    label_tree(tree, names, joins, support)
    if return_replicates:
        return tree, support, int(n_ok[0]), (rep_joins, rep_roots)
    return tree, support, int(n_ok[0])
