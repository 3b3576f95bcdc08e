"""Likelihood-based branch support on a TreeModel's resident partials (the
reference has no support measure): aLRT (Anisimova & Gascuel 2006), aBayes (Anisimova et al.
2011) and SH-aLRT (Guindon et al. 2010) of every internal edge, from the three arrangements of
the quartet around it, each at its own optimised central length -- what ``nni.nni_scores``
computes -- and a RELL resampling of their per-pattern log-likelihoods.

* ``quartet_site_lnl(tm, nodes, lens, t)`` -- the unweighted per-pattern lnL of the three
  arrangements of four nodes (pu_quartet_site_lnl).
* ``rell_sums(site_lnl, W)`` -- sum_p W[r][p] L[v][p] for every replicate row and vector, a zero
  weight adding nothing (pu_rell_sums).
* ``branch_support(tm)`` -- one scoring pass with the four values per internal edge
  (pu_branch_support).
* ``label_tree(tree, quartets, values, fmt)`` -- the Newick with every internal edge labelled.

Arrangement numbering and the (NOD, PAR) naming of an edge are those of ``phylo_utils_amd.nni``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .nni import _check
from .tree import Traversal, prepare_tree

FIELDS = ("lrt", "alrt_chi2", "abayes", "sh_alrt")


def quartet_site_lnl(tm, nodes, lens, t=None):
    """(site [3][S], out [3][3]): the unweighted per-pattern lnL of arrangements 0..2 of the four
    `nodes` at central lengths `t` (None: all at lens[4]), -inf where a pattern has no positive
    likelihood, and ``nni.quartet_derivatives`` of the same arguments, bit for bit
    (pu_quartet_site_lnl).  Changes nothing in the model."""
    _check(tm, "quartet_site_lnl")
    tm._ensure()
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    lens = N.f64(lens)
    if nodes.shape != (4,) or lens.shape != (5,):
        raise ValueError("four nodes and five lengths (four pendant, one central)")
    tt = None if t is None else N.f64(t)
    if tt is not None and tt.shape != (3,):
        raise ValueError("one central length per arrangement")
    site = np.zeros((3, tm._ctx_shape[2]))
    out = np.zeros((3, 3))
    N.check(N.lib().pu_quartet_site_lnl(tm._ctx, N.ptr(nodes), N.ptr(lens), N.ptr(tt),
                                        N.ptr(site), N.ptr(out)), tm._ctx, "pu_quartet_site_lnl")
    return site, out


def rell_sums(site_lnl, W, device=0):
    """out [R][V] = sum_p W[r][p] site_lnl[v][p] (pu_rell_sums): `site_lnl` fp64 [V][S] (or [S]),
    `W` uint32 [R][S] (or [S]).  A pattern with W[r][p] == 0 adds nothing, whatever
    site_lnl[v][p] is.  out[r][v] depends on (W[r], site_lnl[v], S) alone."""
    L = np.atleast_2d(N.f64(site_lnl))
    W = np.atleast_2d(np.ascontiguousarray(W, dtype=np.uint32))
    if L.ndim != 2 or W.ndim != 2 or L.shape[1] != W.shape[1]:
        raise ValueError("site_lnl [V][S] and W [R][S] must share S, not %r and %r"
                         % (L.shape, W.shape))
    out = np.zeros((W.shape[0], L.shape[0]))
    N.check(N.lib().pu_rell_sums(int(device), L.shape[0], L.shape[1], N.ptr(L), W.shape[0],
                                 N.ptr(W), N.ptr(out)), None, "pu_rell_sums")
    return out


def branch_support(tm, n_replicates=1000, seed=0, epsilon=0.05, tol=1e-8, max_iter=50,
                   first_replicate=0, full=False):
    """One scoring pass with supports (pu_branch_support).  Returns (quartets, scores, support):
    the first two exactly ``nni.nni_scores``'s, `support` a dict of arrays [n] -- ``lrt`` = 2 max(d,
    0) with d = l_0 - max(l_1, l_2), ``alrt_chi2`` = erf(sqrt(lrt / 2)), ``abayes`` = 1 / sum_k
    exp(l_k - l_0) and ``sh_alrt``, the share of the RELL replicates first_replicate ..
    first_replicate + n_replicates - 1 (``bootstrap.bootstrap_weights``' rows for `seed`) whose
    centred gap stays below d - epsilon.  An edge whose standing arrangement is not the best has
    lrt = alrt_chi2 = sh_alrt = 0.  With `full` a fourth value: the RELL sums [n][R + 1][3], row 0
    of the pattern weights themselves (l_k), then one row per replicate.  The pattern weights
    must be non-negative integers.  The model is left as ``nni_scores`` leaves it."""
    _check(tm, "branch_support")
    tm._ensure()
    R = int(n_replicates)
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    cap = max(len(tm.names) - 3, 1)
    scores = np.zeros((cap, 3, 4))
    quartets = np.zeros((cap, 6), dtype=np.int32)
    sup = np.zeros((cap, 4))
    rell = np.zeros((cap, max(R, 0) + 1, 3)) if full else None
    n = ctypes.c_int()
    N.check(N.lib().pu_branch_support(tm._ctx, len(rows), N.ptr(rows), float(tol), int(max_iter),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_replicate), R,
                                      float(epsilon), N.ptr(scores), N.ptr(quartets), N.ptr(sup),
                                      N.ptr(rell), ctypes.byref(n)), tm._ctx, "pu_branch_support")
    tm._site_valid = True
    n = n.value
    support = {f: sup[:n, i].copy() for i, f in enumerate(FIELDS)}
    out = (quartets[:n].copy(), scores[:n].copy(), support)
    return out + (rell[:n].copy(),) if full else out


def support_label(sh_alrt, abayes):
    """``SH-aLRT/aBayes``: percent with one decimal, probability with three."""
    return "%.1f/%.3f" % (100.0 * float(sh_alrt), float(abayes))


def label_tree(tree, quartets, values, fmt=None):
    """A copy of the prepared `tree` (``TreeModel.tree``, whose numbering `quartets` was taken on; a
    Newick string is prepared first) whose internal edge
    (NOD, PAR) of every row of `quartets` carries ``fmt(values[i])`` as the label of NOD, the
    edge's child end; the root edge's label sits on the seed's first child, the node that keeps
    it when the tree is derooted.  `fmt` defaults to ``"%g" % v``."""
    fmt = (lambda v: "%g" % v) if fmt is None else fmt
    t = prepare_tree(tree) if isinstance(tree, str) else tree.copy()
    node = {i: n for n, i in Traversal(t).node_dict.items()}
    if len(quartets) != len(values):
        raise ValueError("%d edges, %d values" % (len(quartets), len(values)))
    for q, v in zip(quartets, values):
        n = node[int(q[0])]
        if n.is_leaf():
            raise ValueError("node %d is a leaf" % int(q[0]))
        n.label = fmt(v)
    return t
