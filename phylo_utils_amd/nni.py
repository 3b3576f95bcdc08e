"""Nearest-neighbour interchange (NNI) tree search on a TreeModel's resident partials
(the reference has no tree search).

While the optimising traversal stands on an internal edge, the four subtree partials around it
are valid in device memory, so the two alternative topologies at that edge are scored by a local
computation over four CLVs (``pu_quartet_derivs`` / ``pu_nni_sweep``, the ``k_quartet`` kernel)
instead of a full traversal per candidate tree.

* ``quartet_derivatives(tm, nodes, lens, t)`` -- {lnL, dlnL/dt, d2lnL/dt2} of the three
  arrangements of four nodes.
* ``nni_scores(tm)`` -- one scoring pass: every internal edge, the central length of each
  arrangement optimised by the library's Newton rule.
* ``nni_search(tm)`` -- rounds of scoring, simultaneous non-adjacent moves and branch-length
  re-optimisation until no alternative gains more than ``min_gain``.

The host side of a move (``internal_edges``, ``apply_nni``, ``select_moves``) lives in
``phylo_utils_amd.tree``.  Arrangement numbering: 0 is the standing (x0, x1 | x2, x3), 1 is
(x0, x2 | x1, x3), 2 is (x0, x3 | x1, x2), with x0, x1 the children of the edge's child end NOD
and x2, x3 its sibling and grandparent side.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .tree import (apply_nni, apply_nni_moves, internal_edges, select_moves,  # noqa: F401
                   with_lengths)


def quartet_max_cat(n_states):
    """The largest category count the quartet kernel takes for 2, 4 or 20 states."""
    n = N.lib().pu_quartet_max_cat(int(n_states))
    if n < 0:
        raise ValueError("quartet scoring does not support %d states" % n_states)
    return n


def _check(tm, what):
    if not tm.keep_partials:
        raise ValueError("%s needs keep_partials=True (PU_LNL_ONLY reuses CLV storage)" % what)
    if tm._host_p():
        raise ValueError("%s needs a reversible model (non-reversible models run on host "
                         "transition matrices)" % what)
    if tm.ascbias:
        raise ValueError("%s with the ascertainment-bias correction is not implemented" % what)
    if tm.alignment is None or len(tm.names) < 4:
        raise ValueError("%s needs at least 4 taxa" % what)


def quartet_derivatives(tm, nodes, lens, t=None):
    """[3][3] = (lnL, dlnL/dt, d2lnL/dt2) of arrangements 0..2 of the four `nodes` (pairwise
    distinct node indices of tm.traversal) with pendant lengths lens[0..3] at central lengths
    `t` (three values; None: all at the standing central length lens[4]), on the nodes' current
    partials (pu_quartet_derivs).  Changes nothing in the model."""
    _check(tm, "quartet_derivatives")
    tm._ensure()
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    lens = N.f64(lens)
    if nodes.shape != (4,) or lens.shape != (5,):
        raise ValueError("four nodes and five lengths (four pendant, one central)")
    tt = None if t is None else N.f64(t)
    if tt is not None and tt.shape != (3,):
        raise ValueError("one central length per arrangement")
    out = np.zeros((3, 3))
    N.check(N.lib().pu_quartet_derivs(tm._ctx, N.ptr(nodes), N.ptr(lens), N.ptr(tt), N.ptr(out)),
            tm._ctx, "pu_quartet_derivs")
    return out


def nni_scores(tm, tol=1e-8, max_iter=50):
    """One scoring pass over the optimising traversal (pu_nni_sweep).  Returns (quartets int32
    [n][6] = NOD, PAR, x0, x1, x2, x3; scores [n][3][4] = per arrangement t*, lnL(t*), lnL'(t*),
    evaluations), one entry per internal edge (n = N - 3), in optimising-traversal order.  No
    length is stored; the model's partials, lnL and sitewise lnL are left as a traversal leaves
    them."""
    _check(tm, "nni_scores")
    tm._ensure()
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    cap = max(len(tm.names) - 3, 1)
    scores = np.zeros((cap, 3, 4))
    quartets = np.zeros((cap, 6), dtype=np.int32)
    n = ctypes.c_int()
    N.check(N.lib().pu_nni_sweep(tm._ctx, len(rows), N.ptr(rows), float(tol), int(max_iter),
                                 N.ptr(scores), N.ptr(quartets), ctypes.byref(n)), tm._ctx,
            "pu_nni_sweep")
    tm._site_valid = True
    return quartets[:n.value].copy(), scores[:n.value].copy()


def candidates(quartets, scores, lnl0, min_gain):
    """The round's candidates: per scored edge its better alternative k (1 on a tie), if
    gain = lnL_k(t*_k) - lnl0 > min_gain."""
    out = []
    for q, s in zip(quartets, scores):
        k = 1 if s[1][1] >= s[2][1] else 2
        gain = float(s[k][1]) - lnl0
        if gain > min_gain:
            out.append(dict(nod=int(q[0]), par=int(q[1]), which=k, gain=gain, t=float(s[k][0])))
    return out


def nni_search(tm, max_rounds=50, min_gain=1e-3, sweeps=1, tol=1e-8, method="newton"):
    """NNI hill climbing from the model's current tree.  Per round: optimise the branch lengths
    (`sweeps` passes, `method` as optimise_branch_lengths) for lnL0; score every internal edge;
    an edge whose better alternative gains more than `min_gain` over lnL0 is a candidate; the
    candidates are taken greedily by descending gain (ties: the sorted (NOD, PAR) pair), skipping
    edges that share an end node with one already taken; all taken moves are applied at their
    optimised central lengths, the tree is set (the resident tips stay) and re-optimised.  If
    that lnL is not above lnL0, the round restarts from its own tree with the top candidate alone;
    if that fails too, the round's tree is restored and the search stops.  Stops when no
    candidate is left or after `max_rounds` rounds.

    Returns (tree, lnL, history): the final Tree with its optimised lengths (also the model's
    tree), its lnL, and per round dict(before, after, moves=[(nod, par, which, gain)],
    fallback)."""
    _check(tm, "nni_search")
    tm._ensure()

    def optimise():
        return tm.optimise_branch_lengths(tol=tol, sweeps=sweeps, method=method)

    def move_to(tree, moves):
        tm.set_tree(apply_nni_moves(tree, [(m["nod"], m["par"], m["which"], m["t"])
                                           for m in moves]))
        tm.initialise()
        return optimise()

    lnl0 = optimise()
    history = []
    for _ in range(int(max_rounds)):
        start = with_lengths(tm.tree, tm.traversal.brlens)
        quartets, scores = nni_scores(tm, tol=tol)
        moves = select_moves(candidates(quartets, scores, lnl0, min_gain))
        if not moves:
            break
        lnl1 = move_to(start, moves)
        fallback = False
        if not lnl1 > lnl0 and len(moves) > 1:
            fallback, moves = True, moves[:1]
            lnl1 = move_to(start, moves)
        done = [(m["nod"], m["par"], m["which"], m["gain"]) for m in moves]
        if not lnl1 > lnl0:  # no move improves the optimised tree: back to the round's tree
            tm.set_tree(start)
            tm.initialise()
            history.append(dict(before=lnl0, after=tm.likelihood(), moves=[], fallback=fallback,
                                rejected=done))
            break
        history.append(dict(before=lnl0, after=lnl1, moves=done, fallback=fallback))
        lnl0 = lnl1
    tree = with_lengths(tm.tree, tm.traversal.brlens)
    return tree, tm.likelihood(), history
