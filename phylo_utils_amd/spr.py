"""Subtree pruning and regrafting (SPR) tree search on a TreeModel's resident partials (DESIGN
4.20; the reference has no tree search).

NNI (``phylo_utils_amd.nni``) reaches the two neighbours of each internal edge; SPR cuts a subtree
and joins it anywhere else.  While the optimising traversal stands on edge (NOD, PAR) every
node's vector points at that edge, so the rest tree of the two prune candidates (NOD, PAR) and
(PAR, NOD) needs no traversal of its own: from the merged edge outward a node is re-oriented by
one in-place update, the regraft at that edge is one launch of ``k_regraft`` over three vectors,
and the node is restored on the way back (``pu_spr_sweep``; the rows come from
``tree.spr_rows``).  A score is the lnL of the rearranged tree at unchanged lengths -- the edge
split into halves, the subtree on its old pendant length -- a lazy pre-score; the search
optimises the lengths of the best few and keeps the first that improves.

* ``regraft_edge(tm, a, b, s, t, l)`` -- one score on the nodes' current partials.
* ``spr_scores(tm, radius=None)``     -- one scoring pass: every move within `radius`.
* ``spr_search(tm, ...)``             -- rounds of scoring, trial moves and re-optimisation.

The host side of a move (``spr_candidates``, ``spr_rows``, ``apply_spr``) lives in
``phylo_utils_amd.tree``.  Not built: optimising the pendant length, the split point or the
merged length inside the scoring pass, several moves per round, multi-rank search,
non-reversible models.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .nni import _check
from .tree import apply_spr, spr_candidates, spr_rows, with_lengths  # noqa: F401


def regraft_max_cat(n_states):
    """The largest category count the regraft kernel takes for 2, 4 or 20 states."""
    n = N.lib().pu_regraft_max_cat(int(n_states))
    if n < 0:
        raise ValueError("regraft scoring does not support %d states" % n_states)
    return n


def regraft_edge(tm, a, b, s, t, l):
    """The score of the subtree vector at node `s` joined, on a branch of length `l`, at the
    midpoint of an edge of length `t` whose ends hold the vectors of nodes `a` and `b`, on the
    nodes' current partials (pu_regraft_edge).  Changes nothing in the model."""
    _check(tm, "regraft_edge")
    tm._ensure()
    out = ctypes.c_double()
    N.check(N.lib().pu_regraft_edge(tm._ctx, int(a), int(b), int(s), float(t), float(l),
                                    ctypes.byref(out)), tm._ctx, "pu_regraft_edge")
    return out.value


def sweep(tm, rows, inner_off, inner_rows, inner_len):
    """pu_spr_sweep on the caller's rows: (scores [I], NaN for the rows that score nothing; the
    lnL of the closing traversal)."""
    _check(tm, "spr_scores")
    tm._ensure()
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    inner_off = np.ascontiguousarray(inner_off, dtype=np.int64)
    inner_rows = np.ascontiguousarray(inner_rows, dtype=np.int32).reshape(-1, 6)
    inner_len = N.f64(inner_len).reshape(-1, 4)
    scores = np.zeros(max(len(inner_rows), 1))
    lnl = ctypes.c_double()
    N.check(N.lib().pu_spr_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(inner_off),
                                 N.ptr(inner_rows), N.ptr(inner_len), N.ptr(scores),
                                 ctypes.byref(lnl)), tm._ctx, "pu_spr_sweep")
    tm._site_valid = True
    return scores[:len(inner_rows)], lnl.value


def spr_scores(tm, radius=None):
    """One scoring pass over the optimising traversal (pu_spr_sweep).  Returns (moves int32
    [n][5] = (n, o, u, v, distance), scores [n]): for every prune candidate (n, o) of the
    model's tree (``tree.spr_candidates``) the lnL of the tree with the subtree regrafted at the
    midpoint of edge (u, v) of the rest tree, at unchanged lengths, for every edge of distance
    <= `radius` (None: all 2(N - k) - 3 of them, k the leaves of the subtree); distance 0 is the
    merged edge.  The model's partials, lnL and sitewise lnL are left as a traversal leaves
    them."""
    rows, off, inner, lens, moves = spr_rows(tm.traversal, radius)
    scores, _ = sweep(tm, rows, off, inner, lens)
    scored = inner[:, 3] >= 0
    return moves[scored].copy(), scores[scored].copy()


def kernel_ms(tm):
    """The HIP-event time in ms of the last k_regraft launch made while the context profiled
    (pu_spr_kernel_ms)."""
    out = ctypes.c_double()
    N.check(N.lib().pu_spr_kernel_ms(tm._ctx, ctypes.byref(out)), tm._ctx, "pu_spr_kernel_ms")
    return out.value


def rank_moves(moves, scores, keep):
    """The round's trial moves: the moves of distance >= 1 by descending score, ties by the
    sorted (n, o, u, v), then the best move of each of the first `keep` distinct pruned subtrees
    (n, o): [(n, o, u, v, distance, score)]."""
    order = sorted((i for i in range(len(moves)) if moves[i][4] >= 1),
                   key=lambda i: (-scores[i], tuple(sorted(int(z) for z in moves[i][:4]))))
    out, seen = [], set()
    for i in order:
        key = (int(moves[i][0]), int(moves[i][1]))
        if key in seen:
            continue
        seen.add(key)
        out.append(tuple(int(z) for z in moves[i]) + (float(scores[i]),))
        if len(out) >= max(int(keep), 1):
            break
    return out


def spr_search(tm, radius=None, max_rounds=50, keep=5, min_gain=1e-3, sweeps=1, tol=1e-8,
               method="newton"):
    """SPR hill climbing from the model's current tree.  Per round: optimise the branch lengths
    (`sweeps` passes, `method` as optimise_branch_lengths) for lnL0; score every move within
    `radius`; rank the moves of distance >= 1 by score (ties: the sorted (n, o, u, v)) and take
    the best move of each of the top `keep` distinct pruned subtrees; try them in that order --
    the move applied, the tree set (the resident tips stay), the lengths optimised -- and accept
    the first whose optimised lnL exceeds lnL0 + `min_gain`.  If none does, the round's tree is
    restored and the search stops; it also stops after `max_rounds` rounds.

    Returns (tree, lnL, history): the final Tree with its optimised lengths (also the model's
    tree), its lnL, and per round dict(before, after, move = (n, o, u, v, distance) or None,
    prescore, rank, tried)."""
    _check(tm, "spr_search")
    tm._ensure()

    def optimise():
        return tm.optimise_branch_lengths(tol=tol, sweeps=sweeps, method=method)

    lnl0 = optimise()
    history = []
    for _ in range(int(max_rounds)):
        start = with_lengths(tm.tree, tm.traversal.brlens)
        moves, scores = spr_scores(tm, radius)
        trial = rank_moves(moves, scores, keep)
        if not trial:
            break
        taken = None
        for rank, (n, o, u, v, dist, pre) in enumerate(trial):
            tm.set_tree(apply_spr(start, n, o, u, v))
            tm.initialise()
            lnl1 = optimise()
            if lnl1 > lnl0 + min_gain:
                taken = dict(before=lnl0, after=lnl1, move=(n, o, u, v, dist), prescore=pre,
                             rank=rank, tried=rank + 1)
                break
        if taken is None:  # no trial move improves the optimised tree: back to the round's tree
            tm.set_tree(start)
            tm.initialise()
            history.append(dict(before=lnl0, after=tm.likelihood(), move=None, prescore=None,
                                rank=None, tried=len(trial)))
            break
        history.append(taken)
        lnl0 = taken["after"]
    tree = with_lengths(tm.tree, tm.traversal.brlens)
    return tree, tm.likelihood(), history
