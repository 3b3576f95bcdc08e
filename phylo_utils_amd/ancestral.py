"""Marginal ancestral states and empirical-Bayes site rates on a TreeModel's resident partials
(the reference has neither).

While the optimising traversal stands on edge (NOD, PAR), ``partials[NOD]`` holds the subtree
below NOD and ``partials[PAR]``, re-oriented, everything else, so for a reversible model the
posterior of NOD's state at a site is a local computation over those two vectors
(``pu_ancestral_edge`` / ``pu_ancestral_sweep``, the ``k_ancestral`` kernel).  One walk of the
optimising traversal reconstructs every internal node; there is no pre-order pass.

* ``ancestral_states(tm, full=False)`` -- per pattern: the most probable state of every
  internal node, its posterior and, with `full`, all posteriors.
* ``ancestral_sequences(tm, alphabet)`` -- the same as sequences over the alignment's columns,
  with the Newick that names the internal nodes.
* ``site_rates(tm)`` -- per column: the posterior of the rate category and the mean rate.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .nni import _check
from .simulation import states_to_sequences
from .tree import Traversal, with_lengths


def ancestral_max_cat(n_states):
    """The largest category count the ancestral kernel takes for 2, 4 or 20 states."""
    n = N.lib().pu_ancestral_max_cat(int(n_states))
    if n < 0:
        raise ValueError("ancestral reconstruction does not support %d states" % n_states)
    return n


def ancestral_edge(tm, node, other, length=None, full=False):
    """The posterior of `node`'s state from the current partials of `node` and `other`, the two
    ends of one edge, at `length` (None: the edge's current length) (pu_ancestral_edge):
    dict(map_state uint8 [S], map_prob [S], lnl[, posteriors [S][K]]), per pattern.  Changes
    nothing in the model."""
    _check(tm, "ancestral_edge")
    tm._ensure()
    S, K = tm._n_patterns(), tm.alignment.shape[2]
    state = np.zeros(S, dtype=np.uint8)
    prob = np.zeros(S)
    post = np.zeros((S, K)) if full else None
    lnl = ctypes.c_double()
    N.check(N.lib().pu_ancestral_edge(tm._ctx, int(node), int(other),
                                      -1.0 if length is None else float(length), N.ptr(state),
                                      N.ptr(prob), N.ptr(post), ctypes.byref(lnl)), tm._ctx,
            "pu_ancestral_edge")
    out = dict(map_state=state, map_prob=prob, lnl=lnl.value)
    if full:
        out["posteriors"] = post
    return out


def ancestral_states(tm, full=False):
    """Every internal node in one pass of the optimising traversal (pu_ancestral_sweep).
    Returns dict(nodes int32 [n], map_state uint8 [n][S], map_prob [n][S], node_lnl [n][,
    posteriors [n][S][K]]) per pattern, n = N - 2 nodes in the order the traversal meets them
    (node indices of tm.traversal); every node_lnl is the tree's lnL.  The model's partials, lnL
    and sitewise lnL are left as a traversal leaves them."""
    _check(tm, "ancestral_states")
    tm._ensure()
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    S, K = tm._n_patterns(), tm.alignment.shape[2]
    cap = max(len(tm.names) - 2, 1)
    nodes = np.zeros(cap, dtype=np.int32)
    state = np.zeros((cap, S), dtype=np.uint8)
    prob = np.zeros((cap, S))
    post = np.zeros((cap, S, K)) if full else None
    lnl = np.zeros(cap)
    n = ctypes.c_int()
    N.check(N.lib().pu_ancestral_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(nodes),
                                       N.ptr(state), N.ptr(prob), N.ptr(post), N.ptr(lnl),
                                       ctypes.byref(n)), tm._ctx, "pu_ancestral_sweep")
    tm._site_valid = True
    n = n.value
    out = dict(nodes=nodes[:n], map_state=state[:n], map_prob=prob[:n], node_lnl=lnl[:n])
    if full:
        out["posteriors"] = post[:n]
    return out


def labelled_newick(tm, labels):
    """The Newick of the model's prepared tree at its current lengths, every internal node
    named labels[node index] (Tree.as_newick writes the labels it finds; this one sets them on
    a copy)."""
    tree = with_lengths(tm.tree, tm.traversal.brlens)
    for node, i in Traversal(tree).node_dict.items():
        if node.children:
            node.label = labels[i]
    return tree.as_newick()


def ancestral_sequences(tm, alphabet):
    """({"N<idx>": sequence}, newick): the most probable state of every internal node at every
    alignment column (patterns expanded through tm.inverse_index), keyed by the node's label,
    in the order ancestral_states meets them, and the Newick of the prepared tree with those
    labels on its internal nodes."""
    res = ancestral_states(tm)
    cols = res["map_state"][:, np.asarray(tm.inverse_index)]
    names = ["N%d" % int(v) for v in res["nodes"]]
    seqs = dict(zip(names, states_to_sequences(cols, alphabet)))
    return seqs, labelled_newick(tm, {int(v): "N%d" % int(v) for v in res["nodes"]})


def site_rates(tm):
    """(cat_posteriors [sites][C], mean_rate [sites]) per alignment column: the posterior of the
    rate category given the column, and sum_c posterior(c) rate_c (pu_site_rates, one launch on
    the root edge).  Changes nothing in the model."""
    _check(tm, "site_rates")
    tm._ensure()
    if not tm._site_valid:  # an edge call or update_partials moved the resident partials
        tm.compute_partials()
    S, C = tm._n_patterns(), tm.rate_model.ncat
    cat = np.zeros((S, C))
    rate = np.zeros(S)
    N.check(N.lib().pu_site_rates(tm._ctx, N.ptr(cat), N.ptr(rate)), tm._ctx, "pu_site_rates")
    ii = np.asarray(tm.inverse_index)
    return cat[ii], rate[ii]
