"""Simulation of alignments down a tree on the GPU -- the counterpart of the reference's
``src/simulation.pyx`` (``set_seed`` :18-19, ``weighted_choice(s)`` :21-61,
``evolve_states`` :63-87).

The reference draws from libc ``rand()``: one sequential stream that cannot be reproduced on
another machine or in parallel.  Here every draw is addressed by (seed, global site, draw
index) through Philox4x32-10 (DESIGN 4.10 gives the exact rule), so a simulated column depends
on nothing but the seed, its global site number, the tree, the lengths and the model: not on
how many sites a call asks for, where it starts, or how the sites are sharded over devices.
``seed`` replaces ``set_seed``; the choice rule is ``weighted_choice``'s comparison, with
``n - 1`` instead of 0 in the tie case no draw reaches in practice (as ``synthetic.py``).

There is no host fallback: every function here runs the HIP kernels of ``pu_simulate.hip``.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .alignment import BINARY, DNA, PROTEIN, alphabet_code
from .data import DNA_STATES, PROTEIN_STATES

_LETTERS = {DNA: DNA_STATES, PROTEIN: PROTEIN_STATES, BINARY: "01"}


def _u8(a, name):
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError("%s must be an integer array" % name)
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("%s out of the uint8 range" % name)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def evolve_states(parent_states, rate_class, probs, seed, first_site=0, draw=0, device=0,
                  layout="ckk"):
    """Child states of one branch (src/simulation.pyx:63-87): child[s] is drawn from row
    probs[rate_class[s]][parent_states[s]][:] with the uniform of (seed, first_site + s, draw).
    `probs` is [C][K][K] (layout="ckk", what ``Model.p`` returns here) or the reference's
    [K][K][C] (layout="kkc").  `rate_class` may be None for one class.  Returns uint8 [S]."""
    probs = np.asarray(probs, dtype=np.float64)
    if probs.ndim != 3:
        raise ValueError("probs must have three dimensions")
    if layout == "kkc":
        probs = probs.transpose(2, 0, 1)
    elif layout != "ckk":
        raise ValueError("layout must be 'ckk' or 'kkc'")
    probs = np.ascontiguousarray(probs)
    C, K, K2 = probs.shape
    if K != K2:
        raise ValueError("probs is not square in its state dimensions: %r" % (probs.shape,))
    parent = _u8(parent_states, "parent_states")
    cls = None if rate_class is None else _u8(rate_class, "rate_class")
    if cls is not None and len(cls) != len(parent):
        raise ValueError("rate_class and parent_states differ in length")
    out = np.empty(len(parent), dtype=np.uint8)
    N.check(N.lib().pu_evolve_states(int(device), K, C, len(parent), int(seed), int(first_site),
                                     int(draw), N.ptr(probs), N.ptr(parent), N.ptr(cls),
                                     N.ptr(out)), None, "pu_evolve_states")
    return out


def simulate_on_context(ctx, n_tips, n_nodes, C, K, n_sites, seed=0, first_site=0,
                        categories=False, ancestral=False, cum=False):
    """pu_simulate on a context: dict(tips [n_tips][n_sites] in tip-slot order, and on request
    cats [n_sites], nodes [n_nodes][n_sites], cum [n_nodes][C][K][K])."""
    n_sites = int(n_sites)
    out = dict(tips=np.empty((n_tips, max(n_sites, 0)), dtype=np.uint8))
    if categories:
        out["cats"] = np.empty(max(n_sites, 0), dtype=np.uint8)
    if ancestral:
        out["nodes"] = np.empty((n_nodes, max(n_sites, 0)), dtype=np.uint8)
    if cum:
        out["cum"] = np.empty((n_nodes, C, K, K))
    N.check(N.lib().pu_simulate(ctx, int(seed), int(first_site), n_sites, N.ptr(out["tips"]),
                                N.ptr(out.get("cats")), N.ptr(out.get("nodes")),
                                N.ptr(out.get("cum"))), ctx, "pu_simulate")
    return out


def simulate_alignment(tree, substitution_model, rate_model, n_sites, seed=0, first_site=0,
                       device=0, return_categories=False, return_ancestral=False):
    """Simulate `n_sites` columns down `tree` (newick or Tree) under the models: returns
    (names, states uint8 [n_taxa][n_sites]) and then, on request, the rate category of every
    site ([n_sites]) and the states of every node ([n_nodes][n_sites], Traversal numbering).
    No alignment is needed: the context holds one dummy coded pattern, which declares the
    schedule's tips."""
    from .tree_model import TreeModel
    tm = TreeModel(device=device, keep_partials=False)
    tm.set_tree(tree)
    names = list(tm.traversal.names)
    K = len(substitution_model.freqs)
    tm.set_alignment_codes(np.zeros((len(names), 1), dtype=np.uint8), np.ones((1, K)), names)
    tm.set_substitution_model(substitution_model)
    tm.set_rate_model(rate_model)
    tm.initialise()
    res = tm.simulate(n_sites, seed=seed, first_site=first_site,
                      return_categories=return_categories, return_ancestral=return_ancestral)
    if not (return_categories or return_ancestral):
        return names, res
    return (names,) + tuple(res)


def states_to_sequences(states, alphabet):
    """State rows uint8 [n][S] -> list of strings in the alphabet's state order
    (``data.DNA_STATES`` / ``PROTEIN_STATES``; binary: "01")."""
    letters = _LETTERS.get(alphabet_code(alphabet))
    if letters is None:
        raise ValueError("unknown alphabet %r" % (alphabet,))
    states = np.asarray(states)
    if states.size and int(states.max()) >= len(letters):
        raise ValueError("state %d is not in the alphabet" % int(states.max()))
    lut = np.frombuffer(letters.encode("ascii"), dtype=np.uint8)
    return [lut[row].tobytes().decode("ascii") for row in np.atleast_2d(states)]
