"""Neighbour-joining and BIONJ trees from a distance matrix on the GPU.

The reference has no tree builder; this is the link between ``distance.pairwise_distances`` and a
``TreeModel``: classic neighbour joining (Saitou-Nei in the Studier-Keppler form) and BIONJ
(Gascuel 1997, variances initialised to the distances), for one matrix or a batch of them.  Tips
are clusters ``0..n-1`` and join ``m`` creates cluster ``n + m``; the result has ``2n - 2`` nodes
and the root on an edge, the project's tree shape.

There is no host fallback: ``nj_joins`` runs the HIP kernels of ``pu_nj.hip``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .tree import Node, Tree

METHODS = {"nj": 0, "bionj": 1}


def _method(method):
    try:
        return METHODS[method]
    except (KeyError, TypeError):
        raise ValueError("method must be 'nj' or 'bionj', not %r" % (method,))


def max_lds_n(method="nj"):
    """The largest n the one-workgroup kernel (tier A) takes: the matrix (both matrices for
    BIONJ) must fit the LDS of one workgroup."""
    return int(N.lib().pu_nj_max_lds_n(_method(method)))


def _matrices(D):
    D = N.f64(D)
    if D.ndim not in (2, 3) or D.shape[-1] != D.shape[-2]:
        raise ValueError("D must be [n][n] or [B][n][n], not %r" % (D.shape,))
    return D.ndim == 2, (D[None] if D.ndim == 2 else D)


def nj_joins(D, method="nj", device=0):
    """pu_nj on `D` ([n][n], or [B][n][n] for a batch; only the upper triangle is read):
    (joins int32 [n-2][2] -- the child ids of cluster n + m --, lens [n-2][2] -- their raw branch
    lengths, which may be negative --, root int32 [2], root_len, q [n-3] -- the criterion of every
    chosen pair), each with a leading batch axis for a batch."""
    single, D3 = _matrices(D)
    B, n = D3.shape[0], D3.shape[1]
    joins = np.empty((B, max(n - 2, 0), 2), dtype=np.int32)
    lens = np.empty((B, max(n - 2, 0), 2))
    root = np.empty((B, 2), dtype=np.int32)
    root_len = np.empty(B)
    q = np.empty((B, max(n - 3, 0)))
    N.check(N.lib().pu_nj(int(device), _method(method), B, n, N.ptr(D3), N.ptr(joins),
                          N.ptr(lens), N.ptr(root), N.ptr(root_len), N.ptr(q)), None, "pu_nj")
    if single:
        return joins[0], lens[0], root[0], float(root_len[0]), q[0]
    return joins, lens, root, root_len, q


def nj_device(stream, d_D, ld, n, d_joins, d_lens, d_root, d_root_len, d_q=None, method="nj",
              n_mat=1, device=0):
    """pu_nj_device: every `d_*` is a device address (an integer), `stream` a hipStream_t handle;
    asynchronous on that stream."""
    vp = lambda x: None if x is None else ctypes.c_void_p(int(x))
    N.check(N.lib().pu_nj_device(int(device), vp(stream), _method(method), int(n_mat), int(n),
                                 vp(d_D), int(ld), vp(d_joins), vp(d_lens), vp(d_root),
                                 vp(d_root_len), vp(d_q)), None, "pu_nj_device")


def pair_matrix_device(stream, n_taxa, d_out5, d_D, ld, pairs=None, device=0):
    """pu_pair_matrix_device: the distances of pu_pair_distances_device's rows `d_out5` as the
    matrix `d_D` (device addresses), on `stream`."""
    vp = lambda x: None if x is None else ctypes.c_void_p(int(x))
    if pairs is None:
        n_pairs = n_taxa * (n_taxa - 1) // 2
    else:
        pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), dtype=np.int32)
        n_pairs = len(pairs)
    N.check(N.lib().pu_pair_matrix_device(int(device), vp(stream), int(n_taxa), n_pairs,
                                          N.ptr(pairs), vp(d_out5), vp(d_D), int(ld)), None,
            "pu_pair_matrix_device")


def _clamped(x, min_length):
    x = float(x)
    return x if min_length is None else max(x, float(min_length))


def joins_to_tree(names, joins, lens, root, root_len, min_length=None):
    """The ``tree.Tree`` of one matrix's ``nj_joins`` arrays: tip i is labelled names[i], the
    seed's two children are the ends of the root edge and the first of them carries its length
    (the second 0).  `min_length` raises shorter (or negative) lengths to it; None keeps them
    raw."""
    names = list(names)
    n = len(names)
    joins = np.asarray(joins).reshape(-1, 2)
    lens = np.asarray(lens, dtype=np.float64).reshape(-1, 2)
    if n < 3 or len(joins) != n - 2 or len(lens) != n - 2:
        raise ValueError("%d names need %d joins, not %d" % (n, n - 2, len(joins)))
    nodes = [Node(str(x)) for x in names]
    used = set()
    for (a, b), (la, lb) in zip(joins, lens):
        parent = Node()
        for c, l in ((int(a), la), (int(b), lb)):
            if not 0 <= c < len(nodes) or c in used:
                raise ValueError("join of cluster %d, which is not live" % c)
            used.add(c)
            nodes[c].length = _clamped(l, min_length)
            parent.add(nodes[c])
        nodes.append(parent)
    ra, rb = int(root[0]), int(root[1])
    if {ra, rb} & used or ra == rb or not (0 <= ra < len(nodes) and 0 <= rb < len(nodes)):
        raise ValueError("root edge (%d, %d) is not the last two clusters" % (ra, rb))
    seed = Node()
    nodes[ra].length = _clamped(root_len, min_length)
    nodes[rb].length = 0.0
    seed.add(nodes[ra])
    seed.add(nodes[rb])
    return Tree(seed)


def _two_taxa(names, d, min_length):
    seed = Node()
    seed.add(Node(str(names[0]), _clamped(d, min_length)))
    seed.add(Node(str(names[1]), 0.0))
    return Tree(seed)


def neighbour_joining(D, names, method="nj", min_length=None, device=0):
    """The NJ (or BIONJ) tree of the distance matrix `D` with tips `names`; for a batch
    [B][n][n] a list of trees.  Two taxa are joined by their distance without the library."""
    single, D3 = _matrices(D)
    names = list(names)
    if D3.shape[1] != len(names):
        raise ValueError("matrix %r for %d names" % (D3.shape[1:], len(names)))
    _method(method)
    if len(names) < 2:
        raise ValueError("a tree needs at least two taxa")
    if len(names) == 2:
        trees = [_two_taxa(names, d[0, 1], min_length) for d in D3]
    else:
        joins, lens, root, root_len, _ = nj_joins(D3, method, device)
        trees = [joins_to_tree(names, joins[b], lens[b], root[b], root_len[b], min_length)
                 for b in range(len(D3))]
    return trees[0] if single else trees
