"""numpy / pure-Python restatement of the bootstrap specification: the resampling
rule of section 1 and the split support of section 4, written from the rule and not from the
kernels.

Test infrastructure: nothing under ``phylo_utils_amd/`` imports it.  Everything here is integer
arithmetic but the one fp64 multiply ``u * N``, so the device result can be compared exactly.
"""
import numpy as np

import sim_reference as SR

_MASK = np.uint64(0xFFFFFFFF)


def uniform(seed, j, r):
    """u of column j (array) of replicate r: the simulator's u with counter word 3 = 1."""
    j = np.atleast_1d(np.asarray(j, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = SR.philox4x32_10((j & _MASK, j >> np.uint64(32), np.uint64(r), np.uint64(1)),
                         (seed & 0xFFFFFFFF, seed >> 32))
    m = ((x[1] >> np.uint64(5)) << np.uint64(26)) | (x[0] >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def weights(weights_or_n_sites, n_rep, seed=0, first_rep=0):
    """W uint32 [n_rep][S] of replicates first_rep .. first_rep + n_rep - 1."""
    if np.ndim(weights_or_n_sites) == 0:
        w = np.ones(int(weights_or_n_sites), dtype=np.int64)
    else:
        w = np.asarray(weights_or_n_sites)
        assert np.all(w == np.floor(w)) and np.all(w >= 0)
        w = w.astype(np.int64)
    prefix = np.cumsum(w)  # inclusive, integers
    N = int(prefix[-1])
    assert 1 <= N <= 2 ** 31 - 1
    out = np.zeros((n_rep, len(w)), dtype=np.uint32)
    j = np.arange(N, dtype=np.uint64)
    for i in range(n_rep):
        u = uniform(seed, j, first_rep + i)
        c = np.minimum(np.floor(u * float(N)).astype(np.int64), N - 1)
        s = np.searchsorted(prefix, c, side="right")  # the first s with prefix[s] > c
        np.add.at(out[i], s, 1)
    return out


def splits(joins, n):
    """The canonical splits of clusters n + m, m = 0..n-4, of a tree in join form: a list of
    frozensets of tips, complemented when they hold tip 0."""
    joins = np.asarray(joins).reshape(-1, 2)
    assert len(joins) == n - 2
    every = frozenset(range(n))
    tips = [frozenset([i]) for i in range(n)]
    out = []
    for m in range(n - 3):
        a, b = (int(x) for x in joins[m])
        assert 0 <= a < n + m and 0 <= b < n + m
        s = tips[a] | tips[b]
        tips.append(s)
        out.append(every - s if 0 in s else s)
    return out


def split_support(ref_joins, rep_joins, ok=None):
    """(support [n-3], n_ok): the share of the ok replicates whose tree holds each reference
    split."""
    ref_joins = np.asarray(ref_joins).reshape(-1, 2)
    n = len(ref_joins) + 2
    rep_joins = np.asarray(rep_joins).reshape(-1, n - 2, 2)
    ok = np.ones(len(rep_joins), dtype=bool) if ok is None else np.asarray(ok) != 0
    ref = splits(ref_joins, n)
    have = [set(splits(j, n)) for j, o in zip(rep_joins, ok) if o]
    n_ok = len(have)
    with np.errstate(invalid="ignore", divide="ignore"):
        sup = np.array([np.float64(sum(s in h for h in have)) / np.float64(n_ok) for s in ref])
    return sup.reshape(-1), n_ok


def random_joins(rng, n):
    """A random tree in join form: (joins int32 [n-2][2], root int32 [2]); smaller id first."""
    live = list(range(n))
    joins = np.zeros((n - 2, 2), dtype=np.int32)
    for m in range(n - 2):
        i, j = sorted(rng.choice(len(live), 2, replace=False))
        joins[m] = (live[i], live[j])
        live = [x for k, x in enumerate(live) if k not in (i, j)] + [n + m]
    assert len(live) == 2 and live[1] == 2 * n - 3
    return joins, np.array([2 * n - 3, live[0]], dtype=np.int32)

