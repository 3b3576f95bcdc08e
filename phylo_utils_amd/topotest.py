"""Topology tests of candidate trees on the GPU (the reference has no topology
test): given a handful of trees -- the NJ tree, the parsimony tree, a search result, a published
topology -- which can the data reject?  RELL bootstrap proportions (Kishino et al. 1990), the KH
test (Kishino & Hasegawa 1989), the SH test (Shimodaira & Hasegawa 1999), expected likelihood
weights (Strimmer & Rambaut 2002) and the AU test (Shimodaira 2002) from one resampling of the
trees' per-pattern log-likelihoods.

* ``scaled_bootstrap_weights(w, n_draw, R)`` -- resampled weights whose rows draw `n_draw`
  columns instead of N (pu_boot_weights_scaled), the multiscale bootstrap's replicates.
* ``topology_counts(L, w, ...)`` -- the raw call (pu_topology_tests): the replicate counts of
  every block, the trees' lnL, the columns drawn per block and, when asked, the RELL sums.
* ``au_pvalue(bp, rho, R)`` -- the AU p-value of one tree from its bootstrap proportions at
  several scales; pure host code.
* ``finish(raw, R)`` -- the host finish of the rule: proportions, p-values, c-ELW.
* ``topology_tests(tm, trees, ...)`` -- the whole test on a TreeModel, which ends on the tree it
  started on.
* ``format_table(res)`` -- one line per tree, each value marked ``+`` (within the 95 % set of its
  test) or ``-`` (rejected).

The weights, the sums and the counts run in the HIP kernels of ``pu_bootstrap.hip``,
``pu_rell.hip`` and ``pu_topotest.hip``; there is no host fallback.  Only the finish -- a few
divisions, a softmax over T values per replicate and a two-parameter least-squares fit per tree
-- is host code.
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

from . import _native as N

DEFAULT_SCALES = tuple(k / 10 for k in range(5, 15))  # 0.5, 0.6, .. 1.4 (CONSEL's ten scales)
FIELDS = ("lnl", "delta", "bp", "p_kh", "p_sh", "c_elw", "p_au", "au_d", "au_c")
_NORMAL = NormalDist()
_U64 = 0xFFFFFFFFFFFFFFFF


def _weights(weights_or_n_sites):
    if np.ndim(weights_or_n_sites) == 0:
        return np.ones(int(weights_or_n_sites))
    return N.f64(weights_or_n_sites).reshape(-1)


def scaled_bootstrap_weights(weights_or_n_sites, n_draw, n_replicates, seed=0, first_replicate=0,
                             device=0):
    """pu_boot_weights_scaled: uint32 [n_replicates][S], the rows of ``bootstrap.
    bootstrap_weights`` drawn over `n_draw` columns instead of N -- an integer for all rows, or
    one per row.  Every row sums to its n_draw, a pattern of weight 0 is never drawn, a row
    depends on (seed, its replicate number, the weights, its n_draw) alone, and with n_draw = N it
    is ``bootstrap_weights``' row bit for bit."""
    R = int(n_replicates)
    w = _weights(weights_or_n_sites)
    rows = None
    if np.ndim(n_draw) != 0:
        rows = np.ascontiguousarray(n_draw, dtype=np.int64).reshape(-1)
        if len(rows) != R:
            raise ValueError("one n_draw per replicate: %d for %d" % (len(rows), R))
    out = np.empty((max(R, 0), len(w)), dtype=np.uint32)
    N.check(N.lib().pu_boot_weights_scaled(int(device), int(seed) & _U64, int(first_replicate), R,
                                           len(w), N.ptr(w), 0 if rows is not None else int(n_draw),
                                           N.ptr(rows), N.ptr(out)), None,
            "pu_boot_weights_scaled")
    return out


def topology_counts(L, weights, n_replicates=10000, scales=DEFAULT_SCALES, seed=0,
                    first_replicate=0, device=0, return_rell=False):
    """The raw call (pu_topology_tests) on `L` fp64 [T][S], the unweighted per-pattern lnL of T
    trees, and the integer pattern `weights` [S].  Returns a dict: ``counts`` uint32 [K + 1][3][T]
    (block, then best / kh / sh; the kh and sh rows of blocks above 0 are zero), ``lnl`` [T],
    ``n_draw`` int64 [K + 1], ``N`` and, with `return_rell`, ``rell`` [K + 1][R][T]."""
    L = N.f64(L)
    w = N.f64(weights).reshape(-1)
    if L.ndim != 2 or L.shape[1] != len(w):
        raise ValueError("L [T][S] and weights [S] must share S, not %r and %r"
                         % (L.shape, w.shape))
    T, S = L.shape
    R = int(n_replicates)
    sc = N.f64(() if scales is None else scales).reshape(-1)
    K = len(sc)
    counts = np.zeros((K + 1, 3, T), dtype=np.uint32)
    lnl = np.zeros(T)
    n_draw = np.zeros(K + 1, dtype=np.int64)
    rell = np.zeros((K + 1, max(R, 0), T)) if return_rell else None
    N.check(N.lib().pu_topology_tests(int(device), T, S, N.ptr(L), N.ptr(w), int(seed) & _U64,
                                      int(first_replicate), R, K, N.ptr(sc) if K else None,
                                      N.ptr(counts), N.ptr(lnl), N.ptr(n_draw), N.ptr(rell)),
            None, "pu_topology_tests")
    out = dict(counts=counts, lnl=lnl, n_draw=n_draw, N=int(n_draw[0]))
    if return_rell:
        out["rell"] = rell
    return out


def au_pvalue(bp, rho, R, bp0=None):
    """The AU p-value of one tree from its bootstrap proportions `bp` [K] at the realised scales
    `rho` [K] = n_k / N over `R` replicates each: (p_au, d, c, the number of scales used).

    z_k = -Phi^-1(bp_k); scales with bp_k <= 0 or >= 1 (a count of 0 or R) are dropped; z_k =
    d sqrt(rho_k) + c / sqrt(rho_k) is fitted by weighted least squares with weights 1 / v_k,
    v_k = bp_k (1 - bp_k) / (R phi(z_k)^2); p_au = 1 - Phi(d - c).  With fewer than two usable
    scales (or scales that do not determine the fit) d and c are NaN and p_au is 0 if `bp0` -- the
    proportion at scale 1; default: that of the scale nearest 1 -- is 0, 1 if it is 1, NaN
    otherwise."""
    bp = np.asarray(bp, dtype=np.float64).reshape(-1)
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    if bp.shape != rho.shape:
        raise ValueError("one scale per proportion")
    R = float(R)
    if bp0 is None and len(bp):
        bp0 = bp[int(np.argmin(np.abs(rho - 1.0)))]
    use = [k for k in range(len(bp)) if 0.0 < bp[k] < 1.0]
    saa = sab = sbb = saz = sbz = 0.0
    for k in use:
        z = -_NORMAL.inv_cdf(bp[k])
        v = bp[k] * (1.0 - bp[k]) / (R * _NORMAL.pdf(z) ** 2)
        a, b = math.sqrt(rho[k]), 1.0 / math.sqrt(rho[k])
        saa += a * a / v
        sab += a * b / v
        sbb += b * b / v
        saz += a * z / v
        sbz += b * z / v
    det = saa * sbb - sab * sab
    if len(use) < 2 or len(set(rho[use])) < 2 or not det > 0.0:
        nan = float("nan")
        p = 0.0 if bp0 is not None and bp0 <= 0.0 else 1.0 if bp0 is not None and bp0 >= 1.0 else nan
        return p, nan, nan, len(use)
    d = (saz * sbb - sbz * sab) / det
    c = (sbz * saa - saz * sab) / det
    return 1.0 - _NORMAL.cdf(d - c), d, c, len(use)


def finish(raw, n_replicates):
    """The host finish of DESIGN 4.24 on ``topology_counts``' dict (with ``rell`` for c-ELW;
    without it ``c_elw`` is NaN): a dict of arrays [T] -- ``lnl``, ``delta`` = max lnl - lnl,
    ``bp``, ``p_kh``, ``p_sh``, ``c_elw``, ``p_au``, ``au_d``, ``au_c`` and ``au_scales`` (the
    number of scales the AU fit used) -- plus ``counts`` and ``n_draw`` as given.  The AU fit
    uses blocks 1 .. K (none: p_au is NaN unless block 0 decides it)."""
    counts, lnl, n_draw = raw["counts"], np.asarray(raw["lnl"]), raw["n_draw"]
    R = int(n_replicates)
    T = len(lnl)
    inc = np.isfinite(lnl)
    out = dict(lnl=lnl.copy(), counts=counts, n_draw=n_draw)
    with np.errstate(invalid="ignore"):
        out["delta"] = np.where(inc, (lnl[inc].max() if inc.any() else np.nan) - lnl, np.inf)
    out["bp"] = counts[0, 0] / R
    out["p_kh"] = counts[0, 1] / R
    out["p_sh"] = counts[0, 2] / R
    elw = np.full(T, np.nan)
    if raw.get("rell") is not None:
        elw = np.zeros(T)
        if inc.any():
            x = raw["rell"][0][:, inc]  # times N / n_0 = 1
            e = np.exp(x - x.max(axis=1, keepdims=True))
            elw[inc] = (e / e.sum(axis=1, keepdims=True)).mean(axis=0)
    out["c_elw"] = elw
    rho = n_draw[1:] / float(n_draw[0])
    au = [au_pvalue(counts[1:, 0, t] / R, rho, R, bp0=counts[0, 0, t] / R) for t in range(T)]
    out["p_au"] = np.array([a[0] for a in au])
    out["au_d"] = np.array([a[1] for a in au])
    out["au_c"] = np.array([a[2] for a in au])
    out["au_scales"] = np.array([a[3] for a in au], dtype=np.int64)
    return out


def topology_tests(tm, trees, n_replicates=10000, scales=DEFAULT_SCALES, seed=0, optimise=True,
                   sweeps=1):
    """The tests of DESIGN 4.24 on the candidate `trees` (Newick strings or trees over the
    model's taxa) under `tm`'s alignment and models.  Each tree in turn is set on the model, its
    branch lengths optimised (`sweeps` passes of ``optimise_branch_lengths``) unless `optimise` is
    False, and its ``sitewise_patterns()`` kept; one call (``topology_counts``) then resamples all
    of them -- `n_replicates` replicates at scale 1 and at each of `scales` (none: no AU test) --
    and ``finish`` turns the counts into a dict of arrays [T]: ``lnl``, ``delta``, ``bp``,
    ``p_kh``, ``p_sh``, ``c_elw``, ``p_au``, ``au_d``, ``au_c`` (and ``au_scales``, ``counts``,
    ``n_draw``, ``trees``: the Newick of every tree at the lengths used, and ``site_lnl`` [T][S]:
    its ``sitewise_patterns()``).  The model is put
    back on the tree and lengths it came with, after an error too; the pattern weights must be
    non-negative integers."""
    from .tree import with_lengths
    trees = list(trees)
    if len(trees) < 2:
        raise ValueError("topology tests compare at least two trees, not %d" % len(trees))
    if getattr(tm, "ascbias", False):
        raise ValueError("topology_tests with the ascertainment correction is not implemented")
    if tm.alignment is None:
        raise ValueError("No alignment has been set")
    saved = (getattr(tm, "tree", None), getattr(tm, "traversal", None))
    had_ctx = tm._ctx is not None
    rows, newicks = [], []
    try:
        for tree in trees:
            tm.set_tree(tree)
            tm.initialise()
            if optimise:
                tm.optimise_branch_lengths(sweeps=sweeps)
            rows.append(tm.sitewise_patterns())
            newicks.append(with_lengths(tm.tree, tm.traversal.brlens).as_newick())
        raw = topology_counts(np.stack(rows), tm.siteweights, n_replicates, scales, seed,
                              device=tm.device, return_rell=True)
    finally:
        if saved[1] is not None:
            tm.tree, tm.traversal = saved
            tm._dirty = True
            if had_ctx:
                tm.initialise()
    res = finish(raw, n_replicates)
    res["trees"] = newicks
    res["site_lnl"] = np.stack(rows)
    return res


def confidence_set(values, level=0.95):
    """The trees of a proportion's confidence set (bp-RELL, c-ELW): in falling order of `values`
    until their sum reaches `level`; a boolean array."""
    values = np.asarray(values, dtype=np.float64)
    keep = np.zeros(len(values), dtype=bool)
    total = 0.0
    for t in np.argsort(-np.nan_to_num(values), kind="stable"):
        if total >= level:
            break
        keep[t] = True
        total += float(np.nan_to_num(values[t]))
    return keep


def format_table(res, au=True, alpha=0.05):
    """One line per tree: ``tree i: lnL deltaL bp-RELL p-KH p-SH c-ELW p-AU``, every value after
    deltaL followed by ``+`` (the tree stays in the test's 95 % set: a p-value of at least
    `alpha`, or membership of ``confidence_set``) or ``-`` (rejected).  Without `au`, p-AU reads
    ``-``.  A list of strings, the header first."""
    T = len(res["lnl"])
    sets = dict(bp=confidence_set(res["bp"], 1.0 - alpha),
                c_elw=confidence_set(res["c_elw"], 1.0 - alpha))
    lines = ["# tree: lnL deltaL bp-RELL p-KH p-SH c-ELW p-AU (+: in the %g%% set, -: rejected)"
             % (100.0 * (1.0 - alpha))]
    for t in range(T):
        cells = ["%.4f" % res["lnl"][t], "%.4f" % res["delta"][t]]
        for f in ("bp", "p_kh", "p_sh", "c_elw", "p_au"):
            if f == "p_au" and not au:
                cells.append("-")
                continue
            v = float(res[f][t])
            ok = bool(sets[f][t]) if f in sets else v >= alpha
            cells.append("%.4f %s" % (v, "+" if ok else "-"))
        lines.append("tree %d: %s" % (t, " ".join(cells)))
    return lines
