"""Likelihood mapping (Strimmer & von Haeseler 1997): does an alignment hold
tree-like signal, and does it resolve the relation between four groups?  Many quartets of taxa
are taken; for each the three four-taxon trees ab|cd, ac|bd, ad|bc are fitted by maximum
likelihood, all five lengths each; the three lnL become posterior weights, a point in a triangle
whose corners are the resolved quartets, whose edges are net-like and whose centre is star-like.
The reference has nothing of the kind; the rule is DESIGN 4.30's.  No tree is needed.

* ``draw_quartets`` -- all quartets where there are no more than asked for, else draws of the
  library's Philox stream (counter word 3 = 3); with four clusters, one taxon of each
  (pu_lmap_quartets).
* ``quartet_likelihoods`` -- the fitted lnL, lengths, rounds and evaluations of the three
  topologies of every quartet (pu_lmap_scores, the HIP kernels of ``pu_lmap.hip``);
  ``quartet_bins`` the exact statistic its default feed runs on (pu_lmap_bins).
* ``posterior_weights``, ``regions``, ``summarise`` -- the float64 finish, done here.
* ``likelihood_mapping`` -- all of it; ``write_table`` and ``write_svg`` its outputs.

There is no host fallback: every quartet and every lnL comes from the device.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from .distance import _coded, _codes, _model_args, _weights

ATTRACTORS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [.5, 0, .5], [0, .5, .5],
                       [1 / 3., 1 / 3., 1 / 3.]])
TOPOLOGIES = ("ab|cd", "ac|bd", "ad|bc")


def default_quartets(n_taxa):
    """min(C(n, 4), 25 n): IQ-TREE's advice for the number of quartets."""
    return min(math.comb(int(n_taxa), 4), 25 * int(n_taxa))


def _cluster_array(clusters, n_taxa, names=None):
    """int32 [n_taxa] in -1..3 of an array of that form or of four lists of rows or names."""
    if clusters is None:
        return None
    if len(clusters) == 4 and not np.isscalar(clusters[0]):
        row = None if names is None else {str(x): i for i, x in enumerate(names)}
        out = np.full(n_taxa, -1, dtype=np.int32)
        for k, group in enumerate(clusters):
            for t in group:
                if isinstance(t, str):
                    if row is None or t not in row:
                        raise ValueError("cluster %d names %r, which is no taxon" % (k, t))
                    t = row[t]
                if not 0 <= int(t) < n_taxa:
                    raise ValueError("cluster %d holds row %d of %d" % (k, int(t), n_taxa))
                if out[int(t)] != -1:
                    raise ValueError("taxon %d is in two clusters" % int(t))
                out[int(t)] = k
        return out
    out = np.ascontiguousarray(clusters, dtype=np.int32).reshape(-1)
    if len(out) != n_taxa:
        raise ValueError("clusters: %d entries for %d taxa" % (len(out), n_taxa))
    return out


def draw_quartets(n_taxa, n_quartets, seed=0, clusters=None, names=None, device=0):
    """pu_lmap_quartets: int32 [min(m, n_quartets)][4], taxa (a, b, c, d) in draw order.
    `clusters`: None, an array [n_taxa] in {-1, 0, 1, 2, 3} or four lists of rows (or of `names`):
    a comes from cluster 0, b from 1, c from 2, d from 3."""
    n_taxa, Q = int(n_taxa), int(n_quartets)
    cl = _cluster_array(clusters, n_taxa, names)
    # room for what the call returns: min(m, Q) quartets, m = C(n, 4) or the clusters' product
    m = math.comb(max(n_taxa, 0), 4) if cl is None else \
        int(np.prod([int((cl == k).sum()) for k in range(4)], dtype=object))
    out = np.zeros((max(min(Q, m), 1), 4), dtype=np.int32)
    n = ctypes.c_int64(0)
    N.check(N.lib().pu_lmap_quartets(int(device), n_taxa, N.ptr(cl), Q,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, N.ptr(out), ctypes.byref(n)),
            None, "pu_lmap_quartets")
    return out[:n.value].copy()


def _quartets(quartets):
    q = np.ascontiguousarray(np.asarray(quartets).reshape(-1, 4), dtype=np.int32)
    return q, len(q)


def _t0(t0):
    if t0 is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (5,)))


def quartet_bins(codes, n_codes, quartets, weights=None, used=None, device=0):
    """pu_lmap_bins: uint64 [Q][n_used^4], entry ((u_a n + u_b) n + u_c) n + u_d the summed
    weight of the patterns where the quartet's taxa show codes used[u_a], used[u_b], used[u_c],
    used[u_d].  `used`: ascending codes (None: all n_codes)."""
    codes = _codes(codes)
    nt, S = codes.shape
    weights = _weights(weights, S)
    q, Q = _quartets(quartets)
    if used is not None:
        used = np.ascontiguousarray(used, dtype=np.uint8)
    nu = int(n_codes) if used is None else len(used)
    out = np.zeros((Q, nu ** 4), dtype=np.uint64)
    N.check(N.lib().pu_lmap_bins(int(device), N.ptr(codes), nt, S, int(n_codes), N.ptr(weights),
                                 Q, N.ptr(q), nu, N.ptr(used), N.ptr(out)), None, "pu_lmap_bins")
    return out


def quartet_likelihoods(coded_alignment, quartets, substitution_model, rate_model=None,
                        weights=None, t0=None, tol=1e-8, max_iter=50, max_rounds=10,
                        min_gain=1e-6, derivs=False, device=0):
    """pu_lmap_scores on ``(codes [n][n_pat], table [n_codes][K][, names])``: out [Q][3][8] =
    (lnL, l_p, l_q, l_r, l_s, l_i, rounds, evaluations) per quartet and topology ab|cd, ac|bd,
    ad|bc; with `derivs` also [Q][3][5][2] = (lnL', lnL'') in each length at the final lengths.
    `t0`: the five start lengths (None: 0.1).  A round optimises p, q, r, s, i in turn; rounds end
    at `max_rounds` or when one gains no more than `min_gain` (negative: never early)."""
    codes, table, _ = _coded(coded_alignment, None, None)
    nt, S = codes.shape
    weights = _weights(weights, S)
    q, Q = _quartets(quartets)
    m = _model_args(substitution_model, rate_model)
    if table.ndim != 2 or table.shape[1] != len(m[3]):
        raise ValueError("code table %r does not match the model's %d states"
                         % (table.shape, len(m[3])))
    t0 = _t0(t0)
    out = np.empty((Q, 3, 8))
    der = np.empty((Q, 3, 5, 2)) if derivs else None
    N.check(N.lib().pu_lmap_scores(
        int(device), table.shape[1], len(m[4]), len(table), N.ptr(table), N.ptr(m[0]),
        N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]), N.ptr(codes), nt, S,
        N.ptr(weights), Q, N.ptr(q), N.ptr(t0), float(tol), int(max_iter), int(max_rounds),
        float(min_gain), N.ptr(out), N.ptr(der)), None, "pu_lmap_scores")
    return (out, der) if derivs else out


def scores_device(stream, d_codes, ld, n_taxa, n_sites, table, quartets, substitution_model,
                  rate_model=None, d_weights=None, t0=None, tol=1e-8, max_iter=50, max_rounds=10,
                  min_gain=1e-6, d_out=None, d_derivs=None, device=0):
    """pu_lmap_scores_device: `d_codes`, `d_weights`, `d_out` [Q][3][8] and `d_derivs` are device
    addresses (integers), `stream` a hipStream_t handle; asynchronous on that stream."""
    table = N.f64(table)
    q, Q = _quartets(quartets)
    m = _model_args(substitution_model, rate_model)
    t0 = _t0(t0)
    vp = lambda x: None if x is None else ctypes.c_void_p(int(x))
    N.check(N.lib().pu_lmap_scores_device(
        int(device), vp(stream), table.shape[1], len(m[4]), len(table), N.ptr(table),
        N.ptr(m[0]), N.ptr(m[1]), N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]),
        vp(d_codes), int(ld), int(n_taxa), int(n_sites), vp(d_weights), Q, N.ptr(q), N.ptr(t0),
        float(tol), int(max_iter), int(max_rounds), float(min_gain), vp(d_out), vp(d_derivs)),
        None, "pu_lmap_scores_device")
    return Q


# ---- the finish (host, float64) -----------------------------------------------------------------

def posterior_weights(lnl):
    """(p [Q][3], ok [Q]) of lnL [Q][3]: p_tau = e^{lnL_tau - M} / sum e^{lnL - M}, M the
    quartet's largest lnL.  A quartet with a non-finite lnL is not ok and its weights are NaN."""
    lnl = np.asarray(lnl, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(lnl).all(axis=1)
    p = np.full(lnl.shape, np.nan)
    if ok.any():
        e = np.exp(lnl[ok] - lnl[ok].max(axis=1, keepdims=True))
        p[ok] = e / e.sum(axis=1, keepdims=True)
    return p, ok


def regions(p):
    """(seven [Q], three [Q]) int: the index of the nearest attractor (1,0,0), (0,1,0), (0,0,1),
    (1/2,1/2,0), (1/2,0,1/2), (0,1/2,1/2), (1/3,1/3,1/3) by squared Euclidean distance, and
    argmax p; the first index wins a tie.  Rows with a NaN get -1."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    seven = np.full(len(p), -1, dtype=np.int64)
    three = np.full(len(p), -1, dtype=np.int64)
    d = ((p[ok][:, None, :] - ATTRACTORS[None, :, :]) ** 2).sum(axis=2)
    seven[ok] = d.argmin(axis=1)
    three[ok] = p[ok].argmax(axis=1)
    return seven, three


def summarise(seven, three):
    """The counts and percentages of the regions over the counted quartets (region >= 0)."""
    seven, three = np.asarray(seven), np.asarray(three)
    n = int((seven >= 0).sum())
    c7 = np.array([int((seven == k).sum()) for k in range(7)])
    c3 = np.array([int((three == k).sum()) for k in range(3)])
    pct = lambda c: (100.0 * c / n) if n else np.full(len(c), np.nan)
    groups = dict(resolved=int(c7[:3].sum()), partly=int(c7[3:6].sum()), unresolved=int(c7[6]))
    out = dict(n_quartets=int(len(seven)), counted=n, left_out=int(len(seven)) - n,
               counts7=c7, pct7=pct(c7), counts3=c3, pct3=pct(c3))
    for k, v in groups.items():
        out[k] = v
        out[k + "_pct"] = 100.0 * v / n if n else float("nan")
    return out


class LikelihoodMap(object):
    """``quartets`` int32 [Q][4]; ``out`` [Q][3][8] the device's rows; ``lnl`` [Q][3];
    ``weights`` [Q][3] and ``ok`` [Q]; ``region7`` and ``region3`` [Q] (-1: left out); ``x``, ``y``
    the plotting coordinates x = p_1 + p_2 / 2, y = (sqrt(3) / 2) p_2; ``summary`` the dict of
    ``summarise``; ``names`` the taxa in row order."""

    def __init__(self, quartets, out, names=None):
        self.quartets = quartets
        self.out = out
        self.names = None if names is None else [str(x) for x in names]
        self.lnl = out[:, :, 0].copy()
        self.weights, self.ok = posterior_weights(self.lnl)
        self.region7, self.region3 = regions(self.weights)
        self.x = self.weights[:, 1] + 0.5 * self.weights[:, 2]
        self.y = (math.sqrt(3.0) / 2.0) * self.weights[:, 2]
        self.summary = summarise(self.region7, self.region3)


def likelihood_mapping(alignment_or_codes, substitution_model, rate_model=None, n_quartets=None,
                       seed=0, clusters=None, alphabet=None, table=None, weights=None,
                       compress=True, device=0, **optimiser):
    """The likelihood map of an alignment ([(name, seq)] / dict / records with `alphabet`, a code
    array with `table`, or a (codes, table[, names]) tuple): `n_quartets` quartets (None:
    ``default_quartets``) under `seed`, of the four `clusters` where given, each fitted under the
    three topologies; returns a ``LikelihoodMap``.  Site patterns are compressed first
    (``compress_codes``); `weights` (per column) skips that.  `optimiser`: t0, tol, max_iter,
    max_rounds, min_gain of ``quartet_likelihoods``."""
    codes, table, names = _coded(alignment_or_codes, alphabet, table)
    n = len(codes)
    if weights is None and compress:
        from .alignment import compress_codes
        codes, weights, _ = compress_codes(codes, len(table), device)
    Q = default_quartets(n) if n_quartets is None else int(n_quartets)
    quartets = draw_quartets(n, Q, seed, clusters, names, device)
    out = quartet_likelihoods((codes, table), quartets, substitution_model, rate_model, weights,
                              device=device, **optimiser)
    return LikelihoodMap(quartets, out, names)


# ---- outputs ------------------------------------------------------------------------------------

def write_table(result, fh):
    """A TSV, one row per quartet: its four taxa, the three lnL, the three weights, the region of
    seven and of three (NA where the quartet was left out)."""
    name = (lambda t: result.names[t]) if result.names else (lambda t: "t%d" % t)
    fh.write("a\tb\tc\td\tlnL_ab|cd\tlnL_ac|bd\tlnL_ad|bc\tp_ab|cd\tp_ac|bd\tp_ad|bc\tregion7\t"
             "region3\n")
    for q in range(len(result.quartets)):
        cells = [name(int(t)) for t in result.quartets[q]]
        cells += [repr(float(v)) for v in result.lnl[q]]
        if result.ok[q]:
            cells += [repr(float(v)) for v in result.weights[q]]
            cells += [str(int(result.region7[q])), str(int(result.region3[q]))]
        else:
            cells += ["NA"] * 5
        fh.write("\t".join(cells) + "\n")


def read_table(fh):
    """The rows of ``write_table`` back: (taxa [Q][4] names, lnl [Q][3], weights [Q][3] (NaN for
    NA), region7 [Q], region3 [Q] (-1 for NA))."""
    lines = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()][1:]
    num = lambda v: float("nan") if v == "NA" else float(v)
    reg = lambda v: -1 if v == "NA" else int(v)
    return ([r[:4] for r in lines], np.array([[float(v) for v in r[4:7]] for r in lines]).reshape(-1, 3),
            np.array([[num(v) for v in r[7:10]] for r in lines]).reshape(-1, 3),
            np.array([reg(r[10]) for r in lines], dtype=np.int64),
            np.array([reg(r[11]) for r in lines], dtype=np.int64))


def write_svg(result, fh, side=300.0):
    """Two triangles side by side: the points of the counted quartets with the percentages of the
    three regions, and the outline of the seven regions with theirs.  Corner ab|cd is bottom left,
    ac|bd bottom right, ad|bc the top: x = p_1 + p_2 / 2, y = (sqrt(3) / 2) p_2."""
    h = side * math.sqrt(3.0) / 2.0
    pad, gap = 40.0, 60.0
    s = result.summary

    def pt(x, y, ox):
        return ox + side * x, pad + h - side * y

    def bary(p, ox):
        return pt(p[1] + 0.5 * p[2], (math.sqrt(3.0) / 2.0) * p[2], ox)

    def line(a, b, ox, extra=""):
        (x1, y1), (x2, y2) = bary(a, ox), bary(b, ox)
        return '<line x1="%.2f" y1="%.2f" x2="%.2f" y2="%.2f" stroke="black"%s/>' % (x1, y1, x2, y2,
                                                                                    extra)

    def text(p, ox, label, dy=0.0):
        x, y = bary(p, ox)
        return '<text x="%.2f" y="%.2f" font-size="11" text-anchor="middle">%s</text>' % (
            x, y + dy, label)

    fmt = lambda v: "NA" if v != v else "%.1f%%" % v
    out = ['<svg xmlns="http://www.w3.org/2000/svg" width="%.0f" height="%.0f">'
           % (2 * side + 2 * pad + gap, h + 2 * pad)]
    corners = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    for ox in (pad, pad + side + gap):
        out.append('<g class="triangle">')
        for i in range(3):
            out.append(line(corners[i], corners[(i + 1) % 3], ox))
        for c, label, dy in zip(corners, TOPOLOGIES, (14.0, 14.0, -6.0)):
            out.append(text(c, ox, label.replace("|", "&#124;"), dy))
        out.append("</g>")
    ox = pad
    dash = ' stroke-dasharray="3,3"'
    centre = (1 / 3., 1 / 3., 1 / 3.)
    for mid in ((.5, .5, 0), (.5, 0, .5), (0, .5, .5)):  # argmax boundaries
        out.append(line(centre, mid, ox, dash))
    out.append('<g class="points">')
    for q in np.flatnonzero(result.ok):
        x, y = pt(float(result.x[q]), float(result.y[q]), ox)
        out.append('<circle class="quartet" cx="%.2f" cy="%.2f" r="1.5" fill="black" '
                   'fill-opacity="0.5"/>' % (x, y))
    out.append("</g>")
    for k, p in enumerate(((.6, .2, .2), (.2, .6, .2), (.2, .2, .6))):
        out.append(text(p, ox, fmt(s["pct3"][k])))
    ox = pad + side + gap
    # the bisectors between neighbouring attractors: corner / edge at 3/4, edge / centre, corner / centre
    a, b = 0.75, 0.25
    cuts = [((a, b, 0), (7 / 12., 1 / 6., 1 / 4.)), ((a, 0, b), (7 / 12., 1 / 4., 1 / 6.)),
            ((b, a, 0), (1 / 6., 7 / 12., 1 / 4.)), ((0, a, b), (1 / 4., 7 / 12., 1 / 6.)),
            ((b, 0, a), (1 / 6., 1 / 4., 7 / 12.)), ((0, b, a), (1 / 4., 1 / 6., 7 / 12.))]
    for p, q in cuts:
        out.append(line(p, q, ox, dash))
    ring = [(7 / 12., 1 / 4., 1 / 6.), (7 / 12., 1 / 6., 1 / 4.), (1 / 4., 1 / 6., 7 / 12.),
            (1 / 6., 1 / 4., 7 / 12.), (1 / 6., 7 / 12., 1 / 4.), (1 / 4., 7 / 12., 1 / 6.)]
    for i in range(6):
        out.append(line(ring[i], ring[(i + 1) % 6], ox, dash))
    spots = ((.8, .1, .1), (.1, .8, .1), (.1, .1, .8), (.45, .45, .1), (.45, .1, .45),
             (.1, .45, .45), centre)
    for k, p in enumerate(spots):
        out.append(text(p, ox, fmt(s["pct7"][k])))
    out.append('<text x="%.2f" y="%.2f" font-size="11">quartets: %d counted, %d left out</text>'
               % (pad, h + 2 * pad - 6, s["counted"], s["left_out"]))
    out.append("</svg>")
    fh.write("\n".join(out) + "\n")


def report_lines(result):
    """The ``lmap:`` lines of the command line."""
    s = result.summary
    pc = lambda v: "NA" if v != v else "%.1f" % v
    lines = ["lmap: quartets = %d (left out: %d)" % (s["n_quartets"], s["left_out"])]
    for k in range(7):
        lines.append("lmap: region %d = %d (%s %%)" % (k + 1, s["counts7"][k], pc(s["pct7"][k])))
    lines.append("lmap: resolved %d (%s %%) partly %d (%s %%) unresolved %d (%s %%)"
                 % (s["resolved"], pc(s["resolved_pct"]), s["partly"], pc(s["partly_pct"]),
                    s["unresolved"], pc(s["unresolved_pct"])))
    return lines


def profile(on, device=0):
    """Switch the event timing of the score calls on `device` on or off."""
    N.check(N.lib().pu_lmap_profile(int(device), int(bool(on))), None, "pu_lmap_profile")


def kernel_ms(device=0):
    """(bins, optimiser): the kernel times of the last score call on `device` while profiling,
    in ms, summed over its chunks."""
    b, o = ctypes.c_double(), ctypes.c_double()
    N.check(N.lib().pu_lmap_kernel_ms(int(device), ctypes.byref(b), ctypes.byref(o)), None,
            "pu_lmap_kernel_ms")
    return b.value, o.value
