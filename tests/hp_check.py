"""The comparison of a computed quantity with the extended-precision fixtures
(tests/golden/hp_*.npz): what tests/test_gpu_hp.py applies to the device and
tests/test_hp_reference.py to the oracle and to deliberately wrong values.

For every quantity the bound is ``FACTOR * E_orc + tol_project``: E_orc the oracle's stored error
against the 50-digit value for that case and quantity, tol_project the tolerance the suite already
uses for device against oracle on that quantity.  Device and oracle are two fp64 roundings of one
formula, so their errors against the truth are draws of the same size: four times the oracle's
leaves room for that and excludes the loss of a digit; tol_project covers the cases where the
oracle happens to be exact.  The bound is applied value by value: per matrix for P, per pattern
for a site lnL, per length of an edge for lnL, d1 and d2.  A single evaluation's error at a single
value changes sign from value to value and can be small by chance, so for the site and edge
quantities the stored E_orc of a value is the largest error over several fp64 roundings of the
oracle's formula at that value (tests/hp_cases.py: three orders of the product V d V^-1, and the
tree's four rootings or the edge's two orientations); tests/test_hp_reference.py shows the
scatter that makes this necessary.
"""
import numpy as np

FACTOR = 4.0
TOL_P = 1e-15       # absolute, on an entry of P
TOL_SITE = 1e-10    # absolute, on a pattern's lnL
TOL_LNL = 1e-12     # relative, on the total lnL
TOL_DERIV = 1e-12   # of max(1, |value|), on d1 and d2 (and the lnL of an edge evaluation)


class Result(object):
    """ok, ratio = the worst error / bound, err = the worst raw error, what = a label."""

    def __init__(self, what, err, bound):
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(np.isnan(err), np.inf, err / bound)
        self.what = what
        self.ratio = float(ratio.max()) if ratio.size else 0.0
        self.err = float(np.nanmax(err)) if err.size and not np.isnan(err).all() else float("nan")
        self.ok = bool(self.ratio <= 1.0) and not bool(np.isnan(err).any())

    def __str__(self):
        return "%s: worst error / bound %.3f, worst error %.3e" % (self.what, self.ratio, self.err)


def p_errors(P, truth):
    """(max |P - truth| per matrix, max |P - truth| / |truth| per matrix over the entries whose
    true value is non-zero; 0 where there is none): [...] for P [...][K][K]."""
    d = np.abs(np.asarray(P) - truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(truth != 0, d / np.abs(truth), 0.0)
    return d.max(axis=(-1, -2)), rel.max(axis=(-1, -2))


def check_p(P, truth, E_abs, E_rel, what="P"):
    """P [...][K][K] against the truth with the stored per-matrix oracle errors: the absolute
    metric against FACTOR E_abs + TOL_P, the relative one, entry by entry, against
    FACTOR E_rel + TOL_P / |truth|.  Returns (absolute Result, relative Result)."""
    P = np.asarray(P, dtype=np.float64)
    d = np.abs(P - truth)
    a = Result(what + " abs", d.max(axis=(-1, -2)), FACTOR * E_abs + TOL_P)
    with np.errstate(invalid="ignore", divide="ignore"):
        nz = truth != 0
        rel = np.where(nz, d / np.abs(truth), np.where(np.isnan(d), np.nan, 0.0))
        bound = np.where(nz, FACTOR * E_rel[..., None, None] + TOL_P / np.abs(truth), 1.0)
    return a, Result(what + " rel", rel, bound)


def check_site(site, truth, E, what="site lnL", mask=None):
    """Per-pattern lnL against the truth: |error_p| <= FACTOR E_p + TOL_SITE on the patterns of
    `mask` (default: all); E [S]."""
    site, truth = np.asarray(site, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    m = np.ones(len(truth), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    E = np.broadcast_to(np.asarray(E, dtype=np.float64), truth.shape)
    return Result(what, np.abs(site[m] - truth[m]), FACTOR * E[m] + TOL_SITE)


def check_total(lnl, truth, E, what="lnL"):
    """The total lnL: relative error <= FACTOR E + TOL_LNL."""
    return Result(what, abs(lnl - truth) / abs(truth), FACTOR * float(E) + TOL_LNL)


def deriv_error(v, truth):
    v, truth = np.asarray(v, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return np.abs(v - truth) / np.maximum(1.0, np.abs(truth))


def check_deriv(v, truth, E, what="derivative"):
    """(lnL, d1, d2) of one edge at several lengths, [n_t][3]: error relative to max(1, |value|)
    <= FACTOR E + TOL_DERIV, value by value; E [n_t][3]."""
    return Result(what, deriv_error(v, truth), FACTOR * np.asarray(E, dtype=np.float64) + TOL_DERIV)
