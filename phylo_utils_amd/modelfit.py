"""Maximum-likelihood fitting of the substitution and rate model parameters, jointly with all
branch lengths, on the exact gradient of phylo_utils_amd.gradient (the reference
has none).

``optimise_model`` runs scipy's L-BFGS-B on -lnL in unconstrained coordinates: log for positive
parameters (alpha, exchangeabilities, kappa, lengths), logit for pinvar, the log-ratio to the
last state for the frequencies.  One objective call is one model upload, one traversal
(``likelihood()``) and one walk of the count kernel (``edge_counts``).
"""
from __future__ import annotations

import numpy as np

from . import gradient as G
from . import rate_models as RM
from . import substitution_models as SM

MIN_LENGTH = 1e-8   # the branch-length optimisers' lower bound (pu_optimise_sweep)
MAX_LENGTH = 100.0
# box of the other coordinates: wide enough never to bind on real data, narrow enough that a
# line search cannot reach values the model classes or the discrete Gamma refuse
_LOG_BOX = {"alpha": (np.log(0.02), np.log(100.0)), "rates": (np.log(1e-4), np.log(1e4)),
            "kappa": (np.log(1e-4), np.log(1e4)), "alpha_y": (np.log(1e-4), np.log(1e4)),
            "alpha_r": (np.log(1e-4), np.log(1e4))}
_LOGIT_BOX = (-20.0, 20.0)
_FREQ_BOX = (-12.0, 12.0)


def free_parameters(model, rate_model):
    """Every parameter optimise_model can fit for this pair of models."""
    return G.model_param_names(model, rate_model)


def _values(model, rm, params):
    """{name: current value(s)} of the named parameters."""
    out = {}
    for p in params:
        if p == "alpha" or p == "pinvar":
            out[p] = float(getattr(rm, p))
        elif p == "rates":
            out[p] = np.array(model.rates[SM._UPPER][:5] / model.rates[2, 3], dtype=float)
        elif p == "kappa":
            out[p] = float(G.kappa_of(model))
        elif p in ("alpha_y", "alpha_r"):
            out[p] = float(getattr(model, "_" + p))
        elif p == "freqs":
            f = np.asarray(model.freqs, dtype=float)
            out[p] = f / f.sum()
    return out


def build_models(model, rm, values):
    """(substitution model, rate model) of the classes of `model` and `rm` at `values` (the
    parameters not named keep their current values)."""
    kind = G.model_kind(model)
    v = dict(_values(model, rm, G.model_param_names(model, rm)), **values)
    sub = [p for p in values if p not in ("alpha", "pinvar")]
    if sub:
        f = v.get("freqs")
        if kind is SM.GTR:
            model = SM.GTR(np.append(v["rates"], 1.0), f)
        elif kind is SM.K80:
            model = SM.K80(v["kappa"])
        elif kind is SM.F81:
            model = SM.F81(f)
        elif kind is SM.F84:
            model = SM.F84(v["kappa"], f)
        elif kind is SM.HKY85:
            model = SM.HKY85(v["kappa"], f)
        elif kind is SM.TN93:
            model = SM.TN93(v["alpha_y"], v["alpha_r"], model._beta, f)
        elif kind is SM.ProteinModel:
            model = type(model)(freqs=f)
    if "alpha" in values or "pinvar" in values:
        if isinstance(rm, RM.GammaRateModel):
            rm = RM.GammaRateModel(rm.ncat, v["alpha"])
        elif isinstance(rm, RM.InvariantGammaModel):
            rm = RM.InvariantGammaModel(v["pinvar"], rm.ncat - 1, v["alpha"])
        elif isinstance(rm, RM.InvariantSitesModel):
            rm = RM.InvariantSitesModel(v["pinvar"])
    return model, rm


def model_string(model, rm):
    """The model in the grammar phy.parse_model_string reads (``GTR{...}+F{...}+G4{...}``,
    %.10g), so that it can be passed back to ``phy -m``."""
    fmt = lambda vals: "{" + ",".join("%.10g" % x for x in np.atleast_1d(vals)) + "}"
    kind = G.model_kind(model)
    s = model.name
    if kind is SM.GTR:
        s += fmt(model.rates[SM._UPPER])
    elif kind in (SM.K80, SM.HKY85, SM.F84):
        s += fmt(G.kappa_of(model))
    elif kind is SM.TN93:
        s += fmt([model._alpha_y, model._alpha_r, model._beta])
    if kind not in (SM.JC69, SM.K80):
        default = kind is SM.ProteinModel and np.array_equal(model.freqs, type(model)().freqs)
        if not default:
            s += "+F" + fmt(model.freqs)
    if isinstance(rm, RM.GammaRateModel):
        s += "+G%d" % rm.ncat + fmt(rm.alpha)
    elif not isinstance(rm, RM.UniformRateModel):
        raise ValueError("the model string grammar has no %s" % type(rm).__name__)
    return s


class _Coordinates(object):
    """The optimiser's vector x <-> named parameter values and edge lengths."""

    def __init__(self, values, edge_keys, lengths):
        self.names, self.slices, x, lo, hi = [], {}, [], [], []
        for name, val in values.items():
            if name == "freqs":
                z = np.log(val[:-1] / val[-1])
                box = _FREQ_BOX
            elif name == "pinvar":
                z = np.atleast_1d(np.log(val / (1.0 - val)))
                box = _LOGIT_BOX
            else:
                z = np.atleast_1d(np.log(val))
                box = _LOG_BOX[name]
            self.slices[name] = slice(len(x), len(x) + len(z))
            self.names.append(name)
            x.extend(np.clip(z, *box))
            lo.extend([box[0]] * len(z))
            hi.extend([box[1]] * len(z))
        self.edge_keys = list(edge_keys)
        self.n_model = len(x)
        if self.edge_keys:
            x.extend(np.log(np.clip(lengths, MIN_LENGTH, MAX_LENGTH)))
            lo.extend([np.log(MIN_LENGTH)] * len(self.edge_keys))
            hi.extend([np.log(MAX_LENGTH)] * len(self.edge_keys))
        self.x0 = np.array(x, dtype=float)
        self.bounds = list(zip(lo, hi))

    def values(self, x):
        out = {}
        for name in self.names:
            z = x[self.slices[name]]
            if name == "freqs":
                e = np.exp(np.append(z, 0.0) - max(z.max(), 0.0))
                out[name] = e / e.sum()
            elif name == "pinvar":
                out[name] = float(1.0 / (1.0 + np.exp(-z[0])))
            elif name == "rates":
                out[name] = np.exp(z)
            else:
                out[name] = float(np.exp(z[0]))
        return out

    def lengths(self, x):
        return np.maximum(np.exp(x[self.n_model:]), MIN_LENGTH)

    def chain(self, x, values, grads, length_grads):
        """The gradient in x from the gradients in the parameters (gradient.model_gradient's
        conventions) and in the lengths."""
        g = np.zeros(len(x))
        for name in self.names:
            sl, v, d = self.slices[name], values[name], np.atleast_1d(grads[name])
            if name == "freqs":
                # pi = softmax(z, 0): dpi_j/dz_k = pi_j (delta_jk - pi_k); d holds the
                # derivatives along e_j - e_last, whose coefficients are dpi_j, j < K - 1
                pj = v[:-1]
                g[sl] = pj * d - pj * d.dot(pj)
            elif name == "pinvar":
                g[sl] = d * v * (1.0 - v)
            else:
                g[sl] = d * v
        if self.edge_keys:
            g[self.n_model:] = length_grads * self.lengths(x)
        return g


def _set_lengths(tm, keys, lengths):
    for key, t in zip(keys, lengths):
        tm.traversal.brlens[key] = float(t)
    tm.update_branch_lengths()


def optimise_model(tm, params=("alpha", "rates", "freqs"), branch_lengths=True, max_iter=200,
                   lnl_tol=1e-6):
    """Fit the named model parameters and, with `branch_lengths`, all 2N - 3 lengths jointly by
    L-BFGS-B on the exact gradient.  Stops when an iteration gains less than `lnl_tol` in lnL
    (or the projected gradient vanishes), or after `max_iter` iterations.  Returns dict(lnl,
    n_iter, n_gradients, params {name: value(s)}, converged); the TreeModel then holds the
    fitted model objects and lengths, and tm.likelihood() is the returned lnl.  A name the model
    does not have is a ValueError that lists the valid ones (protein empirical models: "freqs",
    "alpha", "pinvar")."""
    from scipy.optimize import minimize

    params = list(params)
    G.check_params(tm.substitution_model, tm.rate_model, params)
    first = G.edge_counts(tm)
    keys = [tuple(sorted((int(a), int(b)))) for a, b in first["edges"]] if branch_lengths else []
    co = _Coordinates(_values(tm.substitution_model, tm.rate_model, params), keys,
                      first["lengths"])
    n_grad = [0]

    def apply(x):
        vals = co.values(x)
        if params:
            m, rm = build_models(tm.substitution_model, tm.rate_model, vals)
            tm.set_substitution_model(m)
            tm.set_rate_model(rm)
        if keys:
            _set_lengths(tm, keys, co.lengths(x))
        return vals

    def objective(x):
        vals = apply(x)
        lnl = tm.likelihood()
        res = G.edge_counts(tm)
        n_grad[0] += 1
        grads = G.model_gradient(tm, params, res) if params else {}
        lg = None
        if keys:
            bg = G.branch_gradient(tm, res)
            lg = np.array([bg[(int(a), int(b))] for a, b in res["edges"]])
        g = co.chain(x, vals, grads, lg)
        if not (np.isfinite(lnl) and np.all(np.isfinite(g))):
            raise FloatingPointError("optimise_model: lnL or its gradient is not finite at %s"
                                     % (vals,))
        return -lnl, -g

    if len(co.x0) == 0:
        return dict(lnl=tm.likelihood(), n_iter=0, n_gradients=0, params={}, converged=True)
    f0 = abs(first["lnl"])
    res = minimize(objective, co.x0, jac=True, method="L-BFGS-B", bounds=co.bounds,
                   options=dict(maxiter=max_iter, ftol=lnl_tol / max(f0, 1.0), gtol=1e-8,
                                maxls=30))
    vals = apply(res.x)  # the line search's last point need not be the best one
    return dict(lnl=tm.likelihood(), n_iter=int(res.nit), n_gradients=n_grad[0], params=vals,
                converged=bool(res.success), coordinates=np.array(res.x), _coordinates=co)


def coordinate_gradient(tm, fit):
    """The gradient of lnL in the optimiser's coordinates at the point `fit` (an
    optimise_model result) left the model in."""
    co, x = fit["_coordinates"], fit["coordinates"]
    params = co.names
    res = G.edge_counts(tm)
    grads = G.model_gradient(tm, params, res) if params else {}
    lg = None
    if co.edge_keys:
        bg = G.branch_gradient(tm, res)
        lg = np.array([bg[(int(a), int(b))] for a, b in res["edges"]])
    return co.chain(x, co.values(x), grads, lg)
