"""Exact gradients of lnL from per-edge joint count matrices (the reference has
none).  The device supplies, in one walk of the optimising traversal (``pu_counts_sweep``, the
``k_counts`` kernel), for every edge e = (NOD, PAR) and rate category c

    M_e[c][i][j] = sum_s pw_s (w_c e^{sigma_sc - m_s} / Z_s) A_sc(i) B_sc(j)

i the state at NOD, j the state at PAR, the end towards the root edge.  M is the derivative of
lnL in every entry of every transition matrix, so for any parameter theta of a reversible model

    dlnL/dtheta = sum_e sum_c sum_ij M_e[c][i][j] pi_j dP_c(t_e)[j][i]/dtheta              (1)
                + sum_c sum_ij M_root[c][i][j] dpi_j/dtheta P_c(t_root)[j][i]              (2)
                + sum_c (dw_c/dtheta / w_c) sum_ij M_root[c][i][j] pi_j P_c(t_root)[j][i]  (3)

"root" being row 0 of the walk.  pi stands on the PAR side: on the NOD side lnL is the same
(reversibility) but its frequency derivatives are not.  Everything here is K x K algebra in
numpy on the host; no device code.

* ``edge_counts(tm)``          the matrices of every edge
* ``branch_gradient(tm)``      dlnL/dt of every edge
* ``rate_gradient(tm)``        dlnL/dr_c and dlnL/dw_c
* ``q_gradient(tm)``           dlnL/dQ with every entry of Q free
* ``model_gradient(tm, names)`` dlnL in named model parameters

Every function leaves the model's lnL, partials and sitewise lnL valid.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from . import rate_models as RM
from . import substitution_models as SM
from .discrete_gamma import discrete_gamma
from .nni import _check

# eigenvalue pairs closer than this (relative to 1 + |lambda|) take the limit tau e^{lambda tau}
# of the divided difference: at 1e-9 the quotient would lose all but ~7 digits to cancellation,
# while the limit is off by (lambda_k - lambda_l) tau / 2 relative, below 1e-9 tau
_EIG_EQUAL = 1e-9
# relative step of the central difference that gives dr_c/dalpha (below)
_ALPHA_STEP = 1e-3


def counts_max_cat(n_states):
    """The largest category count the counts kernel takes for 2, 4 or 20 states."""
    n = N.lib().pu_counts_max_cat(int(n_states))
    if n < 0:
        raise ValueError("edge counts do not support %d states" % n_states)
    return n


def edge_counts_at(tm, node, other, length=None):
    """(counts [C][K][K], lnl) of one edge on the current partials of `node` and `other` at
    `length` (None: the edge's current length) (pu_edge_counts).  Changes nothing in the
    model."""
    _check(tm, "edge_counts_at")
    tm._ensure()
    K, C = tm.alignment.shape[2], tm.rate_model.ncat
    counts = np.zeros((C, K, K))
    lnl = ctypes.c_double()
    N.check(N.lib().pu_edge_counts(tm._ctx, int(node), int(other),
                                   -1.0 if length is None else float(length), N.ptr(counts),
                                   ctypes.byref(lnl)), tm._ctx, "pu_edge_counts")
    return counts, lnl.value


def edge_counts(tm):
    """Every edge in one pass of the optimising traversal (pu_counts_sweep): dict(edges int32
    [n][2] = (NOD, PAR), lengths [n], counts [n][C][K][K], edge_lnl [n], lnl), n = 2N - 3 edges
    in the order the traversal meets them, row 0 the root edge.  Raises ValueError if an edge's
    lnL is not finite (a pattern of likelihood 0: the matrices are then unspecified)."""
    _check(tm, "edge_counts")
    tm._ensure()
    rows = np.ascontiguousarray(tm.traversal.optimising_traversal, dtype=np.int32)
    K, C = tm.alignment.shape[2], tm.rate_model.ncat
    cap = max(2 * len(tm.names) - 3, 1)
    edges = np.zeros((cap, 2), dtype=np.int32)
    lengths = np.zeros(cap)
    counts = np.zeros((cap, C, K, K))
    lnl = np.zeros(cap)
    n = ctypes.c_int()
    N.check(N.lib().pu_counts_sweep(tm._ctx, len(rows), N.ptr(rows), N.ptr(edges),
                                    N.ptr(lengths), N.ptr(counts), N.ptr(lnl), ctypes.byref(n)),
            tm._ctx, "pu_counts_sweep")
    tm._site_valid = True
    n = n.value
    if not np.all(np.isfinite(lnl[:n])):
        raise ValueError("edge_counts: the lnL is not finite (a pattern has likelihood 0)")
    return dict(edges=edges[:n], lengths=lengths[:n], counts=counts[:n], edge_lnl=lnl[:n],
                lnl=float(lnl[0]))


# ------------------------------------------------------------------ K x K algebra
def _model_parts(tm):
    m = tm.substitution_model
    ev, el, iv = m.engine_eigen()
    return (ev, el, iv, np.asarray(m.freqs, dtype=np.float64),
            np.asarray(tm.rate_model.rates, dtype=np.float64),
            np.asarray(tm.rate_model.weights, dtype=np.float64))


def _pmats(ev, el, iv, tau):
    """P(tau) for an array tau [...]: [...][K][K]."""
    e = np.exp(el * np.asarray(tau)[..., None])
    return np.einsum("ik,...k,kj->...ij", ev, e, iv)


def _weighted(counts, pi):
    """W[e][c][j][i] = pi_j M_e[c][i][j]: dlnL/dP_c(t_e)[j][i]."""
    return pi[None, None, :, None] * np.swapaxes(counts, 2, 3)


def divided_differences(el, tau):
    """Phi[k][l] = (e^{l_k tau} - e^{l_l tau}) / (l_k - l_l), tau e^{l_k tau} where the two
    eigenvalues agree within _EIG_EQUAL (1 + |l_k|) (repeated eigenvalues: JC69, K80, F81)."""
    el = np.asarray(el, dtype=np.float64)
    e = np.exp(el * tau)
    d = el[:, None] - el[None, :]
    same = np.abs(d) <= _EIG_EQUAL * (1.0 + np.abs(el)[:, None])
    # e^{max(l_k, l_l) tau} (1 - e^{-|l_k - l_l| tau}) / |l_k - l_l|: no cancellation for close
    # eigenvalues, no overflow for distant ones
    ad = np.where(same, 1.0, np.abs(d))
    quot = np.maximum(e[:, None], e[None, :]) * -np.expm1(-ad * tau) / ad
    return np.where(same, tau * e[:, None], quot)


def frechet(ev, el, iv, tau, dq):
    """The derivative of P = exp(Q tau) in the direction dQ, from the eigen-system Q = U diag(l)
    U^-1: dP = U ((U^-1 dQ U) o Phi(tau)) U^-1."""
    return ev.dot((iv.dot(dq).dot(ev)) * divided_differences(el, tau)).dot(iv)


def _q_grad(res, parts):
    """dlnL/dQ[k][l], every entry free: sum_e,c U^-T ((U^T W U^-T) o Phi(t_e r_c)) U^T."""
    ev, el, iv, pi, rates, _ = parts
    W = _weighted(res["counts"], pi)
    Wh = np.einsum("ka,ecab,lb->eckl", ev.T, W, iv)
    acc = np.zeros_like(ev)
    for e, t in enumerate(res["lengths"]):
        for c, r in enumerate(rates):
            acc += Wh[e, c] * divided_differences(el, t * r)
    return iv.T.dot(acc).dot(ev.T)


def _branch_grad(res, parts):
    ev, el, iv, pi, rates, _ = parts
    W = _weighted(res["counts"], pi)
    tau = res["lengths"][:, None] * rates[None, :]
    e = np.exp(el * tau[..., None]) * el  # Q P = U diag(l e^{l tau}) U^-1
    QP = np.einsum("ik,eck,kj->ecij", ev, e, iv)
    per = np.einsum("ecji,ecji->ec", W, QP)
    return per  # [e][c]: <W_ec, Q P_c(t_e)>


def _rate_grad(res, parts):
    ev, el, iv, pi, rates, weights = parts
    per = _branch_grad(res, parts)
    d_rate = (per * res["lengths"][:, None]).sum(axis=0)
    P0 = _pmats(ev, el, iv, res["lengths"][0] * rates)  # [c][j][i]
    s = np.einsum("cij,j,cji->c", res["counts"][0], pi, P0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_weight = np.where(weights > 0, s / weights, 0.0)
    return d_rate, d_weight


def _pi_grad(res, parts):
    """Term (2): g[j] = sum_c sum_i M_root[c][i][j] P_c(t_root)[j][i], to be dotted with
    dpi/dtheta."""
    ev, el, iv, _, rates, _ = parts
    P0 = _pmats(ev, el, iv, res["lengths"][0] * rates)
    return np.einsum("cij,cji->j", res["counts"][0], P0)


def branch_gradient(tm, res=None):
    """{(nod, par): dlnL/dt} of every edge, from (1) with dP_c/dt = r_c Q P_c."""
    res = edge_counts(tm) if res is None else res
    parts = _model_parts(tm)
    g = (_branch_grad(res, parts) * parts[4][None, :]).sum(axis=1)
    return {(int(a), int(b)): float(v) for (a, b), v in zip(res["edges"], g)}


def rate_gradient(tm, res=None):
    """(dlnL/dr_c [C], dlnL/dw_c [C]), rates and weights taken as free: (1) with dP_c/dr_c =
    t_e Q P_c, and (3)."""
    res = edge_counts(tm) if res is None else res
    return _rate_grad(res, _model_parts(tm))


def q_gradient(tm, res=None):
    """dlnL/dQ [K][K], every entry of Q taken as free (pi and the rates held)."""
    res = edge_counts(tm) if res is None else res
    return _q_grad(res, _model_parts(tm))


# ------------------------------------------------------------------ named parameters
_UP = SM._UPPER
_AY = ((1, 3), (3, 1))  # C<->T
_AR = ((0, 2), (2, 0))  # A<->G


def _mask(pairs):
    m = np.zeros((4, 4))
    for i, j in pairs:
        m[i, j] = 1.0
    return m


def model_kind(model):
    """The class that decides a model's free parameters (F84 before TN93, its base)."""
    for cls in (SM.JC69, SM.K80, SM.F81, SM.F84, SM.HKY85, SM.TN93, SM.GTR, SM.ProteinModel):
        if isinstance(model, cls):
            return cls
    raise ValueError("no parameter derivatives for model %r" % type(model).__name__)


def model_param_names(model, rate_model):
    """The parameters model_gradient / optimise_model know for this pair of models."""
    kind = model_kind(model)
    names = {SM.JC69: [], SM.K80: ["kappa"], SM.F81: ["freqs"], SM.F84: ["kappa", "freqs"],
             SM.HKY85: ["kappa", "freqs"], SM.TN93: ["alpha_y", "alpha_r", "freqs"],
             SM.GTR: ["rates", "freqs"], SM.ProteinModel: ["freqs"]}[kind][:]
    if isinstance(rate_model, (RM.GammaRateModel, RM.InvariantGammaModel)):
        names.append("alpha")
    if isinstance(rate_model, (RM.InvariantSitesModel, RM.InvariantGammaModel)):
        names.append("pinvar")
    return names


def kappa_of(model):
    """kappa of K80 / HKY85 / F84 from the TN93 rates they are built on."""
    if isinstance(model, SM.F84):
        return (model._alpha_y - 1.0) * (model.freqs[1] + model.freqs[3])
    return model._alpha_y


def _exchange_derivs(model, names):
    """{name: [dR/dparam ...]} for the exchangeability parameters in `names`, and dR/dpi_j [K]
    (None where R does not depend on pi: every model but F84)."""
    kind = model_kind(model)
    out, dr_dpi = {}, None
    if "rates" in names:
        mats = []
        for k in range(5):
            m = np.zeros((4, 4))
            m[_UP[0][k], _UP[1][k]] = m[_UP[1][k], _UP[0][k]] = 1.0
            mats.append(m)
        # the exchangeabilities are relative to GT: R = R[2][3] x (r, 1)
        out["rates"] = [m * model.rates[2, 3] for m in mats]
    if "alpha_y" in names:
        out["alpha_y"] = [_mask(_AY)]
    if "alpha_r" in names:
        out["alpha_r"] = [_mask(_AR)]
    if kind is SM.F84:
        f = model.freqs
        py, pr, k = f[1] + f[3], f[0] + f[2], kappa_of(model)
        if "kappa" in names:
            out["kappa"] = [_mask(_AY) / py + _mask(_AR) / pr]
        dr_dpi = [(-k / pr ** 2) * _mask(_AR) if j in (0, 2) else (-k / py ** 2) * _mask(_AY)
                  for j in range(4)]
    elif "kappa" in names:
        out["kappa"] = [_mask(_AY) + _mask(_AR)]
    return out, dr_dpi


def q_direction(R, pi, dR, dpi, scaled=True):
    """dQ for the direction (dR, dpi) through compute_q_matrix: q~_ij = R_ij pi_j off the
    diagonal, rows summing to zero, Q = q~ / mu with mu = -sum_i pi_i q~_ii (scale_q)."""
    K = len(pi)
    off = 1.0 - np.eye(K)
    qt = R * pi[None, :] * off
    qt[np.diag_indices(K)] = -qt.sum(axis=1)
    dqt = (dR * pi[None, :] + R * dpi[None, :]) * off
    dqt[np.diag_indices(K)] = -dqt.sum(axis=1)
    if not scaled:
        return dqt
    mu = -np.diag(qt).dot(pi)
    dmu = -(np.diag(dqt).dot(pi) + np.diag(qt).dot(dpi))
    return dqt / mu - qt * (dmu / mu ** 2)


def _is_scaled(model):
    """compute_q_matrix(scale=True) leaves -sum_i pi_i q_ii = 1; a model built with
    scale_q=False is recognised by missing that."""
    return abs(-np.diag(model.q()).dot(model.freqs) - 1.0) < 1e-9


def dgamma_dalpha(alpha, ncat):
    """d discrete_gamma(alpha, ncat)/dalpha by the five-point central difference
    (8 (f(a+h) - f(a-h)) - (f(a+2h) - f(a-2h))) / (12 h) at h = _ALPHA_STEP alpha.  The rates
    cost nothing next to a traversal, so four evaluations buy the O(h^4) rule: its truncation
    error is h^4 f^(5) / 30 ~ 3e-14 relative for a function that varies on the scale of
    alpha, and its rounding error 1.5 eps_f / h, with eps_f the accuracy of discrete_gamma
    (its incomplete-gamma series stop at 1e-14 relative or below): 1e-10 relative."""
    h = _ALPHA_STEP * alpha
    f = lambda a: np.asarray(discrete_gamma(a, ncat), dtype=np.float64)
    return (8.0 * (f(alpha + h) - f(alpha - h)) - (f(alpha + 2 * h) - f(alpha - 2 * h))) / \
        (12.0 * h)


def rate_model_derivs(rm, name):
    """(dr_c/dparam [C], dw_c/dparam [C]) of `name` in ("alpha", "pinvar")."""
    C = rm.ncat
    zero = np.zeros(C)
    if name == "alpha":
        if isinstance(rm, RM.GammaRateModel):
            return dgamma_dalpha(rm.alpha, C), zero
        if isinstance(rm, RM.InvariantGammaModel):
            dg = dgamma_dalpha(rm.alpha, C - 1) / (1.0 - rm.pinvar)
            return np.concatenate([[0.0], dg]), zero
    if name == "pinvar":
        if isinstance(rm, RM.InvariantSitesModel):
            p = rm.pinvar
            return np.array([0.0, 1.0 / (1.0 - p) ** 2]), np.array([1.0, -1.0])
        if isinstance(rm, RM.InvariantGammaModel):
            p, n = rm.pinvar, C - 1
            return (np.concatenate([[0.0], rm.rates[1:] / (1.0 - p)]),
                    np.concatenate([[1.0], np.full(n, -1.0 / n)]))
    raise ValueError("rate model %s has no parameter %r" % (type(rm).__name__, name))


def check_params(model, rate_model, params):
    valid = model_param_names(model, rate_model)
    bad = [p for p in params if p not in valid]
    if bad:
        raise ValueError("model %s with %s has no parameter %s; valid: %s" % (
            model.name, type(rate_model).__name__, ", ".join(map(repr, bad)),
            ", ".join(valid) if valid else "none"))


def model_gradient(tm, params, res=None):
    """{name: dlnL/dparam} for the named parameters of the model's substitution and rate
    models: "rates" [5] (the GTR exchangeabilities AC AG AT CG CT relative to GT), "kappa",
    "alpha_y", "alpha_r", "freqs" [K - 1] (pi_k for k < K - 1 free, the last frequency taking up
    the difference), "alpha", "pinvar".  A name the model lacks is a ValueError that lists the
    valid ones."""
    params = list(params)
    model, rm = tm.substitution_model, tm.rate_model
    check_params(model, rm, params)
    res = edge_counts(tm) if res is None else res
    parts = _model_parts(tm)
    pi = parts[3]
    K = len(pi)
    out = {}
    sub = [p for p in params if p not in ("alpha", "pinvar")]
    if sub:
        gq = _q_grad(res, parts)
        R = np.asarray(model.rates, dtype=np.float64)
        scaled = _is_scaled(model)
        dRs, dr_dpi = _exchange_derivs(model, sub)
        zero = np.zeros(K)
        for name, mats in dRs.items():
            g = [float(np.sum(gq * q_direction(R, pi, dR, zero, scaled))) for dR in mats]
            out[name] = np.array(g) if name == "rates" else g[0]
        if "freqs" in sub:
            gpi = _pi_grad(res, parts)
            g = np.zeros(K - 1)
            for k in range(K - 1):
                dpi = np.zeros(K)
                dpi[k], dpi[K - 1] = 1.0, -1.0
                dR = np.zeros((K, K))
                if dr_dpi is not None:
                    dR = dr_dpi[k] - dr_dpi[K - 1]
                g[k] = np.sum(gq * q_direction(R, pi, dR, dpi, scaled)) + gpi.dot(dpi)
            out["freqs"] = g
    if "alpha" in params or "pinvar" in params:
        d_rate, d_weight = _rate_grad(res, parts)
        for name in ("alpha", "pinvar"):
            if name in params:
                dr, dw = rate_model_derivs(rm, name)
                out[name] = float(d_rate.dot(dr) + d_weight.dot(dw))
    return {p: out[p] for p in params}
