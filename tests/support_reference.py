"""CPU restatement of the branch supports for the tests, composed from what
exists: ``nni_reference.sweep`` for the optimised central lengths t*, ``nni_reference.
quartet_ends`` + the oracle's ``edge_lnl`` for the per-pattern log-likelihoods s_k,
``boot_reference.weights`` for the resampled weights W (bit-exact with the device by DESIGN
4.14), ``math.fsum`` for the RELL sums and the formulas of the rule for the four values.  `orc`
is the oracle module (the ``oracle_mod`` fixture).

Test infrastructure: nothing under ``phylo_utils_amd/`` imports it."""
import math

import numpy as np

import boot_reference as BR
import nni_reference as NR


def site_lnl(orc, P, S, nodes, lens, t, e):
    """pu_quartet_site_lnl: [3][S] at central lengths t[3] (None: lens[4])."""
    tt = [lens[4]] * 3 if t is None else t
    out = []
    for k in range(3):
        L, sL, R, sR = NR.quartet_ends(orc, P, S, nodes, lens, k, e)
        out.append(orc.edge_lnl(L, sL, R, sR, e["evecs"], e["evals"], e["ivecs"], tt[k],
                                e["rates"], e["weights"], e["freqs"]))
    return np.array(out)


def rell(u, s):
    """B(u, s) = sum_p u[p] s[p], exactly rounded; a zero weight adds nothing."""
    terms = [int(a) * float(b) for a, b in zip(u, s) if int(a) != 0]
    if all(math.isfinite(x) for x in terms):
        return math.fsum(terms)
    return float(np.sum(terms))  # -inf, or NaN where the terms say so


def supports(s3, w, W, epsilon=0.05):
    """The rule on one edge: s3 [3][S] per-pattern lnL, w [S] integer pattern weights, W [R][S]
    replicate weights.  dict(l [3], B [R][3], d, gaps [R], count, lrt, alrt_chi2, abayes,
    sh_alrt)."""
    w = np.asarray(w)
    assert np.all(w == np.floor(w)) and np.all(w >= 0)
    l = np.array([rell(w, s3[k]) for k in range(3)])
    B = np.array([[rell(u, s3[k]) for k in range(3)] for u in W]).reshape(len(W), 3)
    out = dict(l=l, B=B)
    if not math.isfinite(l[0]):
        nan = float("nan")
        out.update(d=nan, gaps=np.full(len(W), nan), count=0, lrt=nan, alrt_chi2=nan, abayes=nan,
                   sh_alrt=nan)
        return out
    d = l[0] - max(l[1], l[2])
    gaps = []
    for b in B:
        # an arrangement whose l_k is not finite never wins: its centred sum is -inf
        c = sorted((b[k] - l[k] if math.isfinite(l[k]) else -math.inf for k in range(3)),
                   reverse=True)
        gaps.append(c[0] - c[1] if math.isfinite(c[1]) else math.inf)
    gaps = np.array(gaps)
    count = int(sum(d > g + epsilon for g in gaps))
    lrt = 2.0 * max(d, 0.0)
    out.update(d=d, gaps=gaps, count=count, lrt=lrt, alrt_chi2=math.erf(math.sqrt(lrt / 2.0)),
               abayes=1.0 / sum(math.exp(x - l[0]) for x in l), sh_alrt=count / len(W))
    return out


def branch_support(orc, tips, tr, e, w, n_rep, seed=0, epsilon=0.05, first_rep=0, tol=1e-8,
                   max_iter=50):
    """pu_branch_support: (quartets [n][6], scores [n][3][2], per edge the dict of ``supports``,
    W [n_rep][S])."""
    w = np.asarray(w, dtype=np.float64)
    _, quartets, scores = NR.sweep(orc, tips, tr, e, tol, max_iter, site_weights=w)
    W = BR.weights(w, n_rep, seed, first_rep)
    st = NR.state(orc, tips, tr, e, w)
    P, S = st["partials"], st["scale"]
    pm = lambda t: orc.pmatrix(e["evecs"], e["evals"], e["ivecs"], t, e["rates"])
    res, i = [], 0
    for row in tr.optimising_traversal:  # NR.sweep's walk
        if row[0] >= 0:
            p, x, y = (int(v) for v in row[:3])
            cml = np.zeros(S[p].shape)
            P[p] = orc.clv_c(pm(tr.brlens[p, x]), pm(tr.brlens[p, y]), P[x], P[y], S[x], S[y], cml)
            S[p] = cml
        if i < len(quartets) and (int(row[3]), int(row[4])) == tuple(int(v) for v in quartets[i][:2]):
            nod, par = int(row[3]), int(row[4])
            nodes = tuple(int(v) for v in quartets[i][2:])
            lens = [tr.brlens[nodes[0], nod], tr.brlens[nodes[1], nod], tr.brlens[nodes[2], par],
                    tr.brlens[nodes[3], par], tr.brlens[nod, par]]
            s3 = site_lnl(orc, P, S, nodes, lens, [scores[i][k][0] for k in range(3)], e)
            res.append(supports(s3, w, W, epsilon))
            i += 1
    assert i == len(quartets)
    return quartets, scores, res, W
