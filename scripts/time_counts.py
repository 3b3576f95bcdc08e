"""Time the joint-count kernel and the gradients built on it against finite differences (DESIGN
4.18).

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4):

* k_counts_ms        HIP-event time of one k_counts launch on the root edge (median of --reps);
* counts_sweep_s     wall time of one pu_counts_sweep (TreeModel.edge_counts()): every edge's
                     matrices in host arrays and the closing traversal done (median of --sweeps);
* model_gradient_s   one sweep plus the host algebra for the model parameters alone (cfg2: alpha,
                     5 rates, 3 freqs; cfg3: alpha, 19 freqs);
* full_gradient_s    the same with all 2N - 3 branch lengths;
* fd_model_s         the baseline a user would write today, host wall time: central differences
                     through likelihood(), two evaluations per model parameter;
* fd_full_s          the same with two evaluations per branch length as well;
* fd_max_rel_diff    the largest difference between the two gradients, relative to max |g|.

With PU_COUNTS_VALU=1 in the environment the K = 20 product runs on the VALU instead of the
matrix cores (the mapping measurement of DESIGN 4.18); --out then names another file.

    python scripts/time_counts.py [--out profiles/counts_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import TreeModel, gradient, modelfit  # noqa: E402
from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}
H = 1e-5


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def fd_gradient(tm, params, lengths):
    """Central differences through likelihood(): the vector model_gradient + branch_gradient
    give, in the same order."""
    m0, rm0 = tm.substitution_model, tm.rate_model
    base = modelfit._values(m0, rm0, params)
    out = []

    def lnl_with(vals):
        m, rm = modelfit.build_models(m0, rm0, vals)
        tm.set_substitution_model(m)
        tm.set_rate_model(rm)
        return tm.likelihood()

    for name in params:
        v = np.atleast_1d(np.asarray(base[name], dtype=float))
        n = len(v) - 1 if name == "freqs" else len(v)
        for k in range(n):
            f = []
            for s in (H, -H):
                w = v.copy()
                w[k] += s
                if name == "freqs":
                    w[-1] -= s
                f.append(lnl_with({name: w if len(v) > 1 else float(w[0])}))
            out.append((f[0] - f[1]) / (2 * H))
    tm.set_substitution_model(m0)
    tm.set_rate_model(rm0)
    if lengths:
        bl = tm.traversal.brlens
        for key in lengths:
            t0, f = bl[key], []
            for s in (H, -H):
                bl[key] = t0 + s
                tm.update_branch_lengths()
                f.append(tm.likelihood())
            bl[key] = t0
            out.append((f[0] - f[1]) / (2 * H))
        tm.update_branch_lengths()
    tm.likelihood()
    return np.array(out)


def measure(name, reps, sweeps, device):
    shape = SHAPES[name]
    if shape["model"].startswith("GTR"):
        m, rm, params = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5), \
            ["alpha", "rates", "freqs"]
    else:
        m, rm, params = SM.LG(freqs=np.asarray(SM.LG().freqs) / np.sum(SM.LG().freqs)), \
            GammaRateModel(4, 0.8), ["alpha", "freqs"]
    tree, names, st = make_problem(shape["n_taxa"], shape["n_sites"], m, rm.rates, seed=1)
    tm = TreeModel(device=device)
    tm.set_alignment_codes(st.astype(np.uint8), np.eye(len(m.freqs)), names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    lnl0 = tm.likelihood()

    res = tm.edge_counts()  # warm-up: buffers, code objects
    keys = [tuple(sorted((int(a), int(b)))) for a, b in res["edges"]]
    counts_sweep_s = median_time(tm.edge_counts, sweeps)

    def grad(with_lengths):
        r = gradient.edge_counts(tm)
        g = gradient.model_gradient(tm, params, r)
        v = [np.atleast_1d(g[p]) for p in params]
        if with_lengths:
            bg = gradient.branch_gradient(tm, r)
            v.append(np.array([bg[(int(a), int(b))] for a, b in r["edges"]]))
        return np.concatenate(v)

    model_gradient_s = median_time(lambda: grad(False), sweeps)
    full_gradient_s = median_time(lambda: grad(True), sweeps)
    g = grad(True)

    nod, par = (int(v) for v in res["edges"][0])
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    ms = []
    for _ in range(reps):
        gradient.edge_counts_at(tm, nod, par)
        v = ctypes.c_double()
        N.check(N.lib().pu_counts_kernel_ms(tm._ctx, ctypes.byref(v)), tm._ctx)
        ms.append(v.value)
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")

    fd_gradient(tm, params[:1], [])  # warm-up of the model uploads
    t0 = time.perf_counter()
    fd_m = fd_gradient(tm, params, [])
    fd_model_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    fd = fd_gradient(tm, params, keys)
    fd_full_s = time.perf_counter() - t0
    return dict(shape, n_edges=len(keys), n_model_params=len(fd_m), lnl=lnl0,
                k20_mapping=("valu" if os.environ.get("PU_COUNTS_VALU") == "1" else "mfma")
                if len(m.freqs) == 20 else None,
                max_edge_lnl_rel_diff=float(np.abs(res["edge_lnl"] - lnl0).max() / abs(lnl0)),
                k_counts_ms=float(np.median(ms)), counts_sweep_s=counts_sweep_s,
                model_gradient_s=model_gradient_s, full_gradient_s=full_gradient_s,
                fd_model_s=fd_model_s, fd_full_s=fd_full_s,
                fd_max_rel_diff=float(np.abs(fd - g).max() / np.abs(g).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "counts_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {s: measure(s, args.reps, args.sweeps, args.device) for s in args.shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
