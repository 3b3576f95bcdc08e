"""Time the ancestral reconstruction pass against the host baseline.

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4):

* k_ancestral_ms   HIP-event time of one k_ancestral launch with all posteriors written (median
                   of --reps launches);
* sweep_s          wall time of one pu_ancestral_sweep (TreeModel.ancestral_states()): every
                   internal node's MAP state and its posterior, in host arrays when the clock
                   stops (median of --sweeps calls);
* sweep_full_s     the same with all posteriors [N - 2][S][K] copied back as well;
* site_rates_s     wall time of one TreeModel.site_rates();
* baseline_s       what the library offered before: update_partials per re-orientation row,
                   node_partials of both ends of every reconstructed node, and the formulas in
                   numpy on the host -- the same result as sweep_full_s;
* ratio            baseline_s / sweep_full_s.

Every time covers the full result on the host, never a read-back of one number.

    python scripts/time_ancestral.py [--out profiles/ancestral_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import TreeModel, ancestral  # noqa: E402
from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}


def host_posterior(A, sA, B, sB, pm, freqs, weights):
    """The formulas of DESIGN 4.16 in numpy: q [S][K] from the two ends' partials."""
    g = freqs[None, None, :] * A * np.einsum("cij,scj->sci", pm, B)
    F = g.sum(axis=2)
    sigma = sA + sB
    we = weights[None, :] * np.exp(sigma - sigma.max(axis=1)[:, None])
    return (we[:, :, None] * g).sum(axis=1) / (we * F).sum(axis=1)[:, None]


def baseline(tm, m, rm):
    """Every internal node's posteriors through the calls of the library without the kernel."""
    tr = tm.traversal
    internal = set(int(p) for p in tr.postorder_traversal[:, 0])
    freqs, weights = np.asarray(m.freqs, dtype=float), np.asarray(rm.weights, dtype=float)
    out = {}

    def visit(n, o):
        if n in internal:
            (A, sA), (B, sB) = tm.node_partials(n), tm.node_partials(o)
            out[n] = host_posterior(A, sA, B, sB, m.p(tr.brlens[n, o], rm.rates), freqs, weights)

    for k, row in enumerate(tr.optimising_traversal):
        if row[0] >= 0:
            p, x, y = (int(v) for v in row[:3])
            tm.update_partials([row[:3]], [[tr.brlens[p, x], tr.brlens[p, y]]])
        if row[3] >= 0:
            visit(int(row[3]), int(row[4]))
            if k == 0:
                visit(int(row[4]), int(row[3]))
    tm.compute_partials()
    return out


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def measure(name, reps, sweeps, device):
    shape = SHAPES[name]
    if shape["model"].startswith("GTR"):
        m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    else:
        m, rm = SM.LG(), GammaRateModel(4, 0.8)
    tree, names, st = make_problem(shape["n_taxa"], shape["n_sites"], m, rm.rates, seed=1)
    tm = TreeModel(device=device)
    tm.set_alignment_codes(st.astype(np.uint8), np.eye(len(m.freqs)), names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    lnl0 = tm.likelihood()

    full = tm.ancestral_states(full=True)  # warm-up: buffers, code objects
    sweep_s = median_time(tm.ancestral_states, sweeps)
    sweep_full_s = median_time(lambda: tm.ancestral_states(full=True), sweeps)
    tm.site_rates()
    site_rates_s = median_time(tm.site_rates, sweeps)

    # one launch, timed by HIP events inside the library, on the root edge's internal end
    left, right = (int(v) for v in tm.traversal.root_edge)
    n, o = (left, right) if left in full["nodes"] else (right, left)
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    ms = []
    for _ in range(reps):
        ancestral.ancestral_edge(tm, n, o, full=True)
        v = ctypes.c_double()
        N.check(N.lib().pu_ancestral_kernel_ms(tm._ctx, ctypes.byref(v)), tm._ctx)
        ms.append(v.value)
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")

    t0 = time.perf_counter()
    base = baseline(tm, m, rm)
    baseline_s = time.perf_counter() - t0
    err = max(float(np.abs(base[int(v)] - q).max()) for v, q in zip(full["nodes"],
                                                                   full["posteriors"]))
    return dict(shape, n_internal_nodes=len(full["nodes"]), lnl=lnl0,
                max_node_lnl_rel_diff=float(np.abs(full["node_lnl"] - lnl0).max() / abs(lnl0)),
                k_ancestral_ms=float(np.median(ms)), sweep_s=sweep_s, sweep_full_s=sweep_full_s,
                site_rates_s=site_rates_s, baseline_s=baseline_s,
                ratio=baseline_s / sweep_full_s, max_abs_diff_vs_baseline=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ancestral_times.json"))
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
