"""Time the NNI scoring pass against the per-topology baseline.

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4):

* k_quartet_ms    HIP-event time of one k_quartet launch (median of --reps launches);
* sweep_s         wall time of one pu_nni_sweep (TreeModel.nni_scores): every internal edge,
                  three arrangements, central lengths optimised;
* sweep_fixed_s   the same pass with max_iter = 0: one evaluation per edge at the standing
                  length -- the information the baseline gives;
* baseline_s      wall time of set_tree + initialise + likelihood() of every one of the 2(N - 3)
                  neighbour topologies on the same TreeModel, at unchanged lengths (what the
                  library offered before the quartet kernel);
* ratio           baseline_s / sweep_s, ratio_fixed = baseline_s / sweep_fixed_s.

    python scripts/time_nni.py [--out profiles/nni_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import TreeModel  # noqa: E402
from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402
from phylo_utils_amd.tree import apply_nni  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}


def measure(name, reps, device):
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

    tm.nni_scores()  # warm-up: buffers, code objects
    t0 = time.perf_counter()
    quartets, scores = tm.nni_scores()
    sweep_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    _, fixed = tm.nni_scores(max_iter=0)
    sweep_fixed_s = time.perf_counter() - t0

    # one launch, timed by HIP events inside the library, on the first scored quartet
    q = quartets[0]
    tr = tm.traversal
    lens = [tr.brlens[int(q[2]), int(q[0])], tr.brlens[int(q[3]), int(q[0])],
            max(tr.brlens[int(q[4]), int(q[1])], 1e-8), max(tr.brlens[int(q[5]), int(q[1])], 1e-8),
            tr.brlens[int(q[0]), int(q[1])]]
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    ms = []
    for _ in range(reps):
        tm.quartet_derivatives(q[2:], lens)
        v = ctypes.c_double()
        N.check(N.lib().pu_quartet_kernel_ms(tm._ctx, ctypes.byref(v)), tm._ctx)
        ms.append(v.value)
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")

    # the baseline: a full traversal (and re-plan) per neighbour topology, unchanged lengths
    cand = [apply_nni(tree, int(e[0]), int(e[1]), k) for e in quartets for k in (1, 2)]
    tm.set_tree(cand[0])
    tm.initialise()  # warm-up of the re-bind path
    t0 = time.perf_counter()
    base = []
    for c in cand:
        tm.set_tree(c)
        tm.initialise()
        base.append(tm.likelihood())
    baseline_s = time.perf_counter() - t0
    got = fixed[:, 1:, 1].reshape(-1)
    err = float(np.max(np.abs(got - np.array(base)) / np.abs(base)))
    return dict(shape, n_internal_edges=len(quartets), n_neighbours=len(cand), lnl=lnl0,
                k_quartet_ms=float(np.median(ms)), sweep_s=sweep_s, sweep_fixed_s=sweep_fixed_s,
                evaluations=int(scores[:, :, 3].max(axis=1).sum()), baseline_s=baseline_s,
                ratio=baseline_s / sweep_s, ratio_fixed=baseline_s / sweep_fixed_s,
                max_rel_diff_fixed_vs_baseline=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "nni_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {s: measure(s, args.reps, args.device) for s in args.shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
