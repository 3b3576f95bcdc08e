"""Time likelihood mapping on the device (pu_lmap.hip) on alignments simulated by
the library on random trees and compressed to patterns: Q = 1250 quartets (25 n) at 50 taxa x
100 000 DNA sites under GTR+G4, and Q = 5000 at 200 taxa x 10 000 protein sites under LG+G4.

* the bin launch and the optimiser launch under each feed that applies (PU_LMAP_FEED=bins and
  patterns; protein rows use 20 codes, so only the patterns) by HIP events (pu_lmap_kernel_ms), and
  the wall time of the whole call ``lmap.quartet_likelihoods``;
* the mean rounds and evaluations per topology;
* the baseline, what the library offered before: per (quartet, topology) a ``TreeModel`` on the
  four rows with the explicit tree, ``optimise_branch_lengths`` to the same tol with as many sweeps
  as the device's mean rounds (rounded up).  Timed on --baseline-quartets quartets and scaled to
  Q: an estimate, said to be scaled.

Medians of --reps runs after --warmup.  Nothing is asserted but that the feeds agree to rounding.
Writes profiles/lmap_times.json.

    python scripts/time_lmap.py [--shapes 50x100000x4x1250,200x10000x20x5000] [--reps 5]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "50x100000x4x1250,200x10000x20x5000"
TOPOLOGY = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2))


def models(K):
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
    sub = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if K == 4 else SM.LG()
    return sub, GammaRateModel(4, 0.7)


def baseline(codes, w, K, quartets, tol, sweeps):
    """Seconds for the three topologies of `quartets` through TreeModel, and their lnL."""
    from phylo_utils_amd import TreeModel
    sub, rm = models(K)
    names = ["p", "q", "r", "s"]
    lnl = np.zeros((len(quartets), 3))
    t0 = time.perf_counter()
    for i, quartet in enumerate(quartets):
        for tau in range(3):
            rows = np.ascontiguousarray(codes[[quartet[k] for k in TOPOLOGY[tau]]])
            tm = TreeModel()
            tm.set_tree("((p:0.1,q:0.1):0.1,r:0.1,s:0.1);")
            tm.set_alignment_codes(rows, np.eye(K), names, siteweights=w)
            tm.set_substitution_model(sub)
            tm.set_rate_model(rm)
            tm.initialise()
            lnl[i, tau] = tm.optimise_branch_lengths(tol=tol, sweeps=sweeps)
    return time.perf_counter() - t0, lnl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="taxa x sites x states x quartets")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--baseline-quartets", type=int, default=20, dest="baseline_quartets")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmap_times.json"))
    args = ap.parse_args()

    from phylo_utils_amd import _native as N
    from phylo_utils_amd import alignment as A
    from phylo_utils_amd import lmap, simulation
    from phylo_utils_amd.synthetic import random_tree
    if N.device_count() < 1:
        raise SystemExit("time_lmap.py: no HIP device")
    tol = 1e-8
    results = []
    for shape in args.shapes.split(","):
        n, S, K, Q = (int(x) for x in shape.split("x"))
        sub, rm = models(K)
        tree = random_tree(np.random.default_rng(n + S), n)
        _, states = simulation.simulate_alignment(tree, sub, rm, S, seed=1)
        codes, w, _ = A.compress_codes(np.ascontiguousarray(states), K)
        w = np.asarray(w, dtype=np.float64)
        quartets = lmap.draw_quartets(n, Q, seed=1)
        row = dict(n_taxa=n, n_sites=S, n_patterns=int(codes.shape[1]), n_states=K,
                   n_quartets=int(len(quartets)), model="GTR+G4" if K == 4 else "LG+G4", tol=tol,
                   max_rounds=10, min_gain=1e-6)
        last = {}
        lmap.profile(True)
        try:
            for feed in (("bins", "patterns") if K == 4 else ("patterns",)):
                os.environ["PU_LMAP_FEED"] = feed
                walls, ms = [], []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    out = lmap.quartet_likelihoods((codes, np.eye(K)), quartets, sub, rm, w,
                                                   tol=tol)
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= args.warmup:
                        walls.append(dt)
                        ms.append(lmap.kernel_ms())
                last[feed] = out
                b, o = np.median(np.array(ms), axis=0)
                row[feed] = dict(bins_ms=float(b), opt_ms=float(o),
                                 call_wall_ms=float(np.median(walls)),
                                 opt_ms_runs=[float(m[1]) for m in ms],
                                 mean_rounds=float(out[:, :, 6].mean()),
                                 mean_evaluations=float(out[:, :, 7].mean()))
                print(feed, json.dumps(row[feed]), flush=True)
        finally:
            lmap.profile(False)
            os.environ.pop("PU_LMAP_FEED", None)
        if K == 4:
            np.testing.assert_allclose(last["bins"][:, :, 0], last["patterns"][:, :, 0], rtol=1e-9)
            row["faster_feed"] = min(("bins", "patterns"),
                                     key=lambda f: row[f]["bins_ms"] + row[f]["opt_ms"])
        else:
            row["faster_feed"] = "patterns (20 codes in use: the bins do not apply)"
        res = lmap.LikelihoodMap(quartets, last["patterns"])
        row["resolved_pct"] = res.summary["resolved_pct"]
        nb = min(args.baseline_quartets, len(quartets))
        sweeps = int(math.ceil(row["patterns"]["mean_rounds"]))
        baseline(codes, w, K, quartets[:1], tol, sweeps)  # warm-up
        secs, lnl = baseline(codes, w, K, quartets[:nb], tol, sweeps)
        row["treemodel_baseline"] = dict(
            quartets_run=nb, sweeps=sweeps, seconds_run=secs,
            seconds_scaled=secs * len(quartets) / nb,
            max_lnl_gap=float(np.abs(lnl - last["patterns"][:nb, :, 0]).max()),
            note="timed on %d of %d quartets and scaled" % (nb, len(quartets)))
        results.append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="likelihood mapping, DESIGN 4.30; medians of %d runs after %d"
                            % (args.reps, args.warmup), shapes=results), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
