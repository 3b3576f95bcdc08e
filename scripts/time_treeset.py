"""Time the tree-set comparison on the device (pu_treeset.hip) on bootstrap-like
sets -- one random tree and, per tree of the set, 0 to 3 random SPR moves away from it -- at
50 taxa x 100, 1000 and 10 000 trees, 200 taxa x 100 and 1000 trees and 1000 taxa x 100 trees:

* the three stages by HIP events (pu_treeset_kernel_ms: splits, ids, RF) and the call's wall time,
  with the RF kernel kept (one lane per pair) and with the other one (PU_TREESET_RF=wave: one wave
  per pair);
* the host restatement tests/treeset_reference.py: its splits on at most --host-trees trees and
  its pair distances on those trees' pairs, the median of --host-reps runs after one, each
  scaled to the whole set (the figure is an estimate wherever the set is larger than that);
* the split kernel with several trees per 64-lane workgroup (PU_TREESET_GROUP=64: as many as
  fill the wave and fit the LDS) beside the mapping kept, one tree per workgroup;
* for the support use alone, at the shapes up to 200 taxa x 1000 trees: pu_split_support on the
  same trees as join arrays against ``treeset.support``, both as the wall time of the
  synchronous call (pu_split_support records no events), with the new path's stage times.

Medians of --reps runs after --warmup.  Nothing is asserted but that both RF kernels and the
host reference agree.  Writes profiles/treeset_times.json.

    python scripts/time_treeset.py [--shapes 50x100,50x1000,...] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = "50x100,50x1000,50x10000,200x100,200x1000,1000x100"


def tree_set(n, T, seed):
    import parsimony_reference as PR
    import treeset_cases as C
    rng = np.random.default_rng(seed)
    base = np.array(PR.random_edges(rng, n), dtype=np.int32)
    return np.stack([C.random_moves(rng, base, int(rng.integers(0, 4))) for _ in range(T)])


def timed(fn, reps, warmup, ms_fn=None):
    """(last result, median wall ms, median of ms_fn() per run or None)."""
    walls, extra, out = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            walls.append(dt)
            if ms_fn:
                extra.append(ms_fn())
    return out, float(np.median(walls)), (np.median(np.array(extra), axis=0) if ms_fn else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-trees", type=int, default=40, dest="host_trees")
    ap.add_argument("--host-reps", type=int, default=3, dest="host_reps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "treeset_times.json"))
    args = ap.parse_args()
    import torch
    import treeset_cases as C
    import treeset_reference as TR
    from phylo_utils_amd import bootstrap, treeset
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "statistic": "median", "cases": []}
    treeset.profile(True)
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        edges = tree_set(n, T, 1000 * n + T)
        case = {"n_taxa": n, "n_trees": T}
        res = {}
        for kernel in ("lane", "wave"):
            if kernel == "wave":
                os.environ["PU_TREESET_RF"] = "wave"
            else:
                os.environ.pop("PU_TREESET_RF", None)
            r, wall, ms = timed(lambda: treeset.compare(edges), args.reps, args.warmup,
                                treeset.kernel_ms)
            res[kernel] = r
            case["rf_" + kernel] = {"call_wall_ms": wall, "splits_ms": float(ms[0]),
                                    "ids_ms": float(ms[1]), "rf_ms": float(ms[2])}
        os.environ.pop("PU_TREESET_RF", None)
        os.environ["PU_TREESET_GROUP"] = "64"
        _, _, ms = timed(lambda: treeset.compare(edges, rows=0), args.reps, args.warmup,
                         treeset.kernel_ms)
        os.environ.pop("PU_TREESET_GROUP")
        case["splits_ms_several_trees_per_workgroup"] = float(ms[0])
        r = res["lane"]
        case["n_unique_splits"] = int(r.n_unique)
        case["topologies"] = int(len(set(treeset.topology_classes(r))))
        case["rf_kernels_equal"] = bool(np.array_equal(r.rf, res["wave"].rf))
        # the host restatement, on a subset, scaled
        sub = min(T, args.host_trees)
        host = []
        for _ in range(1 + args.host_reps):  # the first run warms up and is dropped
            t0 = time.perf_counter()
            per = [TR.edge_splits("edges", e) for e in edges[:sub]]
            t1 = time.perf_counter()
            sets = [frozenset(s for s in p if s is not None) for p in per]
            rf = [[len(a ^ b) for b in sets] for a in sets]
            t2 = time.perf_counter()
            host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        h_splits, h_pairs = (float(x) for x in np.median(np.array(host[1:]), axis=0))
        case["host_reference"] = {
            "trees_timed": sub, "runs": args.host_reps, "splits_ms": h_splits, "pairs_ms": h_pairs,
            "scaled_to_all_ms": h_splits * T / sub + h_pairs * (T / sub) ** 2,
            "scaled": sub < T,
            "equal": bool(np.array_equal(np.array(rf), r.rf[:sub, :sub]))}
        # the support use alone against pu_split_support
        if n <= 200 and T <= 1000:
            rng = np.random.default_rng(n + T)
            enc = [C.as_joins(rng, e) for e in edges]
            joins = np.stack([x[0] for x in enc]).astype(np.int32)
            roots = np.stack([x[1] for x in enc]).astype(np.int32)
            ref, reps = (joins[0], roots[0]), (joins[1:], roots[1:])
            (want, _), wall_old, _ = timed(lambda: bootstrap.split_support(ref, reps), args.reps,
                                           args.warmup)
            (got, _), wall_new, ms = timed(
                lambda: treeset.support(ref, reps, form="joins"), args.reps, args.warmup,
                treeset.kernel_ms)
            live = got[~np.isnan(got)]
            case["support_only"] = {
                "replicates": T - 1, "pu_split_support_call_wall_ms": wall_old,
                "treeset_support_call_wall_ms": wall_new, "treeset_splits_ms": float(ms[0]),
                "treeset_ids_ms": float(ms[1]),
                "equal": bool(np.array_equal(np.sort(live), np.sort(want)))}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    treeset.profile(False)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
