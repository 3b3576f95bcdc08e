"""Time the tree distances on the device (pu_treedist.hip) on the bootstrap-like sets
of scripts/time_treeset.py -- one random tree and, per tree of the set, 0 to 3 random SPR moves
away from it -- with random lengths, at 50 taxa x 100, 1000 and 10 000 trees, 200 taxa x 100 and
1000 trees and 1000 taxa x 100 trees:

* the stages by HIP events (pu_treedist_kernel_ms: the tree-set stages, the weighted stage, the
  paths per tree, the integer and the fp64 path reduction) and the wall time of one call that
  asks for all four matrices; a shape whose buffers the device refuses (PU_E_NOMEM) is recorded
  as refused;
* the plain-Python restatement tests/treedist_reference.py on --host-trees trees (their keyed
  lengths and paths, then their pair distances), the per-tree part scaled by T / trees and the
  pairs by (T / trees)^2: an estimate;
* a numpy formulation on dense vectors: the keyed lengths as A [T][n + U] and
  ``np.abs(A - A[a]).sum(-1)`` / ``((A - A[a]) ** 2).sum(-1)`` per row a, the path vectors
  [T][n(n-1)/2] (int64 and fp64) likewise; the vectors themselves are taken from the device's
  results and not timed.  --numpy-rows rows are timed and scaled by T / rows where T is larger
  (the T x T x K broadcast of all rows at once does not fit the host at the larger shapes).

Medians of --reps runs after --warmup.  Nothing is asserted.  Writes profiles/treedist_times.json.

    python scripts/time_treedist.py [--shapes 50x100,50x1000,...] [--reps 5]
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
ALL = ("wrf", "kf", "path", "wpath")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-trees", type=int, default=3, dest="host_trees")
    ap.add_argument("--numpy-rows", type=int, default=20, dest="numpy_rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "treedist_times.json"))
    args = ap.parse_args()
    import torch
    import treedist_reference as D
    from phylo_utils_amd import _native as N
    from phylo_utils_amd import treeset
    from time_treeset import tree_set
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "statistic": "median", "cases": []}
    treeset.distance_profile(True)
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        edges = tree_set(n, T, 1000 * n + T)
        L = np.random.default_rng(n + T).random((T, 2 * n - 3))
        case = {"n_taxa": n, "n_trees": T}
        walls, stages, got = [], [], None
        try:
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                got = treeset.distances(edges, ALL, lengths=L, squared=True)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    walls.append(dt)
                    stages.append(treeset.distance_kernel_ms())
        except N.PhyloHipError as e:
            case["refused"] = str(e)
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
            continue
        ms = np.median(np.array(stages), axis=0)
        case["device"] = {"call_wall_ms": float(np.median(walls)), "treeset_stages_ms": float(ms[0]),
                          "weighted_ms": float(ms[1]), "paths_per_tree_ms": float(ms[2]),
                          "path2_ms": float(ms[3]), "wpath2_ms": float(ms[4])}
        # the plain-Python restatement on a few trees, scaled
        sub = min(T, args.host_trees if n < 1000 else 2)
        trees = list(edges[:sub])
        t0 = time.perf_counter()
        keys = [D.keyed("edges", t, x) for t, x in zip(trees, L)]
        ep = [D.paths("edges", t, x) for t, x in zip(trees, L)]
        t1 = time.perf_counter()
        index = {s: i for i, s in enumerate(sorted(set(s for k in keys for s in k[1])))}
        for a in range(sub):
            for b in range(sub):
                D.weighted_pair(keys[a], keys[b], index)
                D.path2_pair(ep[a][0], ep[b][0])
                D.wpath2_pair(ep[a][1], ep[b][1])
        t2 = time.perf_counter()
        case["python_restatement"] = {
            "trees_timed": sub, "per_tree_ms": (t1 - t0) * 1e3, "pairs_ms": (t2 - t1) * 1e3,
            "scaled_to_all_ms": (t1 - t0) * 1e3 * T / sub + (t2 - t1) * 1e3 * (T / sub) ** 2,
            "scaling": "per-tree part by T / trees_timed, pairs by (T / trees_timed)^2"}
        # numpy on dense vectors
        r = treeset.compare(edges, rows=0)
        A = np.zeros((T, n + r.n_unique))
        for t in range(T):
            for (a, b), u, x in zip(r.edges[t], r.edge_ids[t], L[t]):
                A[t, n + u if u >= 0 else min(a, b)] = x
        rows = min(T, args.numpy_rows)
        t0 = time.perf_counter()
        for a in range(rows):
            d = A - A[a]
            np.abs(d).sum(-1)
            (d * d).sum(-1)
        t1 = time.perf_counter()
        case["numpy_weighted"] = {"rows_timed": rows, "ms": (t1 - t0) * 1e3,
                                  "scaled_to_all_ms": (t1 - t0) * 1e3 * T / rows}
        P = n * (n - 1) // 2
        if T * P * 16 <= 8e9:
            # the path vectors: tip-to-tip edge counts and lengths by numpy on the rooted form
            # would be a third implementation; the restatement's on the timed trees stand in
            E = np.empty((T, P), dtype=np.int64)
            W = np.empty((T, P))
            for t in range(T):
                src = ep[t % sub]
                E[t], W[t] = src[0], src[1]
            t0 = time.perf_counter()
            for a in range(rows):
                d = E - E[a]
                (d * d).sum(-1)
                f = W - W[a]
                (f * f).sum(-1)
            t1 = time.perf_counter()
            case["numpy_paths"] = {"rows_timed": rows, "ms": (t1 - t0) * 1e3,
                                   "scaled_to_all_ms": (t1 - t0) * 1e3 * T / rows,
                                   "note": "reduction only, on stand-in vectors of the right shape"}
        else:
            case["numpy_paths"] = {"refused": "T P 16 bytes of path vectors exceed 8 GB"}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    treeset.distance_profile(False)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
