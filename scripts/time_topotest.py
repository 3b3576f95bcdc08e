"""Time the topology-test call and its three stages against what the library offered before
(DESIGN 4.24).  Nothing here is a pass mark.

For the cfg2 (100k DNA sites) and cfg3 (10k protein sites) pattern counts, unit weights, T = 10
and T = 100 trees, R = --replicates (10000) replicates per block and the ten default scales
(11 R rows in all), on synthetic per-pattern lnL rows (a common row plus small differences: the
call does not look at where L came from):

* weights_ms / rell_ms / counts_ms   HIP-event times of the weight launches, the RELL sums and
                  the k_topo_counts launches of one pu_topology_tests call, summed over its
                  ranges (pu_topotest_kernel_ms), and weights_share = weights / their sum;
* call_s          wall time of that call (uploads, the three stages, the counts coming back);
* baseline        what a user could do before: bootstrap_weights per block -- available at scale
                  1 only, so the ten scaled blocks are charged at the scale-1 block's time --, then
                  W.astype(float) @ L.T and the counts in numpy on the host.  The host product of
                  all 11 R rows does not fit a host's memory at cfg2 (88 GB of fp64 W), so it is
                  timed on --baseline-rows rows and scaled to 11 R rows; baseline_s says so by
                  being the sum of the scaled parts.

    python scripts/time_topotest.py [--out profiles/topotest_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import bootstrap, topotest  # noqa: E402

SHAPES = {"cfg2": 100000, "cfg3": 10000}  # patterns (unit weights: N = S)


def host_counts(B, lnl):
    """Block-0 counts in numpy, as a user would have written them."""
    C = B - lnl[None, :]
    T = len(lnl)
    best = np.bincount(np.argmax(B, axis=1), minlength=T)
    order = np.argsort(-lnl, kind="stable")
    u = np.where(np.arange(T) == order[0], order[1], order[0])
    kh = (C[:, u] - C >= (lnl[u] - lnl)[None, :]).sum(axis=0)
    sh = (C.max(axis=1)[:, None] - C >= (lnl.max() - lnl)[None, :]).sum(axis=0)
    return best, kh, sh


def measure(S, T, R, rows_host, device):
    rng = np.random.default_rng(S + T)
    L = -rng.gamma(2.0, 3.0, S)[None, :] + 0.05 * rng.standard_normal((T, S))
    w = np.ones(S)
    scales = topotest.DEFAULT_SCALES
    topotest.topology_counts(L, w, 8, scales, device=device)  # warm-up: code objects, buffers
    N.check(N.lib().pu_topotest_profile(device, 1), None, "pu_topotest_profile")
    t0 = time.perf_counter()
    raw = topotest.topology_counts(L, w, R, scales, seed=1, device=device)
    call_s = time.perf_counter() - t0
    ms = [ctypes.c_double() for _ in range(3)]
    N.check(N.lib().pu_topotest_kernel_ms(device, *map(ctypes.byref, ms)), None,
            "pu_topotest_kernel_ms")
    N.check(N.lib().pu_topotest_profile(device, 0), None, "pu_topotest_profile")
    weights_ms, rell_ms, counts_ms = (x.value for x in ms)
    # the baseline, on rows_host rows
    n = min(rows_host, R)
    bootstrap.bootstrap_weights(S, 2, device=device)
    t0 = time.perf_counter()
    W = bootstrap.bootstrap_weights(S, n, seed=1, device=device)
    boot_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    B = W.astype(np.float64) @ L.T
    matmul_s = time.perf_counter() - t0
    lnl = L.sum(axis=1)
    t0 = time.perf_counter()
    host_counts(B, lnl)
    counts_s = time.perf_counter() - t0
    rows = (len(scales) + 1) * R
    scale_up = rows / float(n)
    baseline_s = (boot_s + matmul_s + counts_s) * scale_up
    total = weights_ms + rell_ms + counts_ms
    return dict(n_patterns=S, n_trees=T, n_replicates=R, n_scales=len(scales), rows=rows,
                weights_ms=weights_ms, rell_ms=rell_ms, counts_ms=counts_ms,
                weights_share=weights_ms / total, call_s=call_s,
                baseline_rows_timed=n, baseline_weights_s=boot_s * scale_up,
                baseline_matmul_s=matmul_s * scale_up, baseline_counts_s=counts_s * scale_up,
                baseline_s=baseline_s, ratio=baseline_s / call_s,
                baseline_note="bootstrap_weights draws scale 1 only; host parts timed on "
                              "baseline_rows_timed rows and scaled to all rows",
                bp=(raw["counts"][0, 0] / R).tolist()[:10])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "topotest_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--trees", nargs="+", type=int, default=[10, 100])
    ap.add_argument("--replicates", type=int, default=10000)
    ap.add_argument("--baseline-rows", type=int, default=256, dest="baseline_rows")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for s in args.shapes:
        for T in args.trees:
            res["%s_T%d" % (s, T)] = measure(SHAPES[s], T, args.replicates, args.baseline_rows,
                                             args.device)
            with open(args.out, "w") as fh:  # after every shape: a long run leaves what it has
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")
            print(json.dumps({"%s_T%d" % (s, T): res["%s_T%d" % (s, T)]}, sort_keys=True),
                  flush=True)


if __name__ == "__main__":
    main()
