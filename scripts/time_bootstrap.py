"""Time the bootstrap of distance trees on the device (pu_bootstrap.hip) stage by stage, beside the
baseline the separate calls offer: R calls of distance.pairwise_distances(weights=W[r]) and one
nj.neighbour_joining on the batch.

Device stages run on resident buffers with HIP events around each call; warm-ups first, then the
median over the repeats: the resampled weights (pu_boot_weights_device), the counts of all
replicates with the Newton step (pu_boot_distances_device) -- and, from the events that call
records around its own launches (pu_boot_profile, pu_boot_kernel_ms), the count pass and the
Newton step each on its own --, the batch of trees (pu_nj_device) and the split support
(pu_split_support_device).  The baseline is host wall time,
its uploads included, as a caller of today's API pays it.  R = 100 at the cfg2 shape (50 taxa x
100k DNA sites, GTR + G4) and the cfg3 shape (200 taxa x 10k protein sites, LG + G4).  Writes
profiles/bootstrap_times.json.

    python scripts/time_bootstrap.py [--reps 5] [--warmup 2] [--replicates 100]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("cfg2", 50, 100000, "dna"), ("cfg3", 200, 10000, "protein")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_times.json"))
    args = ap.parse_args()
    import torch
    from phylo_utils_amd import _native as N
    from phylo_utils_amd import alignment as A
    from phylo_utils_amd import bootstrap, distance, nj, simulation
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, random_tree
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = N.lib()
    R = args.replicates
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "replicates": R, "cases": []}

    def timed(fn):
        ms = []
        for it in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if it >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    for name, n, S, kind in CASES:
        model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if kind == "dna" else SM.LG()
        table, _ = A.code_table(A.DNA if kind == "dna" else A.PROTEIN)
        K = table.shape[1]
        rm = GammaRateModel(4, 0.5)
        tree = random_tree(np.random.default_rng(n), n, 0.02, 0.3)
        names, states = simulation.simulate_alignment(tree, model, rm, S, seed=1)
        sc = np.array([int(np.where((table == np.eye(K)[k]).all(1))[0][0]) for k in range(K)])
        codes, w, _ = A.compress_codes(sc[states].astype(np.uint8), len(table), 0)
        w = N.f64(w)
        P = codes.shape[1]
        m = distance._model_args(model, rm)
        margs = (K, len(m[4]), len(table), N.ptr(N.f64(table)), N.ptr(m[0]), N.ptr(m[1]),
                 N.ptr(m[2]), N.ptr(m[3]), N.ptr(m[4]), N.ptr(m[5]))
        n_pairs = n * (n - 1) // 2
        d_codes = torch.from_numpy(codes).to(dev)
        d_w = torch.from_numpy(w).to(dev)
        d_W = torch.zeros((R, P), dtype=torch.int32, device=dev)
        d_out5 = torch.zeros((R, n_pairs, 5), dtype=torch.float64, device=dev)
        d_D = torch.zeros((R, n, n), dtype=torch.float64, device=dev)
        d_joins = torch.zeros((R, n - 2, 2), dtype=torch.int32, device=dev)
        d_lens = torch.zeros((R, n - 2, 2), dtype=torch.float64, device=dev)
        d_root = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        d_rl = torch.zeros(R, dtype=torch.float64, device=dev)
        d_sup = torch.zeros(n, dtype=torch.float64, device=dev)
        d_nok = torch.zeros(1, dtype=torch.int32, device=dev)

        def weights():
            N.check(lib.pu_boot_weights_device(0, stream, 7, 0, R, P, vp(d_w), vp(d_W), P))

        def distances(max_iter=50):
            N.check(lib.pu_boot_distances_device(
                0, stream, *margs, vp(d_codes), P, n, P, vp(d_W), P, R, n_pairs, None, 1e-5, 10.0,
                1e-10, max_iter, vp(d_out5), vp(d_D), n))

        def trees():
            N.check(lib.pu_nj_device(0, stream, 0, R, n, vp(d_D), n, vp(d_joins), vp(d_lens),
                                     vp(d_root), vp(d_rl), None))

        def support():
            N.check(lib.pu_split_support_device(0, stream, n, R, vp(d_joins), vp(d_root),
                                                vp(d_joins), vp(d_root), None, vp(d_sup),
                                                vp(d_nok)))

        case = {"case": name, "taxa": n, "sites": S, "patterns": int(P), "alphabet": kind,
                "weights_ms": timed(weights),
                "counts_and_newton_ms": timed(distances)}
        # the two stages of that call, from the events around its own launches
        N.check(lib.pu_boot_profile(0, 1))
        counts, newton = [], []
        for it in range(args.warmup + args.reps):
            distances()
            c, w_ms = ctypes.c_double(), ctypes.c_double()
            N.check(lib.pu_boot_kernel_ms(0, ctypes.byref(c), ctypes.byref(w_ms)))
            if it >= args.warmup:
                counts.append(c.value)
                newton.append(w_ms.value)
        N.check(lib.pu_boot_profile(0, 0))
        case["counts_ms"] = float(np.median(counts))
        case["newton_ms"] = float(np.median(newton))
        case["nj_ms"] = timed(trees)
        case["support_ms"] = timed(support)
        case["device_total_ms"] = (case["weights_ms"] + case["counts_and_newton_ms"]
                                   + case["nj_ms"] + case["support_ms"])
        W = d_W.cpu().numpy().view(np.uint32)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        Ds = [distance.pairwise_distances((codes, table, names), model, rm,
                                          weights=W[r].astype(np.float64))[1] for r in range(R)]
        t1 = time.perf_counter()
        nj.neighbour_joining(np.stack(Ds), names)
        t2 = time.perf_counter()
        case["baseline_distance_calls_wall_ms"] = (t1 - t0) * 1e3
        case["baseline_nj_wall_ms"] = (t2 - t1) * 1e3
        t0 = time.perf_counter()
        bootstrap.bootstrap_nj((codes, table, names), model, rm, n_replicates=R, seed=7,
                               weights=w)
        case["fused_call_wall_ms"] = (time.perf_counter() - t0) * 1e3
        case["same_bits_as_baseline"] = bool(np.array_equal(
            d_D.cpu().numpy().view(np.uint64), np.stack(Ds).view(np.uint64)))
        result["cases"].append(case)
        print(json.dumps(case))
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
