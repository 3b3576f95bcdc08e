"""Time the pairwise-distance kernels (pu_distance.hip) against the numpy restatement of their
specification (tests/dist_reference.py) on the cfg2 shape (50 taxa x 100k DNA sites, GTR + G4)
and the cfg3 shape (200 taxa x 10k protein sites, LG + G4).

Device: pu_pair_distances_device on resident codes, HIP events around the count launches
(k_pair_counts + the slab merge) and the k_pair_newton launches (pu_pair_profile /
pu_pair_kernel_ms); warm-ups first, then the median over the repeats.  The restatement is timed
on a sample of pairs (np.add.at counts, then brentq) and scaled to all pairs.  Writes
profiles/distance_times.json.

    python scripts/time_distances.py [--reps 10] [--warmup 3] [--ref-pairs 6]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def problem(kind, rng):
    from phylo_utils_amd import alignment as A
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
    if kind == "cfg2":
        n_taxa, S, model, table = 50, 100000, SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), A.code_table(A.DNA)[0]
    else:
        n_taxa, S, model, table = 200, 10000, SM.LG(), A.code_table(A.PROTEIN)[0]
    K = table.shape[1]
    s2c = np.array([int(np.where((table == np.eye(K)[k]).all(1))[0][0]) for k in range(K)])
    rows = [rng.integers(0, K, S)]
    for _ in range(n_taxa - 1):  # a chain of relatives: distances from small to saturated
        prev = rows[int(rng.integers(0, len(rows)))]
        rows.append(np.where(rng.random(S) < 0.15, rng.integers(0, K, S), prev))
    return s2c[np.stack(rows)].astype(np.uint8), table, model, GammaRateModel(4, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-pairs", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_times.json"))
    args = ap.parse_args()
    import torch
    import dist_reference as DR
    from phylo_utils_amd import _native as N
    from phylo_utils_amd import distance
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    for kind in ("cfg2", "cfg3"):
        rng = np.random.default_rng(1)
        codes, table, model, rm = problem(kind, rng)
        nt, S = codes.shape
        n_pairs = nt * (nt - 1) // 2
        d_codes = torch.from_numpy(codes).to(dev)
        d_out = torch.empty((n_pairs, 5), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        N.check(N.lib().pu_pair_profile(0, 1))
        counts_ms, newton_ms, wall_ms = [], [], []
        for it in range(args.warmup + args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            distance.distances_device(stream, d_codes.data_ptr(), S, nt, S, table, model, rm,
                                      d_out5=d_out.data_ptr())
            torch.cuda.synchronize(dev)
            wall = (time.perf_counter() - t0) * 1e3
            a, b = ctypes.c_double(), ctypes.c_double()
            N.check(N.lib().pu_pair_kernel_ms(0, ctypes.byref(a), ctypes.byref(b)))
            if it >= args.warmup:
                counts_ms.append(a.value)
                newton_ms.append(b.value)
                wall_ms.append(wall)
        N.check(N.lib().pu_pair_profile(0, 0))
        out5 = d_out.cpu().numpy()
        # the restatement on a sample of pairs
        pairs = DR.all_pairs(nt)
        pick = pairs[rng.choice(len(pairs), args.ref_pairs, replace=False)]
        pm = DR.PairModel(table, model, rm.rates, rm.weights)
        t0 = time.perf_counter()
        Nc = DR.counts(codes, len(table), None, pick)
        t1 = time.perf_counter()
        ref = [pm.optimum(n) for n in Nc]
        t2 = time.perf_counter()
        idx = {tuple(p): k for k, p in enumerate(map(tuple, pairs))}
        err = max(abs(out5[idx[tuple(p)], 0] - r[0]) / max(r[0], 1e-3) for p, r in zip(pick, ref))
        scale = n_pairs / float(args.ref_pairs)
        med = lambda x: float(np.median(x))
        result[kind] = {
            "n_taxa": nt, "n_sites": S, "n_codes": int(len(table)), "n_pairs": n_pairs,
            "k_pair_counts_ms_median": med(counts_ms), "k_pair_newton_ms_median": med(newton_ms),
            "call_wall_ms_median": med(wall_ms),
            "k_pair_counts_ms_all": counts_ms, "k_pair_newton_ms_all": newton_ms,
            "code_bytes_read_by_pairs": 2 * n_pairs * S,
            "counts_GBps_of_code_bytes": 2 * n_pairs * S / (med(counts_ms) * 1e-3) / 1e9,
            "evaluations_mean": float(out5[:, 4].mean()), "evaluations_max": float(out5[:, 4].max()),
            "numpy_counts_ms_all_pairs_scaled": (t1 - t0) * 1e3 * scale,
            "numpy_brentq_ms_all_pairs_scaled": (t2 - t1) * 1e3 * scale,
            "numpy_sample_pairs": args.ref_pairs,
            "max_rel_distance_difference_on_sample": float(err),
        }
        print(kind, json.dumps(result[kind]))
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
