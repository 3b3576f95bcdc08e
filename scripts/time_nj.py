"""Time neighbour joining on the device (pu_nj.hip) against the numpy restatement of its rule
(tests/nj_reference.py) on the same matrices.

Device: pu_nj_device on resident matrices, HIP events around the call; warm-ups first, then the
median over the repeats.  Tier A (one workgroup per matrix, the matrix in LDS) at n = 50 and
n = 200, one matrix and a batch of 64; tier B (the matrix in memory, two launches per join) at
n = 200 and n = 1000.  Classic NJ throughout (BIONJ's two matrices fit tier A only up to
nj.max_lds_n("bionj")); BIONJ is timed beside it where it fits.  The restatement's wall time is
taken once per matrix (of a batch: on its first matrix, times the batch).  The largest deviation
of the device's lengths and criterion from the restatement's is recorded too.  Writes
profiles/nj_times.json.

    python scripts/time_nj.py [--reps 10] [--warmup 3]
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

CASES = [  # tier, n, batch
    ("A", 50, 1), ("A", 50, 64), ("A", 200, 1), ("A", 200, 64), ("B", 200, 1), ("B", 1000, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nj_times.json"))
    args = ap.parse_args()
    import torch
    import nj_reference as NR
    from phylo_utils_amd import nj
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "tier_a_max_n": {m: nj.max_lds_n(m) for m in ("nj", "bionj")}, "cases": []}
    ref_cache = {}
    worst = 0.0
    for tier, n, batch in CASES:
        for method in ("nj", "bionj"):
            if tier == "A" and n > nj.max_lds_n(method):
                continue
            os.environ["PU_NJ_TIER"] = tier
            Ds = np.stack([NR.perturbed_additive(10 * n + b, n) for b in range(batch)])
            d_D = torch.from_numpy(Ds).to(dev)
            d_joins = torch.zeros((batch, n - 2, 2), dtype=torch.int32, device=dev)
            d_lens = torch.zeros((batch, n - 2, 2), dtype=torch.float64, device=dev)
            d_root = torch.zeros((batch, 2), dtype=torch.int32, device=dev)
            d_rl = torch.zeros(batch, dtype=torch.float64, device=dev)
            d_q = torch.zeros((batch, n - 3), dtype=torch.float64, device=dev)
            ms, wall = [], []
            for it in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                e0.record()
                nj.nj_device(stream, d_D.data_ptr(), n, n, d_joins.data_ptr(), d_lens.data_ptr(),
                             d_root.data_ptr(), d_rl.data_ptr(), d_q.data_ptr(), method=method,
                             n_mat=batch)
                e1.record()
                torch.cuda.synchronize(dev)
                if it >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(e0.elapsed_time(e1))
            key = (n, method)
            if key not in ref_cache:  # the first matrix is the same for every batch size
                t0 = time.perf_counter()
                ref = NR.nj(Ds[0], method, gaps=False)
                ref_cache[key] = (ref, (time.perf_counter() - t0) * 1e3)
            ref, ref_ms = ref_cache[key]
            joins, lens = d_joins.cpu().numpy()[0], d_lens.cpu().numpy()[0]
            same = bool(np.array_equal(joins, ref["joins"])
                        and np.array_equal(d_root.cpu().numpy()[0], ref["root"]))
            dev_max = max(float(np.abs(lens - ref["lens"]).max()),
                          abs(float(d_rl.cpu()[0]) - ref["root_len"]),
                          float(np.abs(d_q.cpu().numpy()[0] - ref["q"]).max()))
            worst = max(worst, dev_max)
            case = {"tier": tier, "n": n, "batch": batch, "method": method,
                    "event_ms_median": float(np.median(ms)), "event_ms_all": ms,
                    "call_wall_ms_median": float(np.median(wall)),
                    "numpy_restatement_ms": ref_ms * batch,
                    "numpy_restatement_ms_one_matrix": ref_ms,
                    "same_joins_as_restatement": same,
                    "largest_deviation_from_restatement": dev_max}
            result["cases"].append(case)
            print(json.dumps({k: v for k, v in case.items() if k != "event_ms_all"}))
    os.environ.pop("PU_NJ_TIER", None)
    result["largest_deviation_seen"] = worst
    b1000 = [c for c in result["cases"] if c["tier"] == "B" and c["n"] == 1000
             and c["method"] == "nj"][0]
    result["tier_b_n1000_event_ms_not_above_numpy_ms"] = bool(
        b1000["event_ms_median"] <= b1000["numpy_restatement_ms"])
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
