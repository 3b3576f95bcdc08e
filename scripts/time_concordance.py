"""Time the site concordance factors on the device (pu_scf.hip) at Q = 100 quartets
per branch on random trees and random alignments with a little signal: 50 taxa x 100 000 DNA
columns, 200 taxa x 10 000 protein columns and 1000 taxa x 1 000 000 DNA columns (unit weights,
every column its own pattern):

* k_scf_counts with each of its two feeds (PU_SCF_FEED=global: the rows read from memory;
  PU_SCF_FEED=lds: the pattern tile of all rows staged in LDS, where n <= 296 lets them fit), the
  pick kernel and the state-byte kernel by HIP events (pu_scf_kernel_ms), and the wall time of the
  whole call ``concordance.site_concordance`` (upload, kernels, read-back, the float64 finish);
* the numpy restatement tests/concordance_reference.py on the picks and counts of --host-branches
  internal branches, its wall time scaled to all n - 3 branches: an estimate, said to be scaled.

Medians of --reps runs after --warmup.  Nothing is asserted but that both feeds agree with each
other everywhere and with the restatement on the branches it was run on.  Writes
profiles/concordance_times.json.

    python scripts/time_concordance.py [--shapes 50x100000x4,200x10000x20] [--reps 5] [--out FILE]
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

SHAPES = "50x100000x4,200x10000x20,1000x1000000x4"


def make_case(n, P, K, seed):
    import parsimony_reference as PR
    rng = np.random.default_rng(seed)
    edges = np.array(PR.random_edges(rng, n), dtype=np.int32)
    table = np.vstack([np.eye(K), np.ones((1, K))])  # the states and a gap
    base = rng.integers(K, size=P, dtype=np.uint8)
    codes = np.empty((n, P), dtype=np.uint8)
    for r in range(n):  # row by row: the largest shape is a gigabyte
        row = np.where(rng.random(P) < 0.3, rng.integers(K, size=P, dtype=np.uint8), base)
        codes[r] = np.where(rng.random(P) < 0.02, np.uint8(K), row)
    return edges, codes, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="taxa x patterns x states, comma-separated")
    ap.add_argument("--quartets", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-branches", type=int, default=2, dest="host_branches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concordance_times.json"))
    args = ap.parse_args()

    import concordance_reference as CR
    from phylo_utils_amd import _native as N
    from phylo_utils_amd import concordance
    if N.device_count() < 1:
        raise SystemExit("time_concordance.py: no HIP device")
    Q = args.quartets
    results = []
    for shape in args.shapes.split(","):
        n, P, K = (int(x) for x in shape.split("x"))
        edges, codes, table = make_case(n, P, K, n + P)
        names = ["t%d" % i for i in range(n)]
        row = dict(n_taxa=n, n_patterns=P, n_states=K, n_quartets=Q, branches=n - 3,
                   quartet_patterns=float(n - 3) * Q * P)
        last = {}
        concordance.profile(True)
        try:
            for feed in ("global", "lds"):
                os.environ["PU_SCF_FEED"] = feed
                walls, ms = [], []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r = concordance.site_concordance((codes, table, names), edges, n_quartets=Q,
                                                     seed=1)
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= args.warmup:
                        walls.append(dt)
                        ms.append(concordance.kernel_ms())
                last[feed] = r
                picks, states, counts = np.median(np.array(ms), axis=0)
                row[feed] = dict(picks_ms=float(picks), states_ms=float(states),
                                 counts_ms=float(counts), call_wall_ms=float(np.median(walls)),
                                 counts_ms_runs=[float(m[2]) for m in ms])
            row["lds"]["staged_in_lds"] = bool(n <= 296)  # else the call fell back to the rows in memory
        finally:
            concordance.profile(False)
            os.environ.pop("PU_SCF_FEED", None)
        assert np.array_equal(last["global"].counts, last["lds"].counts)
        assert np.array_equal(last["global"].taxa, last["lds"].taxa)
        # the restatement on a few branches, scaled
        r = last["global"]
        some = [int(e) for e in r.internal[:args.host_branches]]
        nq = np.zeros_like(r.nq)
        nq[some] = r.nq[some]
        t0 = time.perf_counter()
        ref_nq, ref_taxa = CR.quartets(edges, Q, 1)
        t_picks = time.perf_counter() - t0
        assert np.array_equal(ref_nq, r.nq) and np.array_equal(ref_taxa, r.taxa)
        t0 = time.perf_counter()
        ref_counts = CR.counts(codes, table, None, nq, ref_taxa)
        t_counts = time.perf_counter() - t0
        assert np.array_equal(ref_counts[some], r.counts[some])
        row["numpy"] = dict(branches_run=len(some), picks_s=t_picks,
                            counts_s_scaled=t_counts * (n - 3) / len(some),
                            note="counts timed on %d of %d branches and scaled; picks on all"
                                 % (len(some), n - 3))
        if row["lds"]["staged_in_lds"]:
            row["faster_feed"] = min(("global", "lds"), key=lambda f: row[f]["counts_ms"])
        else:  # both runs read the rows from memory: there is one feed at this shape
            row["faster_feed"] = "global (the rows of %d taxa do not fit in LDS)" % n
        results.append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="site concordance factors, DESIGN 4.29; medians of %d runs after %d"
                            % (args.reps, args.warmup), shapes=results), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
