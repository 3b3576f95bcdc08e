"""Time Fitch parsimony on the device (pu_parsimony.hip) against the numpy
restatement of its rule (tests/parsimony_reference.py) on the same inputs, at the cfg2 shape (50
taxa x 100k DNA sites) and the cfg3 shape (200 taxa x 10k protein sites), both simulated down a
random tree and compressed to site patterns:

* one tree's length (the generating tree);
* the Q x E insertion table for 1000 queries (the restatement on the first --ref-queries of them,
  scaled);
* stepwise addition with n_rep = 1 and 100 random orders (the restatement on the first order,
  scaled);
* the optimised lnL that spr_search reaches from the shortest parsimony tree and from the BIONJ
  tree (--spr-rounds 0 leaves it out).

Per item: the call's wall time (median over --reps after --warmup; stepwise addition once), the
HIP-event time of its kernels (pu_parsimony_kernel_ms), the restatement's wall time, and whether
the two agree exactly.  Nothing is asserted.  Writes profiles/parsimony_times.json.

    python scripts/time_parsimony.py [--cfg cfg2,cfg3] [--n-rep 1,100] [--spr-rounds 5]
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

SHAPES = {"cfg2": (50, 100000, "dna"), "cfg3": (200, 10000, "protein")}


def problem(cfg):
    from phylo_utils_amd import alignment as A
    from phylo_utils_amd import substitution_models as SM
    from phylo_utils_amd.rate_models import GammaRateModel
    from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem
    n, S, kind = SHAPES[cfg]
    model = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS) if kind == "dna" else SM.LG()
    rm = GammaRateModel(4, 0.5)
    tree, names, states = make_problem(n, S, model, rm.rates, seed=n)
    K = len(model.freqs)
    codes, weights, _ = A.compress_codes(states.astype(np.uint8), K)
    return tree, names, codes, np.eye(K), weights.astype(np.int64), model, rm


def timed(fn, reps, warmup):
    from phylo_utils_amd import parsimony
    wall, ms, out = [], [], None
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            wall.append(dt)
            ms.append(parsimony.kernel_ms())
    return out, float(np.median(wall)), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg3")
    ap.add_argument("--n-rep", default="1,100", dest="n_rep")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--ref-queries", type=int, default=5, dest="ref_queries")
    ap.add_argument("--spr-rounds", type=int, default=5, dest="spr_rounds")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parsimony_times.json"))
    args = ap.parse_args()
    import parsimony_reference as PR
    from phylo_utils_amd import TreeModel, parsimony
    result = {"reps": args.reps, "warmup": args.warmup, "cases": []}
    parsimony.profile(True)
    for cfg in args.cfg.split(","):
        tree, names, codes, table, w, model, rm = problem(cfg)
        n, P = codes.shape
        aln = (codes, table, names)
        S = PR.tip_sets(codes, table)
        ops, root, _ = parsimony.tree_schedule(tree, names)
        edges = PR.schedule_edges(ops, root)
        case = {"cfg": cfg, "n_taxa": n, "n_sites": SHAPES[cfg][1], "n_patterns": P}

        got, wall, ms = timed(lambda: parsimony.fitch_lengths(aln, (ops, root), weights=w),
                              args.reps, args.warmup)
        t0 = time.perf_counter()
        ref = PR.lengths(edges, S, w)
        case["length"] = {"value": got, "call_wall_ms": wall, "kernel_ms": ms,
                          "numpy_restatement_ms": (time.perf_counter() - t0) * 1e3,
                          "equal": bool(got == ref)}
        print(json.dumps({cfg: case["length"]}), flush=True)

        rng = np.random.default_rng(1)
        q = codes[rng.integers(n, size=args.queries)].copy()
        flip = rng.random(q.shape) < 0.1
        q[flip] = rng.integers(len(table), size=int(flip.sum()))
        got, wall, ms = timed(lambda: parsimony.insertion_lengths(aln, (ops, root), q, weights=w),
                              args.reps, args.warmup)
        nq = min(args.ref_queries, args.queries)
        t0 = time.perf_counter()
        ref = PR.insertion_lengths(edges, S, PR.tip_sets(q[:nq], table), w)
        ref_ms = (time.perf_counter() - t0) * 1e3
        case["insertion"] = {"n_query": args.queries, "n_edges": 2 * n - 3, "call_wall_ms": wall,
                             "kernel_ms": ms, "numpy_restatement_ms_scaled":
                             ref_ms * args.queries / nq, "numpy_queries_timed": nq,
                             "equal": bool([[int(x) for x in r] for r in got[:nq]] == ref)}
        print(json.dumps({cfg: case["insertion"]}), flush=True)

        case["stepwise"] = []
        best = None
        for R in [int(x) for x in args.n_rep.split(",")]:
            orders = parsimony.random_orders(n, R, 0)
            (e, steps, lens), wall, ms = timed(
                lambda: parsimony.stepwise_addition(aln, orders=orders, weights=w), 1, 0)
            t0 = time.perf_counter()
            ref = PR.stepwise(S, orders[0], w)
            ref_ms = (time.perf_counter() - t0) * 1e3
            row = {"n_rep": R, "call_wall_ms": wall, "kernel_ms": ms,
                   "numpy_restatement_ms_scaled": ref_ms * R, "shortest": int(lens.min()),
                   "longest": int(lens.max()),
                   "equal_first_order": bool(np.array_equal(e[0], ref["edges"])
                                             and int(lens[0]) == ref["length"])}
            case["stepwise"].append(row)
            best = (R, e[int(np.argmin(lens))])
            print(json.dumps({cfg: row}), flush=True)

        if args.spr_rounds > 0:
            case["spr_search"] = {}
            for start in ("parsimony", "bionj"):
                tm = TreeModel()
                tm.set_alignment_codes(codes, table, names, siteweights=w)
                tm.set_substitution_model(model)
                tm.set_rate_model(rm)
                t0 = time.perf_counter()
                if start == "parsimony":
                    _, plen, _ = tm.set_parsimony_tree(n_rep=best[0], seed=0)
                else:
                    tm.set_nj_tree(method="bionj")
                    plen = tm.parsimony_length()
                tm.initialise()
                tm.optimise_branch_lengths()
                lnl0 = float(tm.likelihood())
                _, lnl, _ = tm.spr_search(max_rounds=args.spr_rounds)
                case["spr_search"][start] = {
                    "parsimony_length_of_start": int(plen), "lnl_start_optimised": lnl0,
                    "lnl_after_spr": float(lnl), "max_rounds": args.spr_rounds,
                    "wall_s": time.perf_counter() - t0}
                print(json.dumps({cfg: {start: case["spr_search"][start]}}), flush=True)
        result["cases"].append(case)
    parsimony.profile(False)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
