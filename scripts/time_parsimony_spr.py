"""Time parsimony SPR on the device (pu_parsimony.hip) at the cfg2 shape (50 taxa x
100k DNA sites) and the cfg3 shape (200 taxa x 10k protein sites) of scripts/time_parsimony.py:

* one scoring pass (all SPR neighbours of a tree) for one stepwise-addition tree and for 100 of
  them, beside the code as it stood before: ``fitch_lengths`` on the explicit list of neighbour
  trees, timed on the first --baseline-moves neighbours of one tree and scaled to all of them;
* the full search from 100 stepwise-addition trees: rounds, time, the lengths before and after;
* the optimised lnL a short likelihood ``spr_search`` reaches from the refined tree, from the
  stepwise-only tree and from the BIONJ tree (--lnl-rounds 0 leaves it out).

Wall times and the HIP-event time of the kernels (pu_parsimony_kernel_ms).  Nothing is asserted
but that the baseline's lengths equal the scores.  Writes profiles/parsimony_spr_times.json.

    python scripts/time_parsimony_spr.py [--cfg cfg2,cfg3] [--n-rep 100] [--lnl-rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_parsimony import SHAPES, problem, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg3")
    ap.add_argument("--n-rep", type=int, default=100, dest="n_rep")
    ap.add_argument("--baseline-moves", type=int, default=200, dest="baseline_moves")
    ap.add_argument("--lnl-rounds", type=int, default=5, dest="lnl_rounds")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parsimony_spr_times.json"))
    args = ap.parse_args()
    import parsimony_reference as PR
    from phylo_utils_amd import TreeModel, parsimony
    result = {"reps": args.reps, "warmup": args.warmup, "cases": []}
    parsimony.profile(True)
    for cfg in args.cfg.split(","):
        _, names, codes, table, w, model, rm = problem(cfg)
        n, P = codes.shape
        aln = (codes, table, names)
        case = {"cfg": cfg, "n_taxa": n, "n_sites": SHAPES[cfg][1], "n_patterns": P}
        starts, _, start_len = parsimony.stepwise_addition(
            aln, orders=parsimony.random_orders(n, args.n_rep, 0), weights=w)

        case["scoring_pass"] = []
        for T in sorted({1, args.n_rep}):
            (L, sc), wall, ms = timed(lambda: parsimony.spr_scores(aln, starts[:T], weights=w),
                                      args.reps, args.warmup)
            moves = int((sc != parsimony.SENTINEL).sum())
            row = {"n_trees": T, "neighbours": moves, "call_wall_ms": wall, "kernel_ms": ms,
                   "shorter_neighbours": int((sc < L[:, None, None]).sum())}
            case["scoring_pass"].append(row)
            print(json.dumps({cfg: row}), flush=True)
            if T == 1:
                one = sc[0]
        # the code as it stood: every neighbour tree built on the host and scored from scratch
        pairs = np.argwhere(one != parsimony.SENTINEL)
        pairs = pairs[np.linspace(0, len(pairs) - 1, min(args.baseline_moves, len(pairs)))
                      .astype(int)]
        t0 = time.perf_counter()
        scheds = [PR.edges_schedule(parsimony.apply_spr_edges(starts[0], d, f), n)[:2]
                  for d, f in pairs]
        host_ms = (time.perf_counter() - t0) * 1e3
        got, wall, ms = timed(lambda: parsimony.fitch_lengths(aln, scheds, weights=w),
                              args.reps, args.warmup)
        scale = case["scoring_pass"][0]["neighbours"] / float(len(pairs))
        case["baseline_fitch_lengths"] = {
            "neighbours_timed": len(pairs), "call_wall_ms": wall, "kernel_ms": ms,
            "host_tree_building_ms": host_ms, "kernel_ms_scaled_to_all": ms * scale,
            "call_wall_ms_scaled_to_all": wall * scale,
            "equal": bool(np.array_equal(got, one[pairs[:, 0], pairs[:, 1]]))}
        print(json.dumps({cfg: case["baseline_fitch_lengths"]}), flush=True)

        (edges, lens, rounds), wall, ms = timed(
            lambda: parsimony.spr_search(aln, starts, weights=w), 1, 0)
        case["search"] = {
            "n_trees": len(starts), "call_wall_ms": wall, "kernel_ms": ms,
            "rounds_total": int(rounds.sum()), "rounds_max": int(rounds.max()),
            "shortest_before": int(start_len.min()), "shortest_after": int(lens.min()),
            "mean_before": float(start_len.mean()), "mean_after": float(lens.mean()),
            "never_longer": bool((lens <= start_len).all())}
        print(json.dumps({cfg: case["search"]}), flush=True)

        if args.lnl_rounds > 0:
            case["likelihood_spr_search"] = {}
            for start in ("parsimony_spr", "parsimony", "bionj"):
                tm = TreeModel()
                tm.set_alignment_codes(codes, table, names, siteweights=w)
                tm.set_substitution_model(model)
                tm.set_rate_model(rm)
                t0 = time.perf_counter()
                if start == "bionj":
                    tm.set_nj_tree(method="bionj")
                    plen = tm.parsimony_length()
                else:
                    _, plen, _ = tm.set_parsimony_tree(
                        n_rep=args.n_rep, seed=0, spr_rounds=0 if start == "parsimony_spr" else None)
                tm.initialise()
                tm.optimise_branch_lengths()
                lnl0 = float(tm.likelihood())
                _, lnl, _ = tm.spr_search(max_rounds=args.lnl_rounds)
                case["likelihood_spr_search"][start] = {
                    "parsimony_length_of_start": int(plen), "lnl_start_optimised": lnl0,
                    "lnl_after_spr": float(lnl), "max_rounds": args.lnl_rounds,
                    "wall_s": time.perf_counter() - t0}
                print(json.dumps({cfg: {start: case["likelihood_spr_search"][start]}}), flush=True)
        result["cases"].append(case)
    parsimony.profile(False)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
