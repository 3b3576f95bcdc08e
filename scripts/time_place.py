"""Time the placement kernels and passes against the baseline a user would write today (DESIGN
4.19).

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4), with
Q = 1000 queries.  Reference alignment and queries are ONE draw of TreeModel.simulate down the
tree with 1000 sister leaves attached at the midpoints of random edges (pendant 0.05): the
reference rows are the alignment, the sister rows the queries:

* k_place_table_ms / k_place_prescore_ms / k_place_newton_ms   HIP-event times of one launch on
  the root edge through pu_place_edge (median of --reps; the Newton launch runs all Q queries);
* prescore_GBps     bytes the pre-score kernel gathers (per query and site one 8-byte table
                    entry, one code byte and the 8-byte site weight) over its time, beside
                    write_ceiling_GBps, the box's measured write-stream ceiling
                    (pu_write_ceiling);
* prescore_pass_s   wall time of one pu_place_prescore: every query at every edge, the scores in
                    host arrays and the closing traversal done (median of --sweeps);
* refine_pass_s     wall time of one pu_place_refine at keep = 5 on the pre-score's candidates;
* newton_evaluations_mean   1 + mean Newton steps per candidate (a lower bound on the lnL
                    evaluations: a halved step costs more);
* baseline_*        attach + set_tree + likelihood() on the alignment extended by one row, host
                    wall time per (query, edge) pair (median, with min and max) over a random
                    subset of baseline_pairs pairs, then EXTRAPOLATED to Q * E pairs (the
                    pre-score) and to Q * keep * newton_evaluations_mean evaluations (the
                    refinement).  The baseline is not run at those sizes;
* best_edge_is_planted_fraction   the share of queries whose best refined edge is the edge they
                    were simulated at (a check of the workload, not a timing).

    python scripts/time_place.py [--out profiles/place_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import json
import os
import sys
import time

import ctypes

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import TreeModel  # noqa: E402
from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import place as PL  # noqa: E402
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402
from phylo_utils_amd.tree import Node, Traversal, prepare_tree  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}
KEEP = 5


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def model_of(tree, names, codes, m, rm, device):
    tm = TreeModel(device=device)
    tm.set_alignment_codes(codes, np.eye(len(m.freqs)), names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    return tm


def planted_problem(tree, m, rm, n_query, n_sites, rng, device):
    """(names, reference states [n_taxa][n_sites], query states [Q][n_sites], NOD of every
    query's planted edge in the reference tree's node numbering) from ONE draw down
    the tree with Q sister leaves attached: leaf q<k> hangs on a pendant branch of 0.05 from the
    midpoint of a random edge (several on one edge share the midpoint through zero-length
    links), the reference rows of the draw are the alignment and the q rows the queries."""
    aug = prepare_tree(tree)
    index = dict(Traversal(aug).node_dict)  # before the sisters go in: the model's numbering
    seed = aug.seed_node
    nodes = [n for n in seed.postorder() if n is not seed and n.parent is not seed]
    hits, planted = {}, np.zeros(n_query, dtype=np.int64)
    for k, j in enumerate(rng.integers(0, len(nodes), size=n_query)):
        hits.setdefault(int(j), []).append(k)
        planted[k] = index[nodes[int(j)]]  # NOD of the planted edge
    for j, ks in hits.items():
        child = nodes[j]
        half = 0.5 * child.edge_length
        child.length = half
        for i, k in enumerate(ks):
            par = child.parent
            new = Node(None, half if i == len(ks) - 1 else 0.0)
            par.children[par.children.index(child)] = new
            new.parent = par
            if i:
                child.length = 0.0
            new.add(child)
            new.add(Node("q%d" % k, 0.05))
            child = new
    ref_names = sorted(Traversal(prepare_tree(tree)).names, key=lambda x: int(x[1:]))
    names = ref_names + ["q%d" % k for k in range(n_query)]
    sim = model_of(aug, names, np.zeros((len(names), 1), dtype=np.uint8), m, rm, device)
    states = np.asarray(sim.simulate(n_sites, seed=1), dtype=np.uint8)
    return (ref_names, states[:len(ref_names)], np.ascontiguousarray(states[len(ref_names):]),
            planted)


def measure(name, reps, sweeps, n_query, n_pairs, device):
    shape = SHAPES[name]
    if shape["model"].startswith("GTR"):
        m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    else:
        m, rm = SM.LG(freqs=np.asarray(SM.LG().freqs) / np.sum(SM.LG().freqs)), \
            GammaRateModel(4, 0.8)
    K = len(m.freqs)
    n_sites = shape["n_sites"]
    tree, _, _ = make_problem(shape["n_taxa"], 1, m, rm.rates, seed=1)  # the tree alone
    rng = np.random.default_rng(7)
    names, st, states, planted = planted_problem(tree, m, rm, n_query, n_sites, rng, device)
    tm = model_of(tree, names, st, m, rm, device)
    lnl0 = tm.likelihood()
    q = PL.encode_queries(tm, (["q%d" % k for k in range(n_query)], states, np.eye(K)))
    l0 = PL.default_pendant(tm)

    pre = PL.prescore(tm, q, l0)  # warm-up: buffers, code objects
    E = len(pre["edges"])
    prescore_pass_s = median_time(lambda: PL.prescore(tm, q, l0), sweeps)
    cand = [(e, k) for k, es in enumerate(PL.select_candidates(pre["scores"], KEEP)) for e in es]
    fine = PL.refine(tm, q, cand, E, l0)
    refine_pass_s = median_time(lambda: PL.refine(tm, q, cand, E, l0), sweeps)
    evals = 1.0 + float(np.mean(fine["iters"]))
    best = {}  # query -> (lnL, NOD) of its best refined candidate
    for e, k, lnl in zip(fine["edge_num"], fine["query"], fine["lnl"]):
        if int(k) not in best or lnl > best[int(k)][0]:
            best[int(k)] = (lnl, int(pre["edges"][e][0]))
    found = float(np.mean([best[k][1] == planted[k] for k in range(n_query)]))

    nod, par = (int(v) for v in pre["edges"][0])
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    ms = []
    for _ in range(reps):
        PL.place_edge(tm, q, nod, par, pendant0=l0)
        ms.append(PL.kernel_ms(tm))
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")
    table_ms, prescore_ms, newton_ms = (float(v) for v in np.median(np.array(ms), axis=0))
    # per (query, site): one 8-byte table entry, one code byte and the 8-byte site weight
    gathered = n_query * n_sites * (9.0 + (8.0 if q["site_weight"] is not None else 0.0))
    nbytes = 1 << 30
    ceil_ms = ctypes.c_double()
    N.check(N.lib().pu_write_ceiling(device, nbytes, 10, ctypes.byref(ceil_ms)), None,
            "pu_write_ceiling")

    # the baseline: one joined tree, one extended alignment and one full traversal per pair
    pairs = [(int(rng.integers(n_query)), int(rng.integers(E))) for _ in range(n_pairs)]
    ext = TreeModel(device=device)
    ext.set_substitution_model(m)
    ext.set_rate_model(rm)
    base_tree = PL.current_tree(tm)
    ref_codes = st

    def one(k, e):
        ext.set_alignment_codes(np.concatenate([ref_codes, states[k][None]]), np.eye(K),
                                list(names) + ["query"])
        ext.set_tree(PL.attach(base_tree, pre["edges"][e], "query", l0))
        ext.initialise()
        return ext.likelihood()

    one(*pairs[0])  # warm-up
    diffs, ts = [], []
    for k, e in pairs:
        t0 = time.perf_counter()
        lnl = one(k, e)
        ts.append(time.perf_counter() - t0)
        diffs.append(abs(lnl - pre["scores"][e, k]) / abs(pre["scores"][e, k]))
    per_pair = float(np.median(ts))
    return dict(shape, n_query=n_query, n_edges=E, keep=KEEP, pendant0=l0, lnl=lnl0,
                k_place_table_ms=table_ms, k_place_prescore_ms=prescore_ms,
                k_place_newton_ms=newton_ms, newton_launch_queries=n_query,
                prescore_GBps=gathered / (prescore_ms * 1e-3) / 1e9,
                write_ceiling_GBps=nbytes / (ceil_ms.value * 1e-3) / 1e9,
                prescore_pass_s=prescore_pass_s, refine_pass_s=refine_pass_s,
                n_candidates=len(cand), newton_evaluations_mean=evals,
                baseline_pairs=len(pairs), baseline_s_per_pair=per_pair,
                baseline_s_per_pair_min=float(np.min(ts)), baseline_s_per_pair_max=float(np.max(ts)),
                newton_steps_min=int(fine["iters"].min()), newton_steps_max=int(fine["iters"].max()),
                pendant_median=float(np.median(fine["pendant"])),
                best_edge_is_planted_fraction=found,
                baseline_max_rel_diff=float(max(diffs)),
                baseline_prescore_s_extrapolated=per_pair * n_query * E,
                baseline_refine_s_extrapolated=per_pair * n_query * KEEP * evals,
                note="baseline_*_extrapolated scale the measured time per pair to Q * E and to "
                     "Q * keep * newton_evaluations_mean; the baseline was not run at those "
                     "sizes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "place_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {s: measure(s, args.reps, args.sweeps, args.queries, args.pairs, args.device)
           for s in args.shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
