"""Time the regraft kernel, the SPR scoring pass and the search against the two baselines a user
has without them.

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4), data
one draw of TreeModel.simulate down a random tree:

* k_regraft_ms      HIP-event time of one launch through pu_regraft_edge on three internal nodes
                    (median of --reps);
* regraft_GBps      the bytes that launch gathers (three partials and their scalers per pattern
                    and category) over its time, beside write_ceiling_GBps, the box's measured
                    write-stream ceiling (pu_write_ceiling);
* composition_ms    the same number from two launches, pu_update_partials of the dissolved node's
                    slot + pu_edge_lnl, host wall time per pair of calls (median of --reps), and
                    fused_call_ms, the wall time of one pu_regraft_edge call, its like;
* scores_radius5_s / scores_all_s   wall time of spr_scores(radius=5) and spr_scores(None), rows
                    generated on the host included (rows_*_s is that share), with their move counts;
* composition_all_s_extrapolated    composition_ms x the moves of the full pass (not run);
* baseline_*        apply_spr + set_tree + likelihood() per move, host wall time (median, min,
                    max) over --moves random moves, EXTRAPOLATED to the moves of the full pass;
                    the baseline is not run at that size;
* search_*          one spr_search from the BIONJ tree of the data: rounds, moves taken, lnL before
                    and after, wall time.

    python scripts/time_spr.py [--out profiles/spr_times.json] [--shapes cfg2 cfg3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phylo_utils_amd import TreeModel  # noqa: E402
from phylo_utils_amd import _native as N  # noqa: E402
from phylo_utils_amd import spr as SPR  # noqa: E402
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402
from phylo_utils_amd.tree import apply_spr, spr_rows, with_lengths  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}


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
    if tree is not None:
        tm.set_tree(tree)
        tm.initialise()
    return tm


def measure(name, reps, n_moves, search_rounds, search_radius, device):
    shape = SHAPES[name]
    if shape["model"].startswith("GTR"):
        m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    else:
        m, rm = SM.LG(freqs=np.asarray(SM.LG().freqs) / np.sum(SM.LG().freqs)), \
            GammaRateModel(4, 0.8)
    K, C = len(m.freqs), rm.ncat
    tree, _, _ = make_problem(shape["n_taxa"], 1, m, rm.rates, seed=1)  # the tree alone
    names = ["t%d" % i for i in range(shape["n_taxa"])]
    sim = model_of(tree, names, np.zeros((len(names), 1), dtype=np.uint8), m, rm, device)
    states = np.asarray(sim.simulate(shape["n_sites"], seed=1), dtype=np.uint8)
    tm = model_of(tree, names, states, m, rm, device)
    lnl0 = tm.likelihood()
    S = tm._n_patterns()
    tr = tm.traversal
    rng = np.random.default_rng(7)

    # one launch, on the root edge's first candidate
    rows, off, inner, lens, table = spr_rows(tr, 0)
    first = int(np.flatnonzero(inner[:, 3] >= 0)[0])
    a, b, s = (int(z) for z in inner[first][3:])
    n, o = int(table[first][0]), int(table[first][1])
    t, l = float(lens[first][2]), float(lens[first][3])
    SPR.regraft_edge(tm, a, b, s, t, l)  # warm-up
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    ms = []
    for _ in range(reps):
        SPR.regraft_edge(tm, a, b, s, t, l)
        ms.append(SPR.kernel_ms(tm))
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")
    regraft_ms = float(np.median(ms))
    fused_call_ms = 1e3 * median_time(lambda: SPR.regraft_edge(tm, a, b, s, t, l), reps)
    gathered = 3.0 * S * C * (K + 1) * 8
    nbytes = 1 << 30
    ceil_ms = ctypes.c_double()
    N.check(N.lib().pu_write_ceiling(device, nbytes, 10, ctypes.byref(ceil_ms)), None,
            "pu_write_ceiling")
    # the two-launch composition of the same number (o is a root-edge end: its post-order
    # partial comes back with compute_partials)
    lnl = ctypes.c_double()
    op = np.array([[o, a, b]], dtype=np.int32)
    bl = np.array([[0.5 * t, 0.5 * t]])

    def composed():
        N.check(N.lib().pu_update_partials(tm._ctx, 1, N.ptr(op), N.ptr(bl)), tm._ctx, "update")
        N.check(N.lib().pu_edge_lnl(tm._ctx, n, o, ctypes.byref(lnl), None), tm._ctx, "edge_lnl")

    fused = SPR.regraft_edge(tm, a, b, s, t, l)
    composed()
    composition_rel_diff = abs(lnl.value - fused) / abs(fused)
    composition_ms = 1e3 * median_time(composed, reps)
    tm.compute_partials()

    # the scoring passes
    def timed_scores(radius):
        t0 = time.perf_counter()
        r = spr_rows(tr, radius)
        t1 = time.perf_counter()
        sc, _ = SPR.sweep(tm, *r[:4])
        t2 = time.perf_counter()
        return t1 - t0, t2 - t0, r[4][r[2][:, 3] >= 0], sc[r[2][:, 3] >= 0]

    timed_scores(1)  # warm-up
    rows5_s, scores5_s, moves5, _ = timed_scores(5)
    rows_all_s, scores_all_s, moves, scores = timed_scores(None)

    # the baseline: one rearranged tree and one full traversal per move
    base = with_lengths(tm.tree, tr.brlens)
    ext = model_of(None, names, states, m, rm, device)
    picks = rng.choice(len(moves), size=min(n_moves, len(moves)), replace=False)

    def one(i):
        ext.set_tree(apply_spr(base, *(int(z) for z in moves[i][:4])))
        ext.initialise()
        return ext.likelihood()

    one(int(picks[0]))  # warm-up
    ts, diffs = [], []
    for i in picks:
        t0 = time.perf_counter()
        v = one(int(i))
        ts.append(time.perf_counter() - t0)
        diffs.append(abs(v - scores[i]) / abs(v))
    per_move = float(np.median(ts))

    # one search from the BIONJ tree of the data
    st = model_of(None, names, states, m, rm, device)
    st.set_nj_tree(method="bionj")
    st.initialise()
    t0 = time.perf_counter()
    _, lnl_end, history = st.spr_search(radius=search_radius, max_rounds=search_rounds)
    search_s = time.perf_counter() - t0
    return dict(shape, n_patterns=int(S), lnl=lnl0, k_regraft_ms=regraft_ms,
                regraft_GBps=gathered / (regraft_ms * 1e-3) / 1e9,
                write_ceiling_GBps=nbytes / (ceil_ms.value * 1e-3) / 1e9,
                fused_call_ms=fused_call_ms, composition_ms=composition_ms,
                composition_over_fused=composition_ms / fused_call_ms,
                composition_rel_diff=composition_rel_diff,
                moves_radius5=int(len(moves5)), moves_all=int(len(moves)),
                rows_radius5_s=rows5_s, scores_radius5_s=scores5_s, rows_all_s=rows_all_s,
                scores_all_s=scores_all_s,
                composition_all_s_extrapolated=composition_ms * 1e-3 * len(moves),
                baseline_moves=int(len(picks)), baseline_s_per_move=per_move,
                baseline_s_per_move_min=float(np.min(ts)), baseline_s_per_move_max=float(np.max(ts)),
                baseline_max_rel_diff=float(max(diffs)),
                baseline_all_s_extrapolated=per_move * len(moves),
                baseline_over_scores_all=per_move * len(moves) / scores_all_s,
                search_radius=search_radius, search_max_rounds=search_rounds,
                search_rounds=len(history),
                search_moves=sum(1 for h in history if h["move"] is not None),
                search_lnl_start=history[0]["before"] if history else lnl_end,
                search_lnl_end=lnl_end, search_s=search_s,
                note="*_extrapolated scale a measured time per move to the moves of the full "
                     "pass; neither baseline was run at that size")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "spr_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--search-rounds", type=int, default=50)
    ap.add_argument("--search-radius", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {}
    if os.path.exists(args.out):  # shapes may be measured one call at a time
        with open(args.out) as fh:
            res = json.load(fh)
    for s in args.shapes:
        res[s] = measure(s, args.reps, args.moves, args.search_rounds, args.search_radius,
                         args.device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
