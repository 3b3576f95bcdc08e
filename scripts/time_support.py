"""Time the branch-support pass and its two kernels against what the library offered before
(DESIGN 4.17).

For cfg2 (50 taxa x 100k DNA sites, GTR+G4) and cfg3 (200 taxa x 10k protein sites, LG+G4), with
R = --replicates (1000) RELL replicates:

* k_quartet_ms / k_quartet_sites_ms   HIP-event time of one plain k_quartet launch and of one
                  k_quartet<K, true> launch, which also stores the per-pattern lnL (medians of
                  --reps launches);
* rell_ms         HIP-event time of pu_rell_sums_device on (R + 1) x S weights and 3 (N - 3)
                  vectors (median of --reps), with its flop and byte counts (W and L read once,
                  the segment sums written and read), the achieved rates and the device peaks;
* weights_ms      HIP-event time of pu_boot_weights_device for the R rows;
* numpy_matmul_s  host wall time of W.astype(float) @ L.T on the same arrays, and the largest
                  difference of the two products relative to sum |W L|;
* support_s / nni_scores_s   wall time of TreeModel.branch_support(R) beside nni_scores();
* baseline_s      wall time of set_tree + initialise + likelihood() + sitewise_patterns() of each
                  of the 2 (N - 3) neighbour topologies at unchanged lengths, plus numpy_matmul_s:
                  what a user could do before.

    python scripts/time_support.py [--out profiles/support_times.json] [--shapes cfg2 cfg3]
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
from phylo_utils_amd import substitution_models as SM  # noqa: E402
from phylo_utils_amd.rate_models import GammaRateModel  # noqa: E402
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES, make_problem  # noqa: E402
from phylo_utils_amd.tree import apply_nni  # noqa: E402

SHAPES = {
    "cfg2": dict(n_taxa=50, n_sites=100000, model="GTR+G4"),
    "cfg3": dict(n_taxa=200, n_sites=10000, model="LG+G4"),
}
# MI355X: fp64 vector peak and HBM3E bandwidth (AMD's product brief)
PEAK_FP64_FLOPS = 78.6e12
PEAK_HBM_BYTES = 8.0e12
SEGMENT = 2048  # pu_rell.hip kSeg


def _kernel_ms(tm, call, reps):
    ms = []
    for _ in range(reps):
        call()
        v = ctypes.c_double()
        N.check(N.lib().pu_quartet_kernel_ms(tm._ctx, ctypes.byref(v)), tm._ctx)
        ms.append(v.value)
    return float(np.median(ms))


def measure(name, reps, R, device):
    import torch
    shape = SHAPES[name]
    if shape["model"].startswith("GTR"):
        m, rm = SM.GTR(CFG2_GTR_RATES, CFG2_FREQS), GammaRateModel(4, 0.5)
    else:
        m, rm = SM.LG(), GammaRateModel(4, 0.8)
    tree, names, st = make_problem(shape["n_taxa"], shape["n_sites"], m, rm.rates, seed=1)
    tm = TreeModel(device=device)
    tm.set_alignment_codes(st.astype(np.uint8), np.eye(len(m.freqs)), names)
    tm.set_substitution_model(m)
    tm.set_rate_model(rm)
    tm.set_tree(tree)
    tm.initialise()
    lnl0 = tm.likelihood()
    S = shape["n_sites"]

    tm.nni_scores()  # warm-up: buffers, code objects
    tm.branch_support(n_replicates=8)
    t0 = time.perf_counter()
    quartets, scores = tm.nni_scores()
    nni_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    q2, s2, sup = tm.branch_support(n_replicates=R)
    support_s = time.perf_counter() - t0
    assert np.array_equal(q2, quartets) and np.array_equal(s2, scores)

    # one launch of each build of the quartet kernel, on the first scored quartet
    q = quartets[0]
    tr = tm.traversal
    lens = [tr.brlens[int(q[2]), int(q[0])], tr.brlens[int(q[3]), int(q[0])],
            max(tr.brlens[int(q[4]), int(q[1])], 1e-8), max(tr.brlens[int(q[5]), int(q[1])], 1e-8),
            tr.brlens[int(q[0]), int(q[1])]]
    N.check(N.lib().pu_ctx_profile(tm._ctx, 1), tm._ctx, "pu_ctx_profile")
    plain_ms = _kernel_ms(tm, lambda: tm.quartet_derivatives(q[2:], lens), reps)
    sites_ms = _kernel_ms(tm, lambda: tm.quartet_site_lnl(q[2:], lens), reps)
    N.check(N.lib().pu_ctx_profile(tm._ctx, 0), tm._ctx, "pu_ctx_profile")

    # the RELL launch alone: R + 1 rows against 3 (N - 3) vectors, HIP events on torch's stream
    dev = torch.device("cuda", device)
    V = 3 * len(quartets)
    rng = np.random.default_rng(0)
    L = -rng.gamma(2.0, 3.0, (V, S))
    d_L = torch.from_numpy(L).to(dev)
    d_W = torch.ones((R + 1, S), dtype=torch.int32, device=dev)
    d_out = torch.zeros((R + 1, V), dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ms = []
        for _ in range(reps):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(ms))

    row1 = ctypes.c_void_p(d_W.data_ptr() + 4 * S)
    weights_ms = timed(lambda: N.check(N.lib().pu_boot_weights_device(
        device, stream, 7, 0, R, S, None, row1, S), None, "pu_boot_weights_device"))
    rell_ms = timed(lambda: N.check(N.lib().pu_rell_sums_device(
        device, stream, V, S, p(d_L), S, R + 1, p(d_W), S, p(d_out), V), None,
        "pu_rell_sums_device"))
    W = d_W.cpu().numpy().astype(np.uint32)
    got = d_out.cpu().numpy()
    t0 = time.perf_counter()
    ref = W.astype(np.float64) @ L.T
    numpy_s = time.perf_counter() - t0
    rell_err = float(np.max(np.abs(got - ref) / (W.astype(np.float64) @ np.abs(L).T)))
    n_seg = (S + SEGMENT - 1) // SEGMENT
    flops = 2.0 * (R + 1) * S * V
    nbytes = 4.0 * (R + 1) * S * ((V + 47) // 48) + 8.0 * V * S * ((R + 128) // 128) \
        + 8.0 * (R + 1) * V * (2 * n_seg + 1 if n_seg > 1 else 1)

    # the baseline: a traversal and the sitewise lnL per neighbour topology, unchanged lengths
    cand = [apply_nni(tree, int(e[0]), int(e[1]), k) for e in quartets for k in (1, 2)]
    tm.set_tree(cand[0])
    tm.initialise()  # warm-up of the re-bind path
    t0 = time.perf_counter()
    for c in cand:
        tm.set_tree(c)
        tm.initialise()
        tm.likelihood()
        tm.sitewise_patterns()
    trees_s = time.perf_counter() - t0
    return dict(shape, n_replicates=R, n_internal_edges=len(quartets), n_vectors=V, lnl=lnl0,
                k_quartet_ms=plain_ms, k_quartet_sites_ms=sites_ms, weights_ms=weights_ms,
                rell_ms=rell_ms, rell_flops=flops, rell_bytes=nbytes,
                rell_flops_per_s=flops / (rell_ms * 1e-3), rell_bytes_per_s=nbytes / (rell_ms * 1e-3),
                peak_fp64_flops_per_s=PEAK_FP64_FLOPS, peak_hbm_bytes_per_s=PEAK_HBM_BYTES,
                numpy_matmul_s=numpy_s, rell_vs_numpy=numpy_s / (rell_ms * 1e-3),
                rell_max_rel_diff_vs_numpy=rell_err, nni_scores_s=nni_s, support_s=support_s,
                baseline_trees_s=trees_s, baseline_s=trees_s + numpy_s,
                ratio=(trees_s + numpy_s) / support_s,
                min_abayes=float(sup["abayes"].min()), min_sh_alrt=float(sup["sh_alrt"].min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "support_times.json"))
    ap.add_argument("--shapes", nargs="+", default=sorted(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {s: measure(s, args.reps, args.replicates, args.device) for s in args.shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
